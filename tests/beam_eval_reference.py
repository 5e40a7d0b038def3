"""CPU restatement of the definitions of `parseq_eval_beams`, plain Python over lists, and the generator of the
synthetic N-bests the operator is tested on.

Definitions.  A slot is live iff its score is not -inf; its live rank is the number of live slots before it in its image.  The string of a
hypothesis: its first `lengths` tokens (clamped to [0, min(T, 32)]), ids outside the head's classes and <eos> dropped, the rest through the
test-charset adapter.  Per live hypothesis {m, n, distance, exact} and distance / max(m, n, 1); per image the top-1 (the first live slot; no
live slot: the empty string, confidence 0, never correct), the live rank of the first exact hypothesis, the smallest distance and ned."""
import math

from parseq_amd.system import edit_distance

MAX_BEAMS, MAX_TOKENS, NO_HIT = 17, 32, -1
NEG_INF = float('-inf')
INT_NAMES = ('num_samples', 'correct', 'label_length', 'top1_distance', 'oracle_correct', 'oracle_distance', 'live', 'miss')
FLOAT_NAMES = ('ned', 'confidence', 'oracle_ned')


def hypothesis_string(ids, length, steps, tokenizer, adapter):
    classes = len(tokenizer) - 2
    keep = min(max(int(length), 0), min(steps, MAX_TOKENS))
    return adapter(''.join(tokenizer._itos[i] for i in ids[:keep] if 0 <= i < classes and i != tokenizer.eos_id))


def evaluate_slots(slots, labels):
    """`slots[b]`: image b's W slots, None for a dead one, else (adapted string, confidence score)."""
    out = dict(hyp_rows=[], hyp_ned=[], image_rows=[], image_ned=[], image_oracle_ned=[], image_confidence=[], first_hit=[0] * MAX_BEAMS)
    for image, gt in zip(slots, labels):
        n = len(gt)
        rows = []
        for slot in image:
            if slot is None:
                out['hyp_rows'].append([-1, -1, -1, 0]); out['hyp_ned'].append(-1.0)
                continue
            d = edit_distance(slot[0], gt)
            ned = d / max(len(slot[0]), n, 1)
            out['hyp_rows'].append([len(slot[0]), n, d, int(slot[0] == gt)]); out['hyp_ned'].append(ned)
            rows.append((len(slot[0]), d, ned, slot[0] == gt, slot[1], len(out['hyp_rows']) - 1))
        if rows:
            m, d, ned, exact, score, at = rows[0]
            hits = [rank for rank, r in enumerate(rows) if r[3]]
            image_row = [m, n, d, int(exact), hits[0] if hits else NO_HIT, min(r[1] for r in rows), len(rows), at % len(image)]
            ned_pair, conf = (ned, min(r[2] for r in rows)), math.exp(score)
        else:
            image_row = [0, n, n, 0, NO_HIT, n, 0, -1]
            ned_pair, conf = (n / max(n, 1),) * 2, 0.0
        out['image_rows'].append(image_row)
        out['image_ned'].append(ned_pair[0]); out['image_oracle_ned'].append(ned_pair[1]); out['image_confidence'].append(conf)
        if image_row[4] != NO_HIT:
            out['first_hit'][image_row[4]] += 1
    rows = out['image_rows']
    out['totals'] = dict(num_samples=len(rows), correct=sum(r[3] for r in rows), label_length=sum(r[0] for r in rows), top1_distance=sum(r[2] for r in rows),
                         oracle_correct=sum(r[4] != NO_HIT for r in rows), oracle_distance=sum(r[5] for r in rows), live=sum(r[6] for r in rows),
                         miss=sum(r[4] == NO_HIT for r in rows), ned=math.fsum(out['image_ned']), confidence=math.fsum(out['image_confidence']),
                         oracle_ned=math.fsum(out['image_oracle_ned']))
    return out


def evaluate(tokens, scores, lengths, conf_scores, labels, tokenizer, adapter):
    """tokens [B][W][T], scores / lengths / conf_scores [B][W] as nested lists, labels [B] strings."""
    slots = [[None if s == NEG_INF else (hypothesis_string(ids, k, len(ids), tokenizer, adapter), c) for ids, s, k, c in zip(*image)]
             for image in zip(tokens, scores, lengths, conf_scores)]
    return evaluate_slots(slots, labels)


def evaluate_strings(beams, labels, adapter, width):
    """The same over `tokenizer.decode_beams`' output (live hypotheses only, best first, (string, score)): dead slots come last."""
    return evaluate_slots([[(adapter(s), score) for s, score in alts] + [None] * (width - len(alts)) for alts in beams], labels)


def add_totals(parts):
    total = {k: (math.fsum(p['totals'][k] for p in parts) if k in FLOAT_NAMES else sum(p['totals'][k] for p in parts)) for k in INT_NAMES + FLOAT_NAMES}
    total['first_hit'] = [sum(p['first_hit'][k] for p in parts) for k in range(MAX_BEAMS)]
    return total


def coverage_holds(ref, width):
    """The condition of the tests with W >= 2: misses occur, the exact hits stand at min(W, B) different ranks at least, and some image's list
    holds a hypothesis nearer than its top-1."""
    images = len(ref['image_rows'])
    return (ref['totals']['miss'] > 0 and sum(c > 0 for c in ref['first_hit']) >= min(width, images)
            and any(r[5] < r[2] for r in ref['image_rows']))


def kinds_present(case, ref, tokenizer, adapter):
    """Every row kind the synthetic cases promise for W >= 2 is there: dead slots before live ones, an image of dead slots only, live
    hypotheses of length 0, strings the adapter drops whole, hypotheses of one image that differ in their tokens and are equal after the
    adapter, near misses at distance 1 - 3, ids outside the classes inside a hypothesis, lengths below 0, of T and above T."""
    tokens, scores, lengths, _, _ = case
    steps, classes = len(tokens[0][0]), len(tokenizer) - 2
    live = [[s != NEG_INF for s in row] for row in scores]
    read = lambda ids, k: tuple(ids[:min(max(k, 0), steps, MAX_TOKENS)])
    flat = [(ids, k) for rows, ks, on in zip(tokens, lengths, live) for ids, k, o in zip(rows, ks, on) if o]
    dropped_whole = any(any(0 < i < classes for i in read(ids, k)) and not hypothesis_string(ids, k, steps, tokenizer, adapter) for ids, k in flat)
    folded = False
    for rows, ks, on in zip(tokens, lengths, live):
        seen = {}
        for ids, k, o in zip(rows, ks, on):
            if o:
                text = hypothesis_string(ids, k, steps, tokenizer, adapter)
                folded = folded or (bool(text) and any(other != read(ids, k) for other in seen.get(text, ())))
                seen.setdefault(text, []).append(read(ids, k))
    return (any(not row[w] and any(row[w + 1:]) for row in live for w in range(len(row))) and any(not any(row) for row in live)
            and any(k <= 0 for _, k in flat) and dropped_whole and folded and any(1 <= r[2] <= 3 for r in ref['hyp_rows'])
            and any(not 0 <= i < classes for ids, k in flat for i in read(ids, k))
            and any(k < 0 for _, k in flat) and any(k > steps for _, k in flat) and any(k == steps for _, k in flat))


# -------------------------------------------------------------------------------------------------------------------
# synthetic N-bests
# -------------------------------------------------------------------------------------------------------------------
CHARSET_36 = '0123456789abcdefghijklmnopqrstuvwxyz'
DROPPED_36 = 'xyz'                               # the test charset of the C = 37 cases lacks them: the adapter drops them


def synthetic_case(B, W, T, G, tokenizer, test_charset, rng):
    """An N-best over `tokenizer`'s classes and its labels over `test_charset` (which the adapter of the case maps into).  Image i aims at
    live rank i mod (W + 1) for its exact hypothesis, W meaning none; the last image of a batch of 4 or more has only dead slots.  Mixed
    in: near misses at distance 1 - 3, dead slots (also one whose tokens spell the label), ids >= C and < 0, strings the adapter drops whole,
    hypotheses equal after folding, lengths 0, T, negative and past T, tokens after the length.  Returns (tokens, scores, lengths,
    conf_scores, labels) as nested lists."""
    classes = len(tokenizer) - 2
    stoi = tokenizer._stoi
    limit = min(T, MAX_TOKENS)
    keeps = [c for c in test_charset if c in stoi]
    drops = [c for c in tokenizer._itos[1:classes] if c.lower() not in test_charset]
    assert keeps and drops

    def spell(text, room):
        """Token ids that adapt to `text`: upper-case variants where the tokenizer has them, dropped characters where there is room."""
        ids = [stoi[c.upper()] if c.upper() in stoi and rng.random() < 0.3 else stoi[c] for c in text]
        while len(ids) < room and rng.random() < 0.3:
            ids.insert(int(rng.integers(len(ids) + 1)), stoi[drops[int(rng.integers(len(drops)))]] if rng.random() < 0.6 else int(rng.choice([classes, classes + 1, classes + 7, -1])))
        return ids

    def near_miss(gt):
        s = list(gt[:limit])
        for at in rng.choice(len(s), size=min(len(s), int(rng.integers(1, 4))), replace=False):
            s[at] = keeps[(keeps.index(s[at]) + 1 + int(rng.integers(len(keeps) - 1))) % len(keeps)]      # another character
        kind = rng.random()
        if kind < 0.2 and len(s) > 1:
            del s[int(rng.integers(len(s)))]
        elif kind < 0.4 and len(s) < limit:
            s.insert(int(rng.integers(len(s) + 1)), keeps[int(rng.integers(len(keeps)))])
        return ''.join(s)

    tokens, scores, lengths, confs, labels = [], [], [], [], []
    for i in range(B):
        aim = i % (W + 1)
        long_label = aim == W and (i // (W + 1)) % 2 == 0
        n = G if long_label or B == 1 else int(rng.integers(1, min(G, limit, 25) + 1))
        if B == 1:
            n = min(G, limit)
        gt = ''.join(keeps[int(rng.integers(len(keeps)))] for _ in range(n))
        labels.append(gt)
        all_dead = B >= 4 and i == B - 1
        dead = 1 if W >= 2 and i % 2 == 0 and (aim == W or aim < W - 1) else 0
        live = 0 if all_dead else W - dead
        texts = []
        for rank in range(live):
            if rank == aim and n <= limit:
                texts.append(gt)
            elif rank and rng.random() < 0.25:
                texts.append(texts[-1] if texts[-1] != gt else near_miss(gt))      # equal to its neighbour after folding
            elif rng.random() < 0.15:
                texts.append('')                                                    # only dropped characters, or length 0
            else:
                texts.append(near_miss(gt))
        dead_at = {i % W} if dead else set()
        if all_dead:
            dead_at = set(range(W))
        rows, row_scores, row_lengths, row_confs, score = [], [], [], [], -float(rng.random())
        texts = iter(texts)
        for w in range(W):
            ids = [classes + 1] * T
            if w in dead_at:
                if rng.random() < 0.5 and n <= limit:
                    ids[:n] = [stoi[c] for c in gt]                                # a dead slot that spells the label: it must not count
                    rows.append(ids); row_lengths.append(n)
                else:
                    rows.append(ids); row_lengths.append(0)
                row_scores.append(NEG_INF); row_confs.append(NEG_INF if rng.random() < 0.5 else -1.0)
                continue
            text = next(texts)
            empty = not text and rng.random() < 0.5                                 # a hypothesis of no tokens, the other empty ones are dropped whole
            body = spell(text, limit) if text else [] if empty else [stoi[drops[int(rng.integers(len(drops)))]] for _ in range(int(rng.integers(1, limit + 1)))]
            length = len(body)
            ids[:length] = body
            if empty and rng.random() < 0.5:
                length = -int(rng.integers(1, 3))                                   # clamped to 0
            if length < T and rng.random() < 0.5:
                ids[max(length, 0):] = [stoi[keeps[int(rng.integers(len(keeps)))]] for _ in range(T - max(length, 0))]      # after the length: not read
            elif 0 <= length < T and rng.random() < 0.3:
                length = T + int(rng.integers(0, 4))                                # clamped to T; the pads in between are dropped
            rows.append(ids); row_lengths.append(length)
            score -= float(rng.random())
            row_scores.append(score); row_confs.append(-5.0 * float(rng.random()))
        tokens.append(rows); scores.append(row_scores); lengths.append(row_lengths); confs.append(row_confs)
    return tokens, scores, lengths, confs, labels
