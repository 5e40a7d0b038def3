"""GPU tests of lexicon matching: the matching operator through `parseq_op_lexicon_match` against the CPU restatement
(tests/lexicon_match_reference.py) with exact equality of ids and distances, and the whole call `lexicon_match` on the synthetic models of
the beam tests: its reading against `forward`, its candidates against the restatement applied to that reading, its scores against the
oracle's refinement pass (tests/beam_refine_reference.py), `keep_reading`, and the refusals.

The score bar is tests/test_beam_refine.py's for the same quantity — a pseudo-log-likelihood of the 'score' selection against the oracle's,
WHOLE_SCORE_BAR in fp32 and bf16x3 — and the oracle's sum is its `_pll`.  The order of two neighbours is compared only where the oracle's gap
between them exceeds twice that bar.
"""
import functools
import random

import numpy as np
import pytest
import torch

import beam_refine_reference as RR
import lexicon_match_reference as MR
from gpu_util import DEV, make_model, native
from oracle.synth import CONFIGS, synth_images
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.lexicon import MATCH_DEAD, Lexicon
from parseq_amd.tokenizer import Tokenizer
from test_beam_refine import WHOLE_SCORE_BAR, _model, _pll, _weights

pytestmark = pytest.mark.gpu

TOK = Tokenizer(CHARSET_94_FULL)
NEG_INF = float('-inf')
CHUNK = 64      # words per partial list of the kernel (LM_CHUNK)


# -------------------------------------------------------------------------------------------------------------------
# 1. the operator
# -------------------------------------------------------------------------------------------------------------------
def _table(words):
    t = np.zeros((len(words), 32), dtype=np.uint8)
    for r, w in enumerate(words):
        t[r, :len(w)] = w
        t[r, 31] = len(w)
    return torch.from_numpy(t)


def _run_op(readings, lengths, words, word_ids, n, C, eos_id, ranges=None, fold=None, crops_per_block=0):
    """(ids [B][n], distances [B][n]) of parseq_op_lexicon_match; `words` are the rows as they are matched (folded by the caller)."""
    nat, lib = native()
    rd = torch.tensor(readings, dtype=torch.int32, device=DEV)
    B, ldt = rd.shape
    dev = lambda v, dt=torch.int32: None if v is None else torch.tensor(v, dtype=dt, device=DEV)
    ln, rng, fd, wid = dev(lengths), dev(ranges), dev(fold), dev(word_ids)
    table = _table(words).to(DEV)
    ids = torch.full((B, n), -7, dtype=torch.int32, device=DEV)
    dist = torch.full((B, n), -7, dtype=torch.int32, device=DEV)
    need = lib.parseq_op_lexicon_match_workspace_bytes(B, len(words), n)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    with nat.guard(rd):
        nat.check(lib.parseq_op_lexicon_match(nat.ptr(rd), ldt, nat.ptr(ln), B, nat.ptr(table), len(words), nat.ptr(wid), nat.ptr(rng), nat.ptr(fd), C, eos_id,
                                              n, crops_per_block, nat.ptr(ids), nat.ptr(dist), nat.ptr(ws), need, nat.stream_ptr(rd)))
    torch.cuda.synchronize()
    return ids.cpu().tolist(), dist.cpu().tolist()


def _words(rng, count, alphabet, longest, lengths=None):
    return [[rng.choice(alphabet) for _ in range(rng.choice(lengths) if lengths else rng.randint(1, longest))] for _ in range(count)]


def _readings(rng, alphabet, lens, ldt, eos_id, filler):
    """Rows of `ldt` ids: a reading of each length in `lens`, then <eos> (where it fits), then `filler` ids the kernel must not read."""
    rows = []
    for n in lens:
        r = [rng.choice(alphabet) for _ in range(n)]
        rows.append((r + [eos_id] + [filler] * ldt)[:ldt])
    return rows


def _check(readings, lengths, words, word_ids, n, C, eos_id, ranges=None, fold=None, grids=(0,)):
    want = MR.match(readings, lengths, words, word_ids, n, eos_id, ranges, fold)
    for cpb in grids:
        got = _run_op(readings, lengths, words, word_ids, n, C, eos_id, ranges, fold, cpb)
        assert got[1] == want[1], f'distances (crops_per_block {cpb})'
        assert got[0] == want[0], f'word ids (crops_per_block {cpb})'
    return want


def _cutoff_ties_across_chunks(readings, words, word_ids, n, eos_id, want):
    """Crops whose n-th distance is shared by a row that was left out and lies in another 64-word chunk than the last row taken."""
    ids, lens = MR.pack(words)
    row_of = {k: r for r, k in enumerate(word_ids)}
    count = 0
    for b, reading in enumerate(readings):
        if want[0][b][n - 1] < 0:
            continue
        d = MR.distances(MR.cut(reading, eos_id), ids, lens)
        cut, last_row = want[1][b][n - 1], row_of[want[0][b][n - 1]]
        left_out = [r for r in range(len(words)) if d[r] == cut and r > last_row]
        count += any(r // CHUNK != last_row // CHUNK for r in left_out)
    return count


@pytest.mark.parametrize('size', [1, 63, 64, 65, 257, 4099])
def test_operator_list_sizes(size):
    """Readings of 0, 1, 31, 25 (and 32: no <eos> in the row) characters over a 6-letter alphabet that holds class 0 and class C - 1; words of 1 ..
    31 characters; B = 5 and B = 1; n = 8, 1 and 16; every crops_per_block gives the same result."""
    C, eos_id = 95, 3
    alphabet = [0, 1, 2, 4, C - 2, C - 1]
    rng = random.Random(100 + size)
    words = _words(rng, size, alphabet, 31, lengths=[1, 1, 2, 3, 4, 5, 6, 8, 25, 31])
    words[0] = [C - 1]                       # a word of one character, the last class
    words[-1] = [0] * 31                     # a word of max length, the first class
    word_ids = [3 * r + 1 for r in range(size)]      # ids that are not the row indices
    readings = _readings(rng, alphabet, [0, 1, 31, 25, 32], 32, eos_id, filler=C - 1)
    assert readings[0][0] == eos_id and eos_id not in readings[4] and readings[2][31] == eos_id
    for i, c in enumerate(words[size // 2][:5]):      # something near
        readings[3][i] = c
    total_ties = 0
    for n in (8, 1, 16):
        want = _check(readings, None, words, word_ids, n, C, eos_id, grids=(0, 4, 8))
        assert want[1][0] == sorted(len(w) for w in words)[:n] + [MATCH_DEAD] * max(0, n - size)      # the empty reading: the shortest words
        if size < n:
            assert all(row[size:] == [-1] * (n - size) for row in want[0]) and all(row[size:] == [MATCH_DEAD] * (n - size) for row in want[1])
        total_ties += _cutoff_ties_across_chunks(readings, words, word_ids, n, eos_id, want)
        _check(readings[2:3], None, words, word_ids, n, C, eos_id)      # B = 1, the 31-character reading
    if size >= 257:
        assert total_ties > 0, 'no tie at a cut-off between words of different chunks: pick another seed'
    # lengths cut a reading before its <eos>; a length past the row is the row
    _check(readings, [0, 1, 7, 40, 31], words, word_ids, 8, C, eos_id)


def test_operator_ranges():
    """Per-crop row ranges: the whole table, an empty list (begin == end and begin > end), ranges inside one chunk, across chunk and workgroup
    edges, clipped at both ends, a list smaller than n."""
    C, eos_id = 95, 0
    rng = random.Random(7)
    alphabet = [1, 2, 3, 4, 5, 94]
    words = _words(rng, 600, alphabet, 9)
    word_ids = list(range(10, 610))
    ranges = [(0, 600), (3, 3), (60, 70), (5, 2), (100, 10 ** 6), (-4, 9), (255, 258), (599, 600), (64, 128), (600, 700)]
    readings = _readings(rng, alphabet, [6, 5, 4, 3, 7, 2, 8, 0, 5, 5], 26, eos_id, filler=96)
    want = _check(readings, None, words, word_ids, 8, C, eos_id, ranges=ranges, grids=(0, 4))
    assert want[0][1] == want[0][3] == want[0][9] == [-1] * 8 and want[1][3] == [MATCH_DEAD] * 8
    assert want[0][6][3:] == [-1] * 5 and sorted(want[0][6][:3]) == [265, 266, 267] and want[0][7][0] == 609
    assert all(70 <= k < 80 for k in want[0][2]) and all(k < 19 for k in want[0][5])


def test_operator_fold():
    """A cased charset against a case-insensitive list: the rows hold folded ids, the reading goes through the same map on the device."""
    lex = Lexicon(['Hello', 'hello', 'HELP', 'World', 'word', 'W0rd', 'x'], TOK)
    fold = lex.fold_map().tolist()
    C, eos_id = lex.num_classes, lex.eos_id
    own = [[int(c) for c in row[:row[31]]] for row in lex.rows(False).numpy()]
    folded = [[int(c) for c in row[:row[31]]] for row in lex.rows(True).numpy()]
    rd, ln = lex.encode_readings(['HELLO', 'wORD', 'help', 'WéRD'])
    ids = lex.row_ids.tolist()
    on = _check(rd.tolist(), ln.tolist(), folded, ids, 3, C, eos_id, fold=fold)
    off = _check(rd.tolist(), ln.tolist(), own, ids, 3, C, eos_id)
    assert on[0][0][:2] == [0, 1] and on[1][0][:2] == [0, 0] and on[0][1][0] == 4 and on[1][1][0] == 0 and on[0][2][0] == 2 and on[1][2][0] == 0
    assert off[0][0][0] == 2 and off[1][0][0] == 2 and off[0][1][0] == 4 and off[1][1][0] == 3      # case counts: HELLO is nearest to HELP
    assert on[0][3][0] == 4 and on[1][3][0] == 1      # the character outside the charset costs one substitution
    # the same through Lexicon.nearest
    got = lex.nearest(['HELLO', 'wORD', 'help', 'WéRD'], 3, ignore_case=True, device=DEV)
    assert got[0].cpu().tolist() == on[0] and got[1].cpu().tolist() == on[1]
    got = lex.nearest(rd[:, :9], 3, device=DEV)
    assert got[0].cpu().tolist() == off[0] and got[1].cpu().tolist() == off[1]


def test_operator_random_64_by_4099():
    C, eos_id = 256, 0
    rng = random.Random(11)
    alphabet = list(range(1, 27)) + [255]
    words = _words(rng, 4099, alphabet, 12)
    readings = []
    for b in range(64):      # half the readings are a word of the list with up to three edits
        r = list(words[rng.randrange(4099)]) if b % 2 else [rng.choice(alphabet) for _ in range(rng.randint(0, 14))]
        for _ in range(rng.randint(0, 3)):
            k = rng.randrange(len(r) + 1)
            r = r[:k] + [rng.choice(alphabet)] * rng.randint(0, 1) + r[k + rng.randint(0, 1):]
        readings.append((r + [eos_id] * 32)[:32])
    want = _check(readings, None, words, list(range(4099)), 8, C, eos_id, grids=(0, 64))
    assert sum(row[0] <= 3 for row in want[1]) >= 32
    again = _run_op(readings, None, words, list(range(4099)), 8, C, eos_id)
    assert again == (want[0], want[1])


def test_operator_refusals():
    nat, lib = native()
    i32 = torch.zeros(64, dtype=torch.int32, device=DEV)
    table = torch.zeros(4, 32, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1 << 12, dtype=torch.uint8, device=DEV)

    def call(ldt=8, B=2, tb=table, rows=4, C=95, eos=0, n=4, cpb=0, nbytes=1 << 12, out=i32, off=0):
        return lib.parseq_op_lexicon_match(nat.ptr(i32), ldt, None, B, tb.data_ptr() + off if tb is not None else None, rows, None, None, None, C, eos, n, cpb,
                                           nat.ptr(out), nat.ptr(i32), nat.ptr(ws), nbytes, nat.stream_ptr(i32))
    for kw, word in (({'ldt': 0}, b'positions'), ({'ldt': 33}, b'positions'), ({'B': 0}, b'batch'), ({'tb': None}, b'table'), ({'rows': 0}, b'table'),
                     ({'rows': (1 << 26) + 1}, b'2^26'), ({'C': 257}, b'classes'), ({'C': 0}, b'classes'), ({'eos': 95}, b'eos_id'), ({'n': 0}, b'n 0'),
                     ({'n': 17}, b'n 17'), ({'cpb': -1}, b'crops_per_block'), ({'nbytes': 16}, b'workspace'), ({'out': None}, b'null'), ({'off': 4}, b'aligned')):
        assert call(**kw) == -1 and word in lib.parseq_last_error(), kw
    assert lib.parseq_op_lexicon_match_workspace_bytes(2, 4, 17) == 0 and lib.parseq_op_lexicon_match_workspace_bytes(0, 4, 4) == 0
    assert lib.parseq_op_lexicon_match_workspace_bytes(2, 0, 4) == 0
    assert lib.parseq_op_lexicon_match_workspace_bytes(5, 4099, 8) == (5 * 65 * 8 * 4 + 255) // 256 * 256
    torch.cuda.synchronize()


def test_one_definition_of_the_distance():
    """Lexicon matching, the metrics kernel and the error analysis share one column step (csrc/myers.h) and, the latter two, one loop over
    the label: for the same 5 x 4 pairs — readings of 0, 1, 2, 31, 32 characters over 37 classes, words of 1, 2, 30, 31 — the three
    operators and `parseq_amd.system.edit_distance` on the host give the same integers."""
    from parseq_amd.system import edit_distance
    nat, lib = native()
    C, eos_id, L = 37, 0, 32
    rng = random.Random(23)
    alphabet = list(range(1, C))
    readings = _readings(rng, alphabet, [0, 1, 2, 31, 32], L, eos_id, filler=C - 1)
    lens = [0, 1, 2, 31, 32]
    words = [[rng.choice(alphabet) for _ in range(n)] for n in (1, 2, 30, 31)]
    words[2][:20], words[3][5:31] = readings[3][:20], readings[4][:26]      # the long pairs are near, not only far
    text = lambda ids: ''.join(chr(48 + i) for i in ids)      # noqa: E731
    want = [[edit_distance(text(r[:n]), text(w)) for w in words] for r, n in zip(readings, lens)]
    assert want[0] == [1, 2, 30, 31] and want[3][2] < 30 and want[4][3] < 31      # the empty reading; the near pairs

    ids, dist = _run_op(readings, None, words, list(range(4)), 4, C, eos_id)      # N = every word: (distance, id) order
    assert [[dict(zip(i, d))[w] for w in range(4)] for i, d in zip(ids, dist)] == want, 'lexicon match'

    # the same pairs, one row each, for the evaluation kernels: identity adapter (class id = code point), the word as the label
    pairs = [(b, w) for b in range(5) for w in range(4)]
    n, G = len(pairs), 31
    table = torch.arange(C, dtype=torch.int32)
    table[eos_id] = -1
    gt = torch.zeros((n, G), dtype=torch.int32)
    logits = torch.zeros((n, L, C))
    for r, (b, w) in enumerate(pairs):
        gt[r, :len(words[w])] = torch.tensor(words[w], dtype=torch.int32)
        for pos, i in enumerate((readings[b][:lens[b]] + [eos_id])[:L]):
            logits[r, pos, i] = 9.0
    gt_len = torch.tensor([len(words[w]) for _, w in pairs], dtype=torch.int32, device=DEV)
    table, gt, logits = table.to(DEV), gt.to(DEV), logits.to(DEV)
    symbols = torch.arange(1, C, dtype=torch.int32, device=DEV)
    ids_out = torch.empty((n, L), dtype=torch.int32, device=DEV)
    lengths, conf = torch.empty((n,), dtype=torch.int32, device=DEV), torch.empty((n,), dtype=torch.float32, device=DEV)
    rows, rows2 = torch.full((n, 4), -7, dtype=torch.int32, device=DEV), torch.full((n, 4), -7, dtype=torch.int32, device=DEV)
    ws, totals = torch.empty(n, dtype=torch.float64, device=DEV), torch.zeros(5, dtype=torch.int64, device=DEV)
    nat.check(lib.parseq_eval_metrics(nat.ptr(logits), n, L, C, eos_id, nat.ptr(table), nat.ptr(gt), nat.ptr(gt_len), G, nat.ptr(ids_out), nat.ptr(lengths),
                                      nat.ptr(conf), nat.ptr(rows), nat.ptr(ws), nat.ptr(totals), nat.stream_ptr(logits)))
    scripts = torch.empty((n, 256 + 32), dtype=torch.int8, device=DEV)
    script_len = torch.empty((n,), dtype=torch.int32, device=DEV)
    acc = torch.zeros(272 + (C - 1 + 2) ** 2, dtype=torch.int64, device=DEV)
    nat.check(lib.parseq_eval_errors(nat.ptr(ids_out), nat.ptr(lengths), n, L, C, nat.ptr(table), nat.ptr(symbols), C - 1, nat.ptr(gt), nat.ptr(gt_len), G,
                                     nat.ptr(scripts), nat.ptr(script_len), nat.ptr(rows2), nat.ptr(acc), nat.stream_ptr(logits)))
    torch.cuda.synchronize()
    flat = [want[b][w] for b, w in pairs]
    assert lengths.cpu().tolist() == [lens[b] for b, _ in pairs]
    assert rows[:, 2].cpu().tolist() == flat, 'metrics kernel'
    assert rows2[:, 2].cpu().tolist() == flat, 'error analysis'


# -------------------------------------------------------------------------------------------------------------------
# 2. the whole call
# -------------------------------------------------------------------------------------------------------------------
WHOLE_B, WHOLE_N, WHOLE_SEED = 10, 4, {'parseq-tiny': 401, 'parseq': 405}
LETTERS = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789'


@functools.lru_cache(maxsize=None)
def _free_reading(name, precision):
    """(images, forward's logits at all L positions on the host) of the model the search tests use."""
    cfg = CONFIGS[name]
    images = synth_images(WHOLE_B, cfg, seed=WHOLE_SEED[name])
    m = _model(name, precision)      # (created outside inference_mode: its parameters keep their version counters)
    with torch.inference_mode():
        logits = m(images.to(DEV), cfg.max_label_length).cpu()
    assert logits.shape[1] == cfg.max_label_length + 1
    return images, logits


def _strings_of(logits, eos_id):
    out = []
    for row in logits.argmax(-1).tolist():
        out.append(TOK._ids2tok(row[:row.index(eos_id)] if eos_id in row else row))
    return out


def _lexicon_around(readings, seed, exact=()):
    """A word list built from the free readings: per reading one substitution, one insertion, one deletion and a two-edit word, the reading itself
    for the crops in `exact`, plus unrelated words."""
    rng = random.Random(seed)
    words = []
    for b, s in enumerate(readings):
        s = s[:20]
        k = rng.randrange(len(s)) if s else 0
        variants = [s[:k] + rng.choice(LETTERS) + s[k + 1:], s[:k] + rng.choice(LETTERS) + s[k:], s[:k] + s[k + 1:],
                    rng.choice(LETTERS) + s[1:k] + s[k + 1:] + rng.choice(LETTERS)]
        words += [v for v in variants if v]
        if b in exact and s:
            words.append(s)
    words += [''.join(rng.choice(LETTERS) for _ in range(rng.randint(1, 9))) for _ in range(40)]
    rng.shuffle(words)
    return words


def _reference_candidates(lex, res, n, keep_reading, ranges=None):
    rows = [[int(c) for c in row[:row[31]]] for row in lex.rows(False).numpy()]
    ids, dist = MR.match(res.reading_tokens.cpu().tolist(), res.reading_lengths.cpu().tolist(), rows, lex.row_ids.tolist(), n, lex.eos_id, ranges)
    return [MR.candidates(i, d, keep_reading) for i, d in zip(ids, dist)]


def _check_reading(res, logits, eos_id):
    picks = logits.argmax(-1)
    assert torch.equal(res.reading_tokens.cpu().long(), picks)
    L = picks.shape[1]
    assert res.reading_lengths.cpu().tolist() == [row.index(eos_id) if eos_id in row else L for row in picks.tolist()]


def _check_tokens(lex, res, cfg):
    """Every live hypothesis is its word's own characters (the reading's for word -1), <eos>, pad_id; a dead one is pad_id, -inf, word -1."""
    L = cfg.max_label_length + 1
    tok, words, ln, fin, sc, dist = (t.cpu().tolist() for t in (res.tokens, res.words, res.lengths, res.finished, res.scores, res.distances))
    rd, rl = res.reading_tokens.cpu().tolist(), res.reading_lengths.cpu().tolist()
    for b in range(len(tok)):
        for w in range(len(tok[b])):
            if dist[b][w] == MATCH_DEAD:
                assert sc[b][w] == NEG_INF and words[b][w] == -1 and tok[b][w] == [cfg.pad_id] * L and ln[b][w] == 0 and fin[b][w] == 0
                continue
            chars = rd[b][:rl[b]] if words[b][w] < 0 else [TOK._stoi[ch] for ch in lex.words[words[b][w]]]
            ended = len(chars) < L
            assert tok[b][w] == (chars + [cfg.eos_id] * ended + [cfg.pad_id] * L)[:L] and ln[b][w] == len(chars) and fin[b][w] == int(ended)
            assert sc[b][w] > NEG_INF


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_whole_call(name, precision):
    cfg = CONFIGS[name]
    L, B, N = cfg.max_label_length + 1, WHOLE_B, WHOLE_N
    images, logits = _free_reading(name, precision)
    readings = _strings_of(logits, cfg.eos_id)
    lex = Lexicon(_lexicon_around(readings, 9), TOK)
    m = _model(name, precision)
    with torch.inference_mode():
        plain = m.lexicon_match(images.to(DEV), lex, N, rescore=False)
        res = m.lexicon_match(images.to(DEV), lex, N)
        beams = m.tokenizer.decode_beams(res, lex)
        again = m.lexicon_match(images.to(DEV), lex, N)
    torch.cuda.synchronize()
    print(f'[lexicon match {name} {precision}] readings {readings}')
    for r in (plain, res):
        assert r.tokens.shape == (B, N, L) and r.distances.shape == (B, N) and r.reading_tokens.shape == (B, L)
        _check_reading(r, logits, cfg.eos_id)
        _check_tokens(lex, r, cfg)
    # without rescoring: the restatement's candidates in its order, a live score is 0
    want = _reference_candidates(lex, plain, N, False)
    assert [[(k, d) for k, d, _ in row] for row in want] == [list(zip(i, d)) for i, d in zip(plain.words.cpu().tolist(), plain.distances.cpu().tolist())]
    assert all(s in (0.0, NEG_INF) for row in plain.scores.cpu().tolist() for s in row)
    # with it: the same candidates, ranked by the pseudo-log-likelihood
    got = [sorted(zip(d, i)) for i, d in zip(res.words.cpu().tolist(), res.distances.cpu().tolist())]
    assert got == [sorted((d, k) for k, d, _ in row) for row in want]
    assert (res.distances.cpu() != MATCH_DEAD).all()      # the list is longer than N: every slot is compared
    tok, fin, ln, sc = res.tokens.cpu().view(-1, L), res.finished.cpu().view(-1), res.lengths.cpu().view(-1), res.scores.cpu().double()
    f = RR.oracle_refine_logits(_weights(name), cfg, images, N, L)
    oracle = torch.tensor(_pll(f, cfg, tok, fin, ln), dtype=torch.float64).view(B, N)
    worst = (sc - oracle).abs().max().item()
    compared = 0
    for b in range(B):
        assert all(x >= y for x, y in zip(sc[b].tolist(), sc[b].tolist()[1:]))
        ranked = sorted(oracle[b].tolist(), reverse=True)
        if min(x - y for x, y in zip(ranked, ranked[1:])) > 2 * WHOLE_SCORE_BAR:
            assert oracle[b].tolist() == ranked      # `oracle` is in the device's row order: it is the oracle's order too
            compared += 1
        assert [s for s, _ in beams[b]] == [lex.words[k] for k in res.words[b].cpu().tolist()]
    print(f'[lexicon match {name} {precision}] worst |dscore| against the oracle {worst:.3e} (bar {WHOLE_SCORE_BAR:.0e}), order compared on {compared} of {B} crops, '
          f'distances {res.distances.cpu().tolist()}')
    assert compared >= 0.9 * B, 'too many near-ties among the candidates: pick another lexicon seed'
    assert worst <= WHOLE_SCORE_BAR
    for k in ('tokens', 'words', 'distances', 'lengths', 'finished', 'reading_tokens'):
        assert torch.equal(getattr(res, k), getattr(again, k)), k
    assert torch.equal(res.scores.view(torch.int32), again.scores.view(torch.int32))


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_keep_reading_and_per_crop_lists(precision):
    """Per-crop lists (a forest, in another order than the crops), the reading as one more candidate: present as word -1 exactly where no word of
    the crop's list is the reading, and read back as the characters read."""
    name = 'parseq-tiny'
    cfg = CONFIGS[name]
    L, B, N = cfg.max_label_length + 1, WHOLE_B, 3
    images, logits = _free_reading(name, precision)
    readings = _strings_of(logits, cfg.eos_id)
    exact = {b for b in range(B) if b % 2 == 0 and 0 < len(readings[b]) <= cfg.max_label_length}
    assert exact, readings
    lists = [([readings[b]] if b in exact else []) + _lexicon_around([readings[b]], 20 + b)[:6 + b] for b in range(B)]
    order = [(3 * b + 1) % B for b in range(B)]      # crop b reads list order[b]
    assert sorted(order) == list(range(B))
    lex, _ = Lexicon.forest([lists[order.index(k)] for k in range(B)], TOK)
    m = _model(name, precision)
    with torch.inference_mode():
        res = m.lexicon_match(images.to(DEV), lex, N, lists=order, keep_reading=True)
        plain = m.lexicon_match(images.to(DEV), lex, N, lists=order, keep_reading=True, rescore=False)
        beams = m.tokenizer.decode_beams(res, lex)
    torch.cuda.synchronize()
    ranges = lex.list_ranges[torch.tensor(order)].tolist()
    want = _reference_candidates(lex, plain, N, True, ranges)
    assert [[(k, d) for k, d, _ in row] for row in want] == [list(zip(i, d)) for i, d in zip(plain.words.cpu().tolist(), plain.distances.cpu().tolist())]
    kept = 0
    _check_reading(res, logits, cfg.eos_id)
    for b in range(B):
        words, dist, sc = res.words[b].cpu().tolist(), res.distances[b].cpu().tolist(), res.scores[b].cpu().tolist()
        assert sorted(zip(dist, words)) == sorted((d, k) for k, d, _ in want[b])
        has_exact = any(d == 0 and k >= 0 for k, d, _ in want[b])
        live_reading = [w for w in range(N + 1) if words[w] == -1 and sc[w] > NEG_INF]
        assert len(live_reading) == (0 if has_exact else 1)
        assert all(lex.words[k] in lists[b] for k in words if k >= 0)      # only words of the crop's own list
        for w in live_reading:
            assert dist[w] == 0 and beams[b][w][0] == readings[b]
            kept += 1
        assert len(beams[b]) == sum(s > NEG_INF for s in sc)
    _check_tokens(lex, res, cfg)
    _check_tokens(lex, plain, cfg)
    assert 0 < kept < B, (kept, readings)      # both cases occur
    print(f'[lexicon match keep_reading {precision}] the reading competes on {kept} of {B} crops')


@pytest.mark.parametrize('decode_ar,refine_iters', [(False, 1), (True, 2)])
def test_reading_is_forwards_under_every_decode(decode_ar, refine_iters):
    name = 'parseq-tiny'
    cfg = CONFIGS[name]
    m = make_model(name, 'bf16x3', decode_ar=decode_ar, refine_iters=refine_iters)
    x = synth_images(5, cfg, seed=77).to(DEV)
    lex = Lexicon(['abc', 'Hello', 'x'], TOK)
    with torch.inference_mode():
        logits = m(x, cfg.max_label_length).cpu()
        res = m.lexicon_match(x, lex, 2, rescore=False, ignore_case=True)
    _check_reading(res, logits, cfg.eos_id)
    assert sorted(res.words[0].cpu().tolist()) != [-1, -1]


def test_whole_call_refusals():
    nat, lib = native()
    name = 'parseq-tiny'
    cfg = CONFIGS[name]
    m = _model(name, 'bf16x3')
    B, N, L = 4, 2, cfg.max_label_length + 1
    x = synth_images(B, cfg, seed=3).to(DEV)
    lex = Lexicon(['abc', 'abd', 'xyz'], TOK)
    t = lex.match_table(DEV)
    plan = m.model._plan(B * N)

    def call(n=N, keep=0, table=t['table'], rows=lex.num_rows, batch=B, short=0, misalign=0, images_ok=True, out_ok=True, refine_iters=0, own_off=0):
        W = max(n, 1) + keep
        outs = [torch.full((B * W * L,), -7, dtype=torch.int32, device=DEV), torch.full((B * W,), -7.0, device=DEV), torch.full((B * W,), -7, dtype=torch.int32, device=DEV),
                torch.full((B * W,), 7, dtype=torch.uint8, device=DEV), torch.full((B * W,), -7, dtype=torch.int32, device=DEV),
                torch.full((B * W,), -7, dtype=torch.int32, device=DEV), torch.full((B * L,), -7, dtype=torch.int32, device=DEV), torch.full((B,), -7, dtype=torch.int32, device=DEV)]
        args = nat.LexiconMatchArgs(table.data_ptr() if table is not None else None, t['own'].data_ptr() + own_off, t['row_ids'].data_ptr(), None, None, rows, n, 1, keep)
        import ctypes as C
        need = lib.parseq_forward_lexicon_match_workspace_bytes(plan, batch, C.byref(args))
        ws = torch.empty(max(need, 1 << 20) + 64, dtype=torch.uint8, device=DEV)
        status = lib.parseq_forward_lexicon_match(plan, nat.ptr(x) if images_ok else None, nat.dtype_code(x.dtype), batch, 1, refine_iters, C.byref(args), nat.ptr(outs[0]),
                                                  nat.ptr(outs[1]), nat.ptr(outs[2]), nat.ptr(outs[3]), nat.ptr(outs[4]), nat.ptr(outs[5]) if out_ok else None,
                                                  nat.ptr(outs[6]), nat.ptr(outs[7]), ws.data_ptr() + misalign, (need - short) if short else ws.numel() - 64, nat.stream_ptr(x))
        torch.cuda.synchronize()
        fills = (-7, -7.0, -7, 7, -7, -7, -7, -7)
        return status, all(bool((o == v).all()) for o, v in zip(outs, fills)), need

    status, untouched, need = call()
    assert status == 0 and not untouched and need > 0 and need % 256 == 0
    assert call(keep=1)[:2] == (0, False)
    for kw, word in (({'n': 0}, b'n 0'), ({'n': 17}, b'n 17'), ({'n': 16, 'keep': 1}, b'n 16'), ({'table': None}, b'table'), ({'rows': 0}, b'table'),
                     ({'batch': 1 << 20}, b'hypotheses'), ({'batch': 0}, b'batch'), ({'short': 1}, b'workspace'), ({'misalign': 4}, b'aligned'),
                     ({'images_ok': False}, b'null'), ({'out_ok': False}, b'null'), ({'refine_iters': -1}, b'refine_iters'), ({'own_off': 4}, b'aligned')):
        status, untouched, need = call(**kw)
        assert (status, untouched) == (-1, True) and word in lib.parseq_last_error(), kw
        if 'n' in kw or 'table' in kw or 'rows' in kw or kw.get('batch') in (0, 1 << 20):
            assert need == 0
    import ctypes as C
    from parseq_amd import create_model
    args = nat.LexiconMatchArgs(t['table'].data_ptr(), None, None, None, None, lex.num_rows, 2, 1, 0)
    deep = create_model(name, dec_depth=2, precision='bf16x3').eval().to(DEV)
    assert lib.parseq_forward_lexicon_match_workspace_bytes(deep.model._plan(8), 4, C.byref(args)) == 0 and b'dec_depth' in lib.parseq_last_error()
    with pytest.raises(ValueError, match='dec_depth'):
        deep.lexicon_match(x, lex, 2)
    vit = create_model('vitstr', precision='bf16').eval().to(DEV)
    assert lib.parseq_forward_lexicon_match_workspace_bytes(vit.model._plan(8), 4, C.byref(args)) == 0 and b'ViTSTR' in lib.parseq_last_error()
    with pytest.raises(ValueError, match='ViTSTR'):
        vit.lexicon_match(torch.zeros(2, 3, *vit.hparams.img_size, device=DEV), lex, 2)
    for bad in (dict(n=0), dict(n=17), dict(n=16, keep_reading=True)):
        with pytest.raises(ValueError, match='n must be'):
            m.lexicon_match(x, lex, **bad)
    with pytest.raises(ValueError, match='empty'):
        m.lexicon_match(x, Lexicon(['é'], TOK), 2)
    with pytest.raises(ValueError, match='lists'):
        m.lexicon_match(x, lex, 2, lists=[0, 0])
    torch.cuda.synchronize()


def test_read_cli_match(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip('PIL.Image')
    import read as read_cli
    from oracle.make_resize_golden import make_input
    files = []
    for i, (h, w) in enumerate([(40, 150), (32, 128)]):
        f = tmp_path / f'crop{i}.png'
        Image.fromarray(make_input(h, w, 1 - i % 2), 'RGB').save(f)
        files.append(str(f))
    m = _model('parseq-tiny', 'bf16x3')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    with torch.inference_mode():
        free = [label for _, label, _ in read_cli.read_files(m, files, DEV)]
    words = tmp_path / 'words.txt'
    words.write_text('\n'.join(_lexicon_around(free, 3)) + '\n')
    read_cli.main(['pretrained=parseq-tiny', '--images', *files, '--device', DEV, '--lexicon', str(words), '--match', '4', '--nbest', '3'])
    out = capsys.readouterr().out.splitlines()[1:]
    with torch.inference_mode():
        best = read_cli.read_files_match(m, files, read_cli.load_word_list(str(words)), 4, DEV)
    want = []
    for (f, alts), reading in zip(best, free):
        assert len(alts) == 4 and all(x[1] >= y[1] for x, y in zip(alts, alts[1:]))
        for label, _, d in alts:      # the distance printed is the edit distance of the word to the free reading
            ids, lens = MR.pack([[ord(ch) for ch in label]])
            assert d == int(MR.distances([ord(ch) for ch in reading], ids, lens)[0]), (label, reading)
        want += read_cli.match_lines(f, alts[:3], True)
    assert out == want and len(out) == 8
    read_cli.main(['pretrained=parseq-tiny', '--images', *files, '--device', DEV, '--lexicon', str(words), '--match', '4'])
    assert capsys.readouterr().out.splitlines()[1:] == [f'{f}: {alts[0][0]}' for f, alts in best]
