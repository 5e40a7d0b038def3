"""CPU restatement of the error analysis, written from the definition: the unit-cost Levenshtein table, the canonical
edit script read from (m, n) back to (0, 0), the symbol indices and the four integer tables.  Sequences are strings or lists of code points.
Nothing here imports parseq_amd.evaluate: `host_edit_script` and the kernel are both held against this file."""
import numpy as np

MATCH, SUBSTITUTION, INSERTION, DELETION = 0, 1, 2, 3
SCRIPT_WIDTH = 288
BINS = 33
HEAD, BY_LENGTH, BY_POSITION, CONFUSION = 0, 8, 8 + 4 * BINS, 8 + 8 * BINS


def levenshtein_table(p, g):
    """D[i][j]: the cheapest way to turn p[:i] into g[:j] with unit-cost substitutions, insertions and deletions."""
    m, n = len(p), len(g)
    d = [[0] * (n + 1) for _ in range(m + 1)]                  # (lists: the scalar loop below is several times slower on a numpy array)
    for i in range(m + 1):
        d[i][0] = i
    for j in range(n + 1):
        d[0][j] = j
    for j in range(1, n + 1):
        for i in range(1, m + 1):
            d[i][j] = min(d[i - 1][j - 1] + (p[i - 1] != g[j - 1]), d[i - 1][j] + 1, d[i][j - 1] + 1)
    d = np.array(d, dtype=np.int64).reshape(m + 1, n + 1)
    return d


def edit_script(p, g, table=None):
    """Forward-order codes.  At (i, j) the first rule that holds: diagonal (match / substitution), up (insertion), left (deletion)."""
    d = levenshtein_table(p, g) if table is None else table
    i, j, backwards = len(p), len(g), []
    while (i, j) != (0, 0):
        if i > 0 and j > 0 and d[i - 1, j - 1] + (p[i - 1] != g[j - 1]) == d[i, j]:
            backwards.append(MATCH if p[i - 1] == g[j - 1] else SUBSTITUTION)
            i, j = i - 1, j - 1
        elif i > 0 and d[i - 1, j] + 1 == d[i, j]:
            backwards.append(INSERTION)
            i -= 1
        else:
            assert j > 0 and d[i, j - 1] + 1 == d[i, j], 'the rule is total'
            backwards.append(DELETION)
            j -= 1
    return backwards[::-1]


def replay(script, p, g):
    """(cost, the predicted characters the script consumes, the label characters it consumes, what applying it to p gives)."""
    i = j = cost = 0
    pred_side, label_side, applied = [], [], []
    for code in script:
        cost += code != MATCH
        if code in (MATCH, SUBSTITUTION):
            assert (p[i] == g[j]) == (code == MATCH)
            pred_side.append(p[i]); label_side.append(g[j]); applied.append(g[j])      # a substitution writes the label's character
            i, j = i + 1, j + 1
        elif code == INSERTION:
            pred_side.append(p[i])                                                         # the surplus predicted character is removed
            i += 1
        else:
            label_side.append(g[j]); applied.append(g[j])                                  # the missing label character is supplied
            j += 1
    return cost, pred_side, label_side, applied


def myers_columns(p, g):
    """[(Pv, Mv)] for columns 0 .. n of the bit-vector recurrence the kernel runs (pattern p, m <= 32 bits of a 64-bit word, text g)."""
    m, word = len(p), (1 << 64) - 1
    pv, mv = (1 << m) - 1, 0
    columns = [(pv, mv)]
    for c in g:
        eq = sum(1 << r for r in range(m) if p[r] == c)
        xv = eq | mv
        xh = ((((eq & pv) + pv) & word) ^ pv) | eq
        ph = (mv | ~(xh | pv)) & word
        mh = pv & xh
        ph = ((ph << 1) | 1) & word
        mh = (mh << 1) & word
        pv = (mh | ~(xv | ph)) & word
        mv = ph & xv
        columns.append((pv, mv))
    return columns


def column_entry(column, i, j):
    """D[i][j] from column j's (Pv, Mv)."""
    mask = (1 << i) - 1
    return j + bin(column[0] & mask).count('1') - bin(column[1] & mask).count('1')


def symbol_set(adapter_table):
    return sorted({int(c) for c in adapter_table if c >= 0})


def adapt(ids_row, length, width, classes, adapter_table):
    """The adapted prediction as code points: the first clamp(length, 0, width) ids, those outside [0, classes) and the dropped ones removed."""
    kept = [int(i) for i in ids_row[:min(max(int(length), 0), width)] if 0 <= i < classes]
    return [int(adapter_table[i]) for i in kept if adapter_table[i] >= 0]


def analyse(preds, labels, symbols):
    """dict(scripts int8 [B, 288], script_len [B], rows [B, 4], words: the flat int64 accumulator) of a batch of (adapted prediction, label) pairs."""
    symbols = list(symbols)
    t = len(symbols)
    index = {s: k for k, s in enumerate(symbols)}
    n_samples = len(preds)
    scripts = np.full((n_samples, SCRIPT_WIDTH), -1, dtype=np.int8)
    script_len = np.zeros(n_samples, dtype=np.int32)
    rows = np.zeros((n_samples, 4), dtype=np.int32)
    head = np.zeros(8, dtype=np.int64)
    by_length = np.zeros((BINS, 4), dtype=np.int64)
    by_position = np.zeros((BINS, 4), dtype=np.int64)
    confusion = np.zeros((t + 2, t + 2), dtype=np.int64)
    for b, (p, g) in enumerate(zip(preds, labels)):
        d = levenshtein_table(p, g)
        script = edit_script(p, g, d)
        distance = int(d[len(p), len(g)])
        scripts[b, :len(script)] = script
        script_len[b] = len(script)
        rows[b] = (len(p), len(g), distance, distance == 0)
        head[0] += 1
        head[5] += distance == 0
        by_length[min(len(g), BINS - 1)] += (1, distance == 0, distance, len(g))
        i = j = 0
        for code in script:
            where = by_position[min(j, BINS - 1)]
            head[1 + code] += 1
            if code == INSERTION:
                confusion[t + 1, index.get(p[i], t)] += 1
                where[3] += 1
                i += 1
            elif code == DELETION:
                confusion[index.get(g[j], t), t + 1] += 1
                where[0] += 1; where[2] += 1
                j += 1
            else:
                confusion[index.get(g[j], t), index.get(p[i], t)] += 1
                where[0] += 1; where[1] += code == SUBSTITUTION
                i, j = i + 1, j + 1
    words = np.concatenate([head, by_length.ravel(), by_position.ravel(), confusion.ravel()])
    return dict(scripts=scripts, script_len=script_len, rows=rows, words=words, head=head, by_length=by_length, by_position=by_position, confusion=confusion)


def check_identities(head, by_length, by_position, confusion, preds, labels):
    """The identities every set of tables satisfies, against the pairs they were made from."""
    t = confusion.shape[0] - 2
    samples, matches, subs, ins, dels, exact = (int(v) for v in head[:6])
    sum_m, sum_n = sum(len(p) for p in preds), sum(len(g) for g in labels)
    distance = int(by_length[:, 2].sum())
    assert samples == len(preds) and int(head[6]) == 0 and int(head[7]) == 0
    assert matches + subs + dels == sum_n and matches + subs + ins == sum_m and subs + ins + dels == distance
    assert int(confusion.sum()) == matches + subs + ins + dels
    assert int(np.trace(confusion[:t, :t])) == matches
    assert not confusion[:, t].any() and confusion[t + 1, t + 1] == 0
    assert int(confusion[:t + 1, t + 1].sum()) == dels and int(confusion[t + 1, :t + 1].sum()) == ins
    assert int(by_length[:, 0].sum()) == samples and int(by_length[:, 1].sum()) == exact and int(by_length[:, 3].sum()) == sum_n
    for n in range(BINS - 1):
        assert by_length[n, 3] == n * by_length[n, 0]
    assert by_position[:, 0].sum() == sum_n and by_position[:, 1].sum() == subs and by_position[:, 2].sum() == dels and by_position[:, 3].sum() == ins
    for j in range(BINS - 1):                      # a label has a character at position j iff it is longer than j
        assert by_position[j, 0] == sum(1 for g in labels if len(g) > j)
