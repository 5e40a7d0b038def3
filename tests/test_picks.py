"""Non-finite and tied logits through every greedy pick of the library.

All of them are built on `argmax_take`, `wave_argmax` and `argmax_final` (csrc/common.h), which promise torch.argmax's rule: the first
maximum wins, a NaN counts as the maximum (the first NaN wins), a row with no finite winner gives 0.

  1. CPU: `pick` restates that rule in plain Python and is held to torch.argmax on every input family below; `O.postprocess` gives id 0 and
     probability NaN exactly where the soft-max of a row is not finite; the vectorised rule of tests/beam_refine_reference.py equals `pick`.
  2. GPU, logits from the caller (C ABI): `parseq_postprocess`, `parseq_eval_metrics`, `parseq_op_beam_refine` (its arg-max and
     log-max-probability), `parseq_op_attention_geometry` (the peak), and the non-finite rule of `parseq_op_beam_step`.
  3. GPU, the picks fused into the decoder: the head's bias and weight shape the model's own logits (a tie, a NaN, a +inf, all -inf),
     through every route that picks: latency and in-flight AR step, `ar_argmax`, `refine_prep` from logits, the early exit; and the device
     reading (`tokenizer.read`, `lexicon_match`) of those logits.

The families (every one at every class count C, a row per line of the table):
  placement   row i holds its single maximum at class i: every lane wins once, for C > 64 in both strided visits
  pair_ties   every pair i < j: two equal maxima, everything else lower and distinct; the pick is i
  nan         one NaN at every class; two NaNs, a NaN before a +inf and a NaN after one, at pairs that span quads, DPP rows and readlane rows
  inf         one +inf, two +inf, -inf everywhere, -inf everywhere but one finite class
  saturation  the largest finite float and its negative in one row
Everything else in a row is -1 - k / 4 for a permutation k of the classes: distinct, exact in fp32, below every planted value.
"""
import functools
import itertools
import math

import numpy as np
import pytest
import torch

import attn_map_reference as AR
import beam_refine_reference as RR
from gpu_util import DEV, native
from oracle import parseq_oracle as O
from oracle.synth import CONFIGS, synth_images, synth_state_dict
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.tokenizer import CharsetAdapter, Tokenizer

NAN, INF = float('nan'), float('inf')
FLT_MAX = float(torch.finfo(torch.float32).max)
CLASS_COUNTS = [1, 37, 63, 64, 65, 95, 128, 129]
TOK = Tokenizer(CHARSET_94_FULL)
PEAK = 4.0


# -------------------------------------------------------------------------------------------------------------------
# 1. the rule, and the families
# -------------------------------------------------------------------------------------------------------------------
def pick(row):
    """common.h's greedy pick in one loop: the first maximum, a NaN above everything (the first NaN stays), 0 for an empty row and for
    one without a finite winner."""
    best, bi = -INF, -1
    for i, v in enumerate(row):
        if best != best:
            break
        if v != v or v > best:
            best, bi = v, i
    return max(bi, 0)


def picks(rows):
    return [pick(r) for r in rows.tolist()]


def _lanes(C):
    """Classes that cover every lane mod 16 and every DPP row of both strided visits, and both ends."""
    fixed = [0, 16, 17, 31, 32, 47, 48, 63, 64, 65, 79, 80, 94, 96, 111, 112, 127, 128]
    return sorted({c for c in fixed + list(range(16)) + [C - 1] if c < C})


def _pairs(C):
    """Pairs i < j in one quad, across quads, across halves of a DPP row, across DPP rows, across the two strided visits."""
    marks = [c for c in (0, 1, 2, 5, 11, 15, 16, 30, 33, 50, 63, 64, 70, 94, 127, 128, C - 1) if c < C]
    return sorted(set(itertools.combinations(sorted(set(marks)), 2)))


def _base(n, C, seed):
    g = torch.Generator().manual_seed(seed)
    return -1.0 - 0.25 * torch.rand(n, C, generator=g).argsort(-1).float()


def _planted(C, seed, plants):
    """One row per entry of `plants`, a list of (class, value) lists."""
    x = _base(len(plants), C, seed)
    for r, entries in enumerate(plants):
        for c, v in entries:
            x[r, c] = v
    return x


@functools.lru_cache(maxsize=None)
def families(C):
    """{name: fp32 [rows, C]}; a family that needs more classes than C has is left out."""
    lanes, pairs = _lanes(C), _pairs(C)
    every = list(itertools.combinations(range(C), 2))
    out = {'placement': _planted(C, 1, [[(i, PEAK)] for i in range(C)])}
    if every:
        out['pair_ties'] = _planted(C, 2, [[(i, PEAK), (j, PEAK)] for i, j in every])
    out['nan'] = _planted(C, 3, [[(i, NAN)] for i in range(C)] + [[(i, NAN), (j, NAN)] for i, j in pairs]
                          + [[(i, NAN), (j, INF)] for i, j in pairs] + [[(i, INF), (j, NAN)] for i, j in pairs])
    rows = _planted(C, 4, [[(i, INF)] for i in lanes] + [[(i, INF), (j, INF)] for i, j in pairs] + [[]] + [[] for _ in lanes])
    first_lone = len(lanes) + len(pairs) + 1
    rows[first_lone - 1:] = -INF
    for k, i in enumerate(lanes):
        rows[first_lone + k, i] = -3.5
    out['inf'] = rows
    if pairs:
        out['saturation'] = _planted(C, 5, [[(i, FLT_MAX), (j, -FLT_MAX)] for i, j in pairs] + [[(i, -FLT_MAX), (j, FLT_MAX)] for i, j in pairs])
    return out


def _no_softmax(rows):
    """Rows whose soft-max is not finite: a NaN, a +inf, or nothing but -inf."""
    return torch.isnan(rows).any(-1) | (rows == INF).any(-1) | (rows == -INF).all(-1)


def _as_batch(rows, L):
    """[B, L, C]: the rows as they are (L = 1), or L to an image, the last image filled up with the first rows."""
    n, C = rows.shape
    if L == 1:
        return rows.view(n, 1, C).clone()
    B = -(-n // L)
    return rows[torch.arange(B * L) % n].view(B, L, C).clone()


@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_the_rule_is_torch_argmax(C):
    for name, rows in families(C).items():
        want = picks(rows)
        assert torch.argmax(rows, -1).tolist() == want, name
        assert RR.first_argmax_rows(rows).tolist() == want, name
        if name == 'placement':
            assert want == list(range(C))
        if name == 'pair_ties':
            assert want == [i for i, _ in itertools.combinations(range(C), 2)]
    assert pick([]) == 0 and pick([-INF, -INF]) == 0 and pick([1.0, NAN, 3.0, NAN]) == 1 and pick([-INF, -5.0]) == 1


def test_the_families_hold_what_they_say():
    f = families(95)
    assert f['pair_ties'].shape[0] == 4465 and f['placement'].shape[0] == 95
    assert sorted({i % 16 for i in _lanes(95)}) == list(range(16)) and {i // 16 for i in _lanes(129)} >= set(range(8))
    assert {(i // 16, j // 16) for i, j in _pairs(95)} >= {(0, 0), (0, 1), (0, 3), (1, 2), (3, 4)}
    for C in CLASS_COUNTS:
        for name, rows in families(C).items():
            finite = torch.where(torch.isfinite(rows) & (rows.abs() < 1e30) & (rows < PEAK), rows, torch.arange(C) * 1e-3 + 100)
            assert all(len(set(r)) == C for r in finite.tolist()), (C, name)      # whatever is not planted is distinct
    nan = families(95)['nan']
    assert int(torch.isnan(nan).any(-1).sum()) == nan.shape[0] and int((nan == INF).any(-1).sum()) == 2 * len(_pairs(95))
    inf = families(95)['inf']
    assert int((inf == -INF).all(-1).sum()) == 1 and int(((inf == -INF).sum(-1) == 94).sum()) == len(_lanes(95))


@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_oracle_postprocess_reads_eos_where_the_softmax_is_not_finite(C):
    """strhub/data/utils.py:90 takes `max` over softmax(logits): with a NaN, a +inf or nothing but -inf in a row every probability is NaN,
    the id is 0 (<eos>) and the label is cut there."""
    for name, rows in families(C).items():
        ids, lengths, probs, conf = O.postprocess(rows.view(-1, 1, C), TOK.eos_id)
        bad = _no_softmax(rows)
        assert (name in ('nan', 'inf')) == bool(bad.any())
        assert torch.equal(torch.isnan(probs[:, 0]), bad) and torch.equal(torch.isnan(conf), bad), name
        assert (ids[bad] == 0).all() and (lengths[bad] == 0).all(), name
        assert ids[~bad, 0].tolist() == [p for p, b in zip(picks(rows), bad.tolist()) if not b], name
        assert torch.isfinite(probs[~bad]).all() and (probs[~bad] > 0).all()
    ids, _, probs, _ = O.postprocess(torch.tensor([[[1.0, NAN, 3.0, NAN]]]))
    assert ids.tolist() == [[0]] and torch.isnan(probs).all()


# -------------------------------------------------------------------------------------------------------------------
# 2. kernels that take logits from the caller
# -------------------------------------------------------------------------------------------------------------------
def _same_nonfinite(got, want):
    """NaN where NaN, +inf where +inf, -inf where -inf."""
    return (torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got == INF, want == INF) and torch.equal(got == -INF, want == -INF))


def _check_postprocess(tag, got, want):
    gi, gl, gp, gc = got
    ids, lengths, probs, conf = want
    assert torch.equal(gi.long(), ids), f'{tag}: ids'
    assert torch.equal(gl.long(), lengths), f'{tag}: lengths'
    if gp is not None:
        assert _same_nonfinite(gp, probs), f'{tag}: non-finite probabilities'
        assert torch.allclose(gp, probs, rtol=2e-6, atol=1e-7, equal_nan=True), f'{tag}: probabilities'
    assert _same_nonfinite(gc, conf), f'{tag}: non-finite confidence'
    assert torch.allclose(gc, conf, rtol=2e-5, atol=1e-30, equal_nan=True), f'{tag}: confidence'


@pytest.mark.gpu
@pytest.mark.parametrize('L', [1, 26])
@pytest.mark.parametrize('C', CLASS_COUNTS)
def test_postprocess_kernel(C, L):
    for name, rows in families(C).items():
        x = _as_batch(rows, L)
        want = O.postprocess(x, TOK.eos_id)
        got = [t.cpu() for t in TOK._postprocess(x.to(DEV))]
        _check_postprocess(f'{name} C={C} L={L}', got, want)


def _metrics_labels(ids, lengths, table):
    """A ground truth per row: the oracle's own reading for two rows of three, the reading with its first character changed or a lone
    character for the third."""
    labels = []
    for r, (row, n) in enumerate(zip(ids.tolist(), lengths.tolist())):
        s = ''.join(chr(table[i]) for i in row[:n] if table[i] >= 0)
        labels.append(s if r % 3 else ('#' + s[1:]))
    return labels


@pytest.mark.gpu
@pytest.mark.parametrize('L', [1, 26])
def test_eval_metrics_kernel(L):
    """ids, lengths and confidence as the oracle's; correct, the distance and the totals from those ids through the brute-force table."""
    from parseq_amd.evaluate import adapter_table
    from test_eval_metrics import dp_distance, new_accum, read_accum, run_metrics
    C = 95
    table = adapter_table(TOK, CharsetAdapter(CHARSET_94_FULL[:36]))      # folds the upper case, drops the punctuation
    for name, rows in families(C).items():
        x = _as_batch(rows, L)
        ids, lengths, _, conf = O.postprocess(x, TOK.eos_id)
        labels = _metrics_labels(ids, lengths, table)
        acc = new_accum()
        gi, gl, gc, grows = run_metrics(x, table, labels, TOK.eos_id, acc)
        _check_postprocess(f'{name} L={L}', (gi, gl, None, gc), (ids, lengths, None, conf))
        want_rows, want_ned = [], 0.0
        for row, n, gt in zip(ids.tolist(), lengths.tolist(), labels):
            pred = [int(table[i]) for i in row[:n] if table[i] >= 0]
            d = dp_distance(pred, [ord(ch) for ch in gt])
            want_rows.append([len(pred), len(gt), d, int(d == 0)])
            want_ned += d / max(len(pred), len(gt), 1)
        assert grows.tolist() == want_rows, name
        n, correct, label_length, ned, confidence = read_accum(acc)
        assert (n, correct, label_length) == (len(labels), sum(r[3] for r in want_rows), sum(r[0] for r in want_rows)), name
        assert abs(ned - want_ned) <= 1e-12 * max(want_ned, 1), name
        if torch.isnan(conf).any():
            assert math.isnan(confidence), name
        else:
            assert abs(confidence - conf.double().sum().item()) <= 2e-5 * conf.double().sum().item(), name


def _refine_op(x, B, W, L, mode, tokens=None):
    """parseq_op_beam_refine on logits [B * W, L, C]; the state after it, and the row statistics it left in the workspace (three arrays of
    B * W * L words, each on a 256-byte boundary: the log-probability of the row's token, the arg-max class, its log-probability)."""
    nat, lib = native()
    n, C = B * W, x.shape[-1]
    eos_id, bos_id, pad_id, ldt = 0, C, C + 1, 32
    tok = torch.full((n, ldt), pad_id, dtype=torch.int32)
    tok[:, 0] = bos_id
    if tokens is not None:
        tok[:, 1:1 + L] = tokens
    d = dict(tok=tok.to(DEV), picked=torch.full((n,), pad_id, dtype=torch.int32, device=DEV),
             scores=torch.full((n,), -1.0, device=DEV), finished=torch.zeros(n, dtype=torch.uint8, device=DEV),
             lengths=torch.full((n,), L, dtype=torch.int32, device=DEV),
             ar=torch.arange(n, dtype=torch.float32, device=DEV))
    lg = x.to(DEV, torch.float32).contiguous()
    need = lib.parseq_op_beam_refine_workspace_bytes(B, W, L)
    assert need > 0
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    with nat.guard(lg):
        nat.check(lib.parseq_op_beam_refine(nat.ptr(lg), B, W, C, L, {'score': 1, 'edit': 2}[mode], nat.ptr(d['tok']), ldt, nat.ptr(d['scores']),
                                            nat.ptr(d['finished']), nat.ptr(d['lengths']), nat.ptr(d['picked']), None, None, nat.ptr(d['ar']),
                                            eos_id, pad_id, nat.ptr(ws), need, nat.stream_ptr(lg)))
    torch.cuda.synchronize()
    out = {k: v.cpu() for k, v in d.items()}
    out['tokens'] = out['tok'][:, 1:1 + L]
    pitch = (n * L * 4 + 255) // 256 * 256
    words = ws.cpu()
    out['amax'] = words[pitch:pitch + n * L * 4].view(torch.int32).view(n, L)
    out['lp_max'] = words[2 * pitch:2 * pitch + n * L * 4].view(torch.float32).view(n, L)
    return out


def _refine_rows(n, L, pad_id):
    """The state _refine_op starts from: n live unfinished rows at score -1, no tokens yet, ar_score = the row's number."""
    return RR.Rows([[pad_id] * L for _ in range(n)], [-1.0] * n, [0] * n, [L] * n, [-1] * n, [-1] * n, [float(r) for r in range(n)])


@pytest.mark.gpu
@pytest.mark.parametrize('L', [1, 26])
def test_beam_refine_argmax(L):
    """'edit' mode at W = 1: every hypothesis becomes the arg-max reading of its logits.  amax follows the rule everywhere, lp_max is the
    float64 log-soft-max at it (4e-5, the term bound of tests/test_beam_refine.py; NaN where the row's log-sum is not a number), and the
    state is the extended restatement's: a row whose score is not a number comes out dead."""
    C, pad_id = 95, 96
    for name, rows in families(C).items():
        x = _as_batch(rows, L)
        n = x.shape[0]
        got = _refine_op(x, n, 1, L, 'edit')
        flat = x.view(-1, C)
        want_amax = torch.tensor(picks(flat)).view(n, L)
        assert torch.equal(got['amax'].long(), want_amax), name
        lp = torch.log_softmax(flat.double(), -1).gather(1, want_amax.view(-1, 1)).view(n, L)
        assert torch.equal(torch.isnan(lp), _no_softmax(flat).view(n, L))
        assert _same_nonfinite(got['lp_max'].double(), lp), name
        assert torch.allclose(got['lp_max'].double(), lp, rtol=0, atol=4e-5, equal_nan=True), name
        want = RR.refine_rows(x, 'edit', _refine_rows(n, L, pad_id), n, 1, 0, pad_id)
        assert got['tokens'].tolist() == [img.tokens[0] for img in want], name
        assert got['lengths'].tolist() == [img.lengths[0] for img in want] and got['finished'].tolist() == [img.finished[0] for img in want], name
        for g, img in zip(got['scores'].tolist(), want):
            assert g == img.scores[0] if img.scores[0] == -INF else abs(g - img.scores[0]) <= 4e-5 * (img.last[0] + 1), name
        dead = sum(img.scores[0] == -INF for img in want)
        assert (dead > 0) == (name in ('nan', 'inf')), name


@pytest.mark.gpu
@pytest.mark.parametrize('mode', ['edit', 'score'])
def test_beam_refine_ranks_a_row_without_a_score_last(mode):
    """Three beams per image; the middle one's logits hold a NaN (image 0), a +inf (image 1), a row of -inf (image 2) at a summed position:
    it comes out dead and last, the other two keep their order."""
    C, W, L, pad_id = 95, 3, 4, 96
    x = _base(3 * W * L, C, 11).view(3 * W, L, C)
    x[:, :, 5] = 2.0 + 0.5 * torch.arange(3 * W).view(-1, 1)      # class 5 wins everywhere, by another margin per row: no ties, no <eos>
    x[1, 2, 40], x[4, 0, 41], x[7, 3] = NAN, INF, -INF
    tokens = torch.full((3 * W, L), 5, dtype=torch.int32)
    rows = RR.Rows(tokens.tolist(), [-1.0] * 9, [0] * 9, [L] * 9, [-1] * 9, [-1] * 9, [float(r) for r in range(9)])
    want = RR.refine_rows(x, mode, rows, 3, W, 0, pad_id)
    got = _refine_op(x, 3, W, L, mode, tokens=tokens)
    for b, img in enumerate(want):
        sl = slice(b * W, (b + 1) * W)
        assert img.scores[2] == -INF and img.src[2] == 1 and all(g > 1e-3 for g in img.gaps)
        assert got['ar'][sl].tolist() == [float(b * W + s) for s in img.src]
        assert got['tokens'][sl].tolist() == img.tokens and got['lengths'][sl].tolist() == img.lengths
        for g, w in zip(got['scores'][sl].tolist(), img.scores):
            assert g == w if w == -INF else abs(g - w) <= 4e-5 * L


@pytest.mark.gpu
@pytest.mark.parametrize('grid', AR.GRIDS)
def test_attention_geometry_peak(grid):
    """The placement sweep and every pair tie over the S weights of a map: the peak is the first maximum, peak_mass its value.  The weights
    are multiples of 2^-12 (distinct but for the planted 1/4), so nothing rounds."""
    from test_attn_map import _geometry_op
    gh, gw, ph, pw = grid
    S = gh * gw
    every = list(itertools.combinations(range(S), 2))
    for name, plants in (('placement', [[(i, 0.25)] for i in range(S)]), ('pair_ties', [[(i, 0.25), (j, 0.25)] for i, j in every])):
        n = len(plants)
        a = (1.0 + torch.rand(n, S, generator=torch.Generator().manual_seed(S)).argsort(-1).float()) / 4096.0
        idx = torch.tensor([[r, c] for r, entries in enumerate(plants) for c, _ in entries])
        a[idx[:, 0], idx[:, 1]] = 0.25
        want = [entries[0][0] for entries in plants]
        assert picks(a[:: max(1, n // 500)]) == want[:: max(1, n // 500)] and torch.argmax(a, -1).tolist() == want
        _, _, peak, mass = _geometry_op(a.view(n, 1, S).numpy(), [0] * n, *grid)
        assert peak.cpu().view(-1).tolist() == want, name
        assert (mass.cpu() == 0.25).all(), name
        ref = AR.geometry(a.view(n, 1, S).numpy(), [0] * n, *grid)
        assert (ref[2].reshape(-1) == np.asarray(want)).all() and (ref[3] == 0.25).all()


def _beam_state(W, C, seed):
    """Four images of W live unfinished beams at step 3: image 0 has a NaN logit in one beam's row, image 1 a +inf, image 2 a row of -inf,
    image 3 one of these in every row."""
    from test_beam import LDT
    B, step, pad_id, bos_id = 4, 3, C + 1, C
    g = torch.Generator().manual_seed(seed)
    rows = B * W
    logits = torch.stack([(torch.randperm(C, generator=g).float() - C // 2) * 0.25 for _ in range(rows)])
    hit = W // 2
    logits[0 * W + hit, 17], logits[1 * W + hit, 64], logits[2 * W + hit] = NAN, INF, -INF
    for w in range(W):
        r = 3 * W + w
        if w % 3 == 0:
            logits[r, (5 * w) % C] = NAN
        elif w % 3 == 1:
            logits[r, (5 * w) % C] = INF
        else:
            logits[r] = -INF
    logits[0, 3] = -INF      # a -inf class in a finite row: that class alone is no candidate
    tok = torch.full((rows, LDT), pad_id, dtype=torch.int64)
    tok[:, 0] = bos_id
    tok[:, 1:step + 1] = torch.randint(1, C, (rows, step), generator=g)
    scores = -1.0 - 7.0 * torch.rand(rows, generator=g)
    scores[torch.arange(3) * W + hit] = -0.25      # the best beam of its image: were its row ranked at all, it would come first
    return B, step, logits, tok, scores, torch.zeros(rows, dtype=torch.int64), torch.full((rows,), step, dtype=torch.int64)


@pytest.mark.gpu
@pytest.mark.parametrize('W', [1, 4, 16])
def test_beam_step_ranks_no_candidate_that_is_not_finite(W):
    """a candidate whose value is not finite is not a candidate.  A row with a NaN or a +inf logit, or of nothing but
    -inf, has a log-sum that is not a number and offers nothing; a slot left without a candidate is dead."""
    from test_beam import LDT, _compare_step, _reference_step, _run_step
    C, eos_id = 95, 0
    pad_id = C + 1
    for attempt in range(200):      # re-drawn on the CPU until every decision is clear of the score bound
        B, step, logits, tok, scores, finished, lengths = _beam_state(W, C, 1000 * attempt + W)
        want = _reference_step(logits, tok, scores, finished, lengths, B, W, step, eos_id, pad_id)
        if min(st.gap for st in want) >= 1e-3:
            break
    assert min(st.gap for st in want) >= 1e-3
    hit = W // 2
    for b in range(3):
        assert hit not in want[b].parent and (W == 1) == (want[b].parent == [-1])      # the row offers nothing; its image goes on without it
        assert all(math.isfinite(s) for s, p in zip(want[b].scores, want[b].parent) if p >= 0)
    assert want[3].parent == [-1] * W and want[3].scores == [-INF] * W and want[3].picked == [pad_id] * W
    assert all(not (p == 0 and c == 3) for p, c in zip(want[0].parent, want[0].picked))
    got = _run_step(logits, tok, scores, finished, lengths, B, W, C, step, LDT, eos_id, pad_id)
    assert not torch.isnan(got['scores']).any()
    for key in ('picked', 'tok'):
        ids = got[key] if key == 'picked' else got[key][:, 1:]
        assert (((ids >= 0) & (ids < C)) | (ids == pad_id)).all(), key
    _compare_step(got, want, B, W, step)


# -------------------------------------------------------------------------------------------------------------------
# 3. picks fused into the decoder: the head shapes the model's own logits
# -------------------------------------------------------------------------------------------------------------------
# 'tie' is the pair (7, 70): lanes 7 and 6 of one quad, which a reduction that keeps its own value on a tie, or that loses a quad step,
# still gets right by the order of its steps (tried: both broken builds pass it).  'tie_rows' is (43, 67): lane 43 of the third DPP row
# against lane 3 of the first, both in the half of their quad pair that a missing quad step loses; both broken builds fail it.
TIES = {'tie': (7, 70), 'tie_rows': (43, 67)}
CASES = {'tie': 7, 'tie_rows': 43, 'nan': 33, 'inf': 33, 'neginf': 0}      # the class every position picks
WRONG = {'tie': 70, 'tie_rows': 67, 'nan': 60}                             # what a broken first-of-two rule would pick instead
PLANTED = {'tie': [7, 70], 'tie_rows': [43, 67], 'nan': [33, 60], 'inf': [33]}
CASE_MODELS = [('tie', 'parseq-tiny'), ('tie', 'parseq'), ('tie_rows', 'parseq-tiny'), ('nan', 'parseq-tiny'), ('inf', 'parseq-tiny'),
               ('neginf', 'parseq-tiny')]
BATCHES = (1, 5, 17)
DECODES = ((True, 0), (True, 1), (False, 1))
TOL = {'fp32': 1e-3, 'bf16x3': 1e-3, 'bf16': 3e-2}        # tests/test_hip_parity.py: test_forward_fp32_matches_reference, test_forward_bf16
BF16_VS_EXACT = 6e-2


@functools.lru_cache(maxsize=None)
def _shaped_weights(case, name):
    sd = synth_state_dict(CONFIGS[name], 0)
    w, b = sd['head.weight'], sd['head.bias']
    if case in TIES:
        i, j = TIES[case]
        w[i], w[j] = 0.0, 0.0
        b[i] = b[j] = 48.0       # exact in bf16; a zero weight row: both logits are 48.0 at every position, in every precision
    elif case == 'nan':
        b[33] = b[60] = NAN
    elif case == 'inf':
        b[33] = INF
    else:
        b[:] = -INF
    return sd


@functools.lru_cache(maxsize=None)
def _crops(name):
    return synth_images(max(BATCHES), CONFIGS[name], seed=4242)


@functools.lru_cache(maxsize=None)
def _oracle_logits(case, name, decode_ar, refine_iters, testing, rounding, teacher=None):
    """The oracle's logits of all 17 crops (rows are independent: a smaller batch is a prefix), and the tokens it fed back.  `teacher`: feed
    this class at every position instead of the pick."""
    cfg = CONFIGS[name]
    x = _crops(name)
    trace = O.Trace()
    kw = {}
    if teacher is not None:
        t = torch.full((x.shape[0], cfg.max_label_length + 1), teacher, dtype=torch.long)
        t[:, 0] = cfg.bos_id
        kw = dict(teacher_tokens=t, teacher_refine_tokens=[t] * refine_iters)
    with torch.inference_mode():
        out = O.forward(_shaped_weights(case, name), cfg, x, None if testing else cfg.max_label_length, decode_ar=decode_ar,
                        refine_iters=refine_iters, rounding=rounding, trace=trace, **kw)
    return out, trace


def _expected(case, name, decode_ar, refine_iters, testing, rounding):
    """Only the all -inf head ever stops early (every crop reads <eos> at step 0), so every other case has one oracle run per decode."""
    return _oracle_logits(case, name, decode_ar, refine_iters, bool(testing and decode_ar and case == 'neginf'), rounding)[0]


@pytest.mark.parametrize('case,name', CASE_MODELS)
def test_oracle_traces_of_the_shaped_heads(case, name):
    cfg = CONFIGS[name]
    cls = CASES[case]
    out, trace = _oracle_logits(case, name, True, 1, False, None)
    assert out.shape == (17, 26, 95)
    assert (trace.ar_tokens[:, 0] == cfg.bos_id).all() and (trace.ar_tokens[:, 1:] == cls).all()
    assert (trace.refine_tokens[0][:, 1:] == cls).all()
    for logits in (trace.ar_logits, out, _oracle_logits(case, name, False, 1, False, None)[0]):
        assert picks(logits.reshape(-1, 95)) == [cls] * (17 * 26)
        if case in TIES:
            assert (logits[..., PLANTED[case]] == 48.0).all()
            rest = logits.clone()
            rest[..., PLANTED[case]] = 0.0
            assert rest.abs().max() < 24.0
        elif case == 'nan':
            assert torch.equal(torch.isnan(logits).nonzero()[:, 2].unique(), torch.tensor([33, 60]))
        elif case == 'inf':
            assert torch.equal((logits == INF).nonzero()[:, 2].unique(), torch.tensor([33])) and not torch.isnan(logits).any()
        else:
            assert (logits == -INF).all()
    if case == 'neginf':
        early = _oracle_logits(case, name, True, 0, True, None)[0]
        assert early.shape == (17, 1, 95)      # every crop reads <eos> at step 0: the early-exit length is 1


@pytest.mark.parametrize('case,name', [cm for cm in CASE_MODELS if cm[0] in WRONG])
@pytest.mark.parametrize('rounding', [None, 'bf16'])
def test_a_wrong_pick_shows_in_the_next_logits(case, name, rounding):
    """The other logits depend on the token fed back: the oracle teacher-forced with the wrong class differs from the right run, at the
    finite classes of every later position of every crop, by at least ten times the tolerance the device is compared at."""
    tol = TOL['bf16' if rounding else 'fp32']
    for decode_ar, refine_iters in ((True, 0), (True, 1)):
        right = _oracle_logits(case, name, decode_ar, refine_iters, False, rounding)[0]
        wrong = _oracle_logits(case, name, decode_ar, refine_iters, False, rounding, teacher=WRONG[case])[0]
        d = torch.where(torch.isfinite(right) & torch.isfinite(wrong), (right - wrong).abs(), torch.zeros(()))
        d[..., PLANTED[case]] = 0.0
        per_position = d.amax(-1)[:, 1:] if refine_iters == 0 else d.amax(-1)[:, 2:]      # the cloze pass of position 1 never sees token 1
        print(f'[{case} {name} {rounding} AR+{refine_iters}] least per-position difference {per_position.min().item():.3e} (needs {10 * tol:.0e})')
        assert per_position.min() >= 10 * tol


@pytest.fixture(scope='module')
def shaped_model():
    """`shaped_model(case, name, precision)`: the device model of a case, built once for the module and dropped with it."""
    from parseq_amd import create_model
    built = {}

    def get(case, name, precision):
        if (case, name, precision) not in built:
            m = create_model(name, decode_ar=True, refine_iters=1, precision=precision)
            m.model.load_state_dict(_shaped_weights(case, name))
            built[case, name, precision] = m.eval().to(DEV)
        return built[case, name, precision]
    yield get
    built.clear()


def _check_logits(tag, got, want, exact, precision):
    assert got.shape == want.shape, f'{tag}: shape {tuple(got.shape)}, oracle {tuple(want.shape)}'
    assert _same_nonfinite(got, want), f'{tag}: non-finite values differ in place or sign'
    finite = torch.isfinite(want)
    err = (got - want)[finite].abs().max().item() if finite.any() else 0.0
    assert err <= TOL[precision], f'{tag}: max |d| {err:.3e} > {TOL[precision]:.0e}'
    if precision == 'bf16':
        gap = (got - exact)[finite].abs().max().item() if finite.any() else 0.0
        assert gap <= BF16_VS_EXACT, f'{tag}: max |d| against the exact oracle {gap:.3e}'
    assert torch.equal(RR.first_argmax_rows(got), RR.first_argmax_rows(want)), f'{tag}: picks'      # (`pick`, vectorised: section 1 holds them equal)
    return err


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('case,name', CASE_MODELS)
def test_fused_picks(case, name, precision, shaped_model):
    cfg = CONFIGS[name]
    m = shaped_model(case, name, precision)
    rounding = 'bf16' if precision == 'bf16' else None
    worst = 0.0
    for decode_ar, refine_iters in DECODES:
        m.model.decode_ar, m.model.refine_iters = decode_ar, refine_iters
        for testing in (False, True):
            want_all = _expected(case, name, decode_ar, refine_iters, testing, rounding)
            exact_all = _expected(case, name, decode_ar, refine_iters, testing, None)
            for n in BATCHES:
                x = _crops(name)[:n].to(DEV)
                for slot in (None, 0):
                    with torch.inference_mode():
                        got = m(x, None if testing else cfg.max_label_length, slot=slot)
                    torch.cuda.synchronize()
                    tag = f'{case} {name} {precision} {"AR" if decode_ar else "NAR"}+{refine_iters} testing={testing} batch {n} slot {slot}'
                    worst = max(worst, _check_logits(tag, got.float().cpu(), want_all[:n], exact_all[:n], precision))
    if case == 'neginf':
        m.model.decode_ar, m.model.refine_iters = True, 0
        with torch.inference_mode():
            assert m(_crops(name)[:5].to(DEV)).shape == (5, 1, 95)
    m.model.decode_ar, m.model.refine_iters = True, 1
    print(f'[fused picks {case} {name} {precision}] worst max|d| against the oracle {worst:.3e} (bar {TOL[precision]:.0e})')


@pytest.mark.gpu
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('case,name', CASE_MODELS)
def test_device_reading_of_shaped_logits(case, name, precision, shaped_model):
    """`tokenizer.read` and the reading of `lexicon_match` on the device logits of each case against the host's
    `Tokenizer.decode(logits.softmax(-1))` and the oracle's post-processing of those logits."""
    from parseq_amd.lexicon import Lexicon
    cfg = CONFIGS[name]
    m = shaped_model(case, name, precision)
    m.model.decode_ar, m.model.refine_iters = True, 1
    x = _crops(name)[:5].to(DEV)
    with torch.inference_mode():
        logits = m(x, cfg.max_label_length)
        labels, conf = m.tokenizer.read(logits)
        res = m.lexicon_match(x, Lexicon(['abc', 'Hello', 'x'], m.tokenizer), 2, rescore=False)
    torch.cuda.synchronize()
    host = logits.float().cpu()
    want_labels, want_probs = m.tokenizer.decode(host.softmax(-1))
    want_conf = torch.stack([p.prod() for p in want_probs])
    assert labels == want_labels
    assert labels == [m.tokenizer._itos[CASES[case]] * 26 if case in TIES else ''] * 5
    assert _same_nonfinite(conf, want_conf) and torch.allclose(conf, want_conf, rtol=2e-5, atol=1e-30, equal_nan=True)
    assert bool(torch.isnan(want_conf).all()) == (case not in TIES)
    ids, lengths, _, _ = O.postprocess(host, cfg.eos_id)
    assert torch.equal(res.reading_tokens.cpu().long(), ids) and torch.equal(res.reading_lengths.cpu().long(), lengths)
    assert lengths.tolist() == [26 if case in TIES else 0] * 5
