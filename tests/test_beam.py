"""GPU tests of beam-search AR decoding: the selection kernel alone against the CPU restatement
(tests/beam_reference.py), the whole search's arithmetic against the oracle's teacher-forced logits, its decisions against a replay of the
restatement from the traced logits, its result against the oracle-driven restatement, the Python surface, the refusals and read.py.

The score bound everywhere: 4e-5 * (step + 1).  One step adds to a beam's fp32 score one log-soft-max term whose fp32 sum of at most 256
exponentials carries a relative error of at most 256 * 2^-24 ~ 1.5e-5, the rest (the max, the log, two subtractions, one addition at
|score| < 64) a few ulp — loose on purpose; the tests print the measured worst."""
import ctypes as C
import functools
import math

import pytest
import torch

import beam_reference as R
from gpu_util import DEV, make_model, native
from oracle import parseq_oracle as O
from oracle.synth import CONFIGS, synth_images, synth_state_dict

pytestmark = pytest.mark.gpu

NEG_INF = float('-inf')
LDT = 32
# The synthetic head's <eos> bias for the whole-search tests, and the image seeds, chosen ON THE CPU with the oracle-driven restatement alone
# (W = 3, max_length = 5, 8 crops): at 2.25 it finishes 58 % (parseq-tiny, seed 101) / 50 % (parseq, seed 105) of the final hypotheses before
# the last step and leaves 33 % / 38 % unfinished, and the smallest adjacent-rank gap over all 48 (image, step) decisions is 2.7e-3 / 1.4e-2,
# 19 / 32 times the skip threshold — test_whole_search_decisions asserts all of this again.
EOS_BIAS = 2.25
SEARCH_SEED = {'parseq-tiny': 101, 'parseq': 105}
SEARCH_B, SEARCH_W, SEARCH_MAXLEN = 8, 3, 5
# Against the independent search: 32 crops, W = 2, max_length = 3; with seed 205 the oracle-driven restatement leaves 26 of 32 images (81 %)
# with every gap above 4 * num_steps * 1e-3
INDEP_SEED, INDEP_B, INDEP_W, INDEP_MAXLEN = 205, 32, 2, 3


def score_bound(step):
    return 4e-5 * (step + 1)


# -------------------------------------------------------------------------------------------------------------------
# 1. the step kernel alone
# -------------------------------------------------------------------------------------------------------------------
def _run_step(logits, tok, scores, finished, lengths, B, W, C, step, ldt, eos_id, pad_id):
    nat, lib = native()
    d = dict(tok=tok.to(DEV, torch.int32).contiguous(), scores=scores.to(DEV, torch.float32).contiguous(),
             finished=finished.to(DEV, torch.uint8).contiguous(), lengths=lengths.to(DEV, torch.int32).contiguous(),
             parent=torch.full((B * W,), -7, dtype=torch.int32, device=DEV), picked=torch.full((B * W,), -7, dtype=torch.int32, device=DEV))
    lg = logits.to(DEV, torch.float32).contiguous()
    with nat.guard(lg):
        nat.check(lib.parseq_op_beam_step(nat.ptr(lg), B, W, C, step, nat.ptr(d['tok']), ldt, nat.ptr(d['scores']), nat.ptr(d['finished']),
                                          nat.ptr(d['lengths']), nat.ptr(d['parent']), nat.ptr(d['picked']), eos_id, pad_id, nat.stream_ptr(lg)))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def _reference_step(logits, tok, scores, finished, lengths, B, W, step, eos_id, pad_id):
    out = []
    for b in range(B):
        rows = slice(b * W, (b + 1) * W)
        out.append(R.step_image(logits[rows], [float(s) for s in scores[rows]], finished[rows].tolist(), lengths[rows].tolist(),
                                tok[rows].tolist(), step, eos_id, pad_id))
    return out


def _compare_step(got, want, B, W, step):
    worst = 0.0
    for b, st in enumerate(want):
        rows = slice(b * W, (b + 1) * W)
        assert got['parent'][rows].tolist() == st.parent
        assert got['picked'][rows].tolist() == st.picked
        assert got['tok'][rows].tolist() == st.hist
        assert got['finished'][rows].tolist() == st.finished
        assert got['lengths'][rows].tolist() == st.lengths
        for g, w in zip(got['scores'][rows].tolist(), st.scores):
            if w == NEG_INF:
                assert g == NEG_INF
            else:
                worst = max(worst, abs(g - w))
    assert worst <= score_bound(step), f'score error {worst:.3e} > {score_bound(step):.3e}'
    return worst


def _state(kind, B, W, C, ldt, seed, eos_id, pad_id, bos_id):
    """Inputs of one step: logits on a 0.25 grid (a permutation per row, |logit| <= 30), distinct per-beam scores."""
    g = torch.Generator().manual_seed(seed)
    rows = B * W
    logits = torch.stack([(torch.randperm(C, generator=g).float() - C // 2) * 0.25 for _ in range(rows)])
    assert logits.abs().max() <= 30
    tok = torch.full((rows, ldt), pad_id, dtype=torch.int64)
    tok[:, 0] = bos_id
    scores = torch.full((rows,), NEG_INF)
    finished = torch.zeros(rows, dtype=torch.int64)
    lengths = torch.zeros(rows, dtype=torch.int64)
    if kind == 'start':
        scores[::W] = 0.0
        return 0, logits, tok, scores, finished, lengths
    step = 3
    for r in range(rows):
        w = r % W
        what = {'middle': ('live', 'finished', 'dead')[w % 3], 'all_finished': 'finished',
                'finished_and_dead': 'dead' if (w == W - 1 and W > 1) else 'finished'}[kind]
        if what == 'dead':
            continue
        scores[r] = -1.0 - 7.0 * torch.rand((), generator=g).item()
        if what == 'live':
            tok[r, 1:step + 1] = torch.randint(1, C, (step,), generator=g)
            lengths[r] = step
        else:
            n = int(torch.randint(0, step, (), generator=g))
            tok[r, 1:n + 1] = torch.randint(1, C, (n,), generator=g)
            tok[r, n + 1] = eos_id
            finished[r], lengths[r] = 1, n
    return step, logits, tok, scores, finished, lengths


@pytest.mark.parametrize('W', [1, 2, 3, 5, 16])
@pytest.mark.parametrize('C', [37, 95, 201])
def test_step_kernel_matches_the_restatement(C, W):
    eos_id, bos_id, pad_id = 0, C, C + 1
    worst, least_gap = 0.0, math.inf
    for B in (1, 3):
        for kind in ('start', 'middle', 'all_finished', 'finished_and_dead'):
            # inputs are re-drawn (on the CPU, before anything runs) until every adjacent-rank gap among the best W + 1 candidates is >= 1e-3
            for attempt in range(200):
                step, logits, tok, scores, finished, lengths = _state(kind, B, W, C, LDT, 1000 * attempt + 17 * C + W + B, eos_id, pad_id, bos_id)
                want = _reference_step(logits, tok, scores, finished, lengths, B, W, step, eos_id, pad_id)
                if min(st.gap for st in want) >= 1e-3:
                    break
            gap = min(st.gap for st in want)
            assert gap >= 1e-3, (kind, B, gap)
            least_gap = min(least_gap, gap)
            got = _run_step(logits, tok, scores, finished, lengths, B, W, C, step, LDT, eos_id, pad_id)
            worst = max(worst, _compare_step(got, want, B, W, step) / score_bound(step))
            again = _run_step(logits, tok, scores, finished, lengths, B, W, C, step, LDT, eos_id, pad_id)
            for k in got:
                a, b = (got[k].view(torch.int32), again[k].view(torch.int32)) if got[k].dtype == torch.float32 else (got[k], again[k])
                assert torch.equal(a, b), f'{k}: two runs differ'
    print(f'[beam step C={C} W={W}] worst score error {worst:.3f} of the bound, least gap {least_gap:.2e}')


def test_step_kernel_without_room_for_the_pick():
    """Rows of step + 1 tokens (the plan's rows at num_steps == 32): the histories are re-parented, the pick is reported in picked_out only."""
    C, W, B, eos_id, bos_id, pad_id = 37, 3, 2, 0, 37, 38
    step, logits, tok, scores, finished, lengths = _state('middle', B, W, C, 4, 5, eos_id, pad_id, bos_id)
    want = _reference_step(logits, tok, scores, finished, lengths, B, W, step, eos_id, pad_id)
    assert min(st.gap for st in want) >= 1e-3
    got = _run_step(logits, tok, scores, finished, lengths, B, W, C, step, 4, eos_id, pad_id)
    _compare_step(got, want, B, W, step)


def test_step_kernel_ties():
    """Equal scores: a duplicated beam (same score, same logits row), and a finished carry that repeats a fresh candidate's score exactly
    (a row of one 0 and -200 elsewhere: its log-soft-max is 0 / -200 exactly in fp32 and in float64)."""
    C, eos_id, bos_id, pad_id = 37, 0, 37, 38
    step, logits, tok, scores, finished, lengths = _state('middle', 1, 3, C, LDT, 3, eos_id, pad_id, bos_id)
    for r in (0, 1, 2):      # three live beams, 0 and 1 the same but for their histories
        scores[r], finished[r], lengths[r] = -2.0 - 0.3 * (r // 2), 0, step
        tok[r, 1:step + 1] = torch.tensor([1 + r, 2, 3])
        tok[r, step + 1:] = pad_id
    logits[1] = logits[0]
    for W in (2, 3):
        lg, tk, sc, fi, le = logits[:W], tok[:W], scores[:W], finished[:W], lengths[:W]
        want = _reference_step(lg, tk, sc, fi, le, 1, W, step, eos_id, pad_id)
        cands = R.rank_candidates(lg, [float(s) for s in sc], fi.tolist())[:W + 1]
        assert want[0].gap == 0.0 and all(a[0] - b[0] == 0.0 or a[0] - b[0] >= 1e-3 for a, b in zip(cands, cands[1:]))
        assert want[0].parent[:2] == [0, 1] and want[0].picked[0] == want[0].picked[1]
        _compare_step(_run_step(lg, tk, sc, fi, le, 1, W, C, step, LDT, eos_id, pad_id), want, 1, W, step)
    for carry_first in (False, True):
        live, done = (1, 0) if carry_first else (0, 1)
        lg = torch.full((2, C), -200.0)
        lg[live, 5] = 0.0
        sc = torch.tensor([-2.5, -2.5])
        fi, le = torch.zeros(2, dtype=torch.int64), torch.zeros(2, dtype=torch.int64)
        tk = torch.full((2, LDT), pad_id, dtype=torch.int64)
        tk[:, 0] = bos_id
        tk[live, 1:4] = torch.tensor([4, 5, 6])
        tk[done, 1:3] = torch.tensor([7, eos_id])
        fi[done], le[done], le[live] = 1, 1, 3
        want = _reference_step(lg, tk, sc, fi, le, 1, 2, 3, eos_id, pad_id)
        assert want[0].scores == [-2.5, -2.5] and want[0].parent == [0, 1]
        assert want[0].picked == ([pad_id, 5] if carry_first else [5, pad_id])
        _compare_step(_run_step(lg, tk, sc, fi, le, 1, 2, C, 3, LDT, eos_id, pad_id), want, 1, 2, 3)


# -------------------------------------------------------------------------------------------------------------------
# 2 - 4. the whole search
# -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _weights(name):
    return synth_state_dict(CONFIGS[name], 0, eos_bias=EOS_BIAS)


@functools.lru_cache(maxsize=None)
def _model(name, precision):
    from parseq_amd import create_model
    m = create_model(name, decode_ar=True, refine_iters=0, precision=precision)
    m.model.load_state_dict(_weights(name))
    return m.eval().to(DEV)


@functools.lru_cache(maxsize=None)
def _search(name, precision):
    """One traced search per (model, precision), shared by the arithmetic and the decision tests; everything on the host."""
    cfg = CONFIGS[name]
    images = synth_images(SEARCH_B, cfg, seed=SEARCH_SEED[name])
    m = _model(name, precision)
    with torch.inference_mode():
        res = m.model.beam_search(m.tokenizer, images.to(DEV), SEARCH_W, SEARCH_MAXLEN, trace=True)
    torch.cuda.synchronize()
    return images, {k: v.cpu() for k, v in vars(res).items()}


@functools.lru_cache(maxsize=None)
def _oracle_search(name):
    cfg = CONFIGS[name]
    images = synth_images(SEARCH_B, cfg, seed=SEARCH_SEED[name])
    return R.beam_search(R.oracle_step_logits(_weights(name), cfg, images, SEARCH_W), SEARCH_B, SEARCH_W, SEARCH_MAXLEN + 1, cfg.bos_id, cfg.eos_id, cfg.pad_id)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_whole_search_arithmetic(name, precision):
    """Every step's traced logits are the oracle's teacher-forced logits for the traced histories and the row's image (row // W): a wrong
    re-parenting, another image's memory or a wrong position would show here.  fp32 / bf16x3: 1e-3; bf16: the rounding-aware oracle, 3e-2
    (the bars of tests/test_hip_parity.py)."""
    cfg = CONFIGS[name]
    images, res = _search(name, precision)
    rounding, tol = (None, 1e-3) if precision != 'bf16' else ('bf16', 3e-2)
    step_logits = R.oracle_step_logits(_weights(name), cfg, images, SEARCH_W, rounding)
    steps = SEARCH_MAXLEN + 1
    assert res['trace_logits'].shape == (steps, SEARCH_B * SEARCH_W, cfg.num_tokens - 2)
    worst = 0.0
    for i in range(steps):
        hist = res['trace_tokens_in'][i].long()
        assert (hist[:, 0] == cfg.bos_id).all() and (hist[:, i + 1:] == cfg.pad_id).all()
        want = step_logits(hist[:, :i + 1])
        worst = max(worst, (res['trace_logits'][i] - want).abs().max().item())
    print(f'[beam arithmetic {name} {precision}] worst |dlogit| over {steps} steps {worst:.3e} (bar {tol:.0e})')
    assert worst <= tol


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_whole_search_decisions(name, precision):
    """The restatement replayed from the traced logits themselves makes the decisions the device made: parents and histories at every step,
    the final outputs, scores within the step bound.  A decision whose float64 gap is below twice that bound is skipped and its image drops
    out from there on; at most 2 % of the (image, step) decisions may be (here: none of 48)."""
    cfg = CONFIGS[name]
    _, res = _search(name, precision)
    steps, B, W = SEARCH_MAXLEN + 1, SEARCH_B, SEARCH_W
    # the crops and the <eos> bias, checked on the CPU with the oracle's logits
    ora = _oracle_search(name)
    limits = torch.tensor([2 * score_bound(i) for i in range(steps)], dtype=torch.float64)
    assert int((ora.gaps < limits).sum()) <= 0.02 * B * steps
    early = ((ora.finished == 1) & (ora.lengths < steps - 1)).double().mean().item()
    unfinished = (ora.finished == 0).double().mean().item()
    assert early >= 0.25 and unfinished >= 0.25, (early, unfinished)

    rep = R.beam_search(lambda h: res['trace_logits'][h.shape[1] - 1], B, W, steps, cfg.bos_id, cfg.eos_id, cfg.pad_id)
    valid = torch.ones(B, dtype=torch.bool)
    skipped, worst = 0, 0.0
    for i in range(steps):
        assert torch.equal(res['trace_tokens_in'][i].long().view(B, W, steps)[valid], rep.tokens_in[i].view(B, W, steps)[valid]), f'histories of step {i}'
        for b in range(B):
            if valid[b] and rep.gaps[b, i] < limits[i]:
                valid[b] = False
                skipped += 1
        assert torch.equal(res['trace_parent'][i].long().view(B, W)[valid], rep.parents[i][valid]), f'parents of step {i}'
        d = (res['trace_score'][i].double().view(B, W)[valid] - rep.step_scores[i][valid]).abs()
        d = d[~torch.isnan(d)]      # -inf against -inf
        assert torch.equal(res['trace_score'][i].view(B, W)[valid] == NEG_INF, rep.step_scores[i][valid] == NEG_INF)
        worst = max(worst, d.max().item() / score_bound(i))
        assert d.max().item() <= score_bound(i), f'step {i}: score error {d.max().item():.3e}'
    print(f'[beam decisions {name} {precision}] skipped {skipped} of {B * steps}, worst score error {worst:.3f} of the bound, least gap {rep.gaps.min().item():.2e}')
    assert skipped <= 0.02 * B * steps
    assert torch.equal(res['tokens'].long()[valid], rep.tokens[valid])
    assert torch.equal(res['lengths'].long()[valid], rep.lengths[valid]) and torch.equal(res['finished'].long()[valid], rep.finished[valid])
    assert torch.equal(res['scores'][valid], res['trace_score'][-1].view(B, W)[valid])


@functools.lru_cache(maxsize=None)
def _independent_reference():
    cfg = CONFIGS['parseq']
    images = synth_images(INDEP_B, cfg, seed=INDEP_SEED)
    return images, R.beam_search(R.oracle_step_logits(_weights('parseq'), cfg, images, INDEP_W), INDEP_B, INDEP_W, INDEP_MAXLEN + 1, cfg.bos_id, cfg.eos_id, cfg.pad_id)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_against_the_oracle_driven_search(precision):
    """32 crops, W = 2, 4 steps against the restatement driven by the CPU oracle's own logits.  Compared: every image whose smallest gap there
    exceeds 4 * num_steps * 1e-3 — twice the worst drift two accumulated scores can have under the 1e-3 logit bar.  With image seed 205 that
    is 26 of the 32 images (81 %; picked on the CPU); at most half may be left out and at least 8 must be compared."""
    cfg = CONFIGS['parseq']
    images, want = _independent_reference()
    steps = INDEP_MAXLEN + 1
    keep = want.gaps.min(1).values > 4 * steps * 1e-3
    assert int(keep.sum()) >= max(8, INDEP_B // 2), int(keep.sum())
    m = _model('parseq', precision)
    with torch.inference_mode():
        res = m.model.beam_search(m.tokenizer, images.to(DEV), INDEP_W, INDEP_MAXLEN)
    torch.cuda.synchronize()
    assert torch.equal(res.tokens.cpu().long()[keep], want.tokens[keep])
    assert torch.equal(res.lengths.cpu().long()[keep], want.lengths[keep]) and torch.equal(res.finished.cpu().long()[keep], want.finished[keep])
    d = (res.scores.cpu().double()[keep] - want.scores[keep]).abs().max().item()
    print(f'[beam vs oracle-driven search {precision}] compared {int(keep.sum())} of {INDEP_B}, worst |dscore| {d:.3e} (bar {2 * steps * 1e-3:.0e})')
    assert d <= 2 * steps * 1e-3


# -------------------------------------------------------------------------------------------------------------------
# 5. surface
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_width_one_reads_what_forward_reads(name, precision, golden):
    g, _ = golden(name)
    m = make_model(name, precision, decode_ar=True, refine_iters=0)
    x = g['images'].to(DEV)
    with torch.inference_mode():
        want, _ = m.tokenizer.read(m(x))
        beams = m.tokenizer.decode_beams(m.beam_search(x, 1))
    assert [b[0][0] for b in beams] == want and all(len(b) == 1 for b in beams)


def test_surface_properties():
    name = 'parseq'
    cfg = CONFIGS[name]
    m = _model(name, 'bf16x3')
    g = torch.Generator().manual_seed(11)
    u8 = torch.randint(0, 256, (5, 3, 32, 128), generator=g, dtype=torch.uint8)
    xf = O.normalize_u8(u8).to(DEV)
    with torch.inference_mode():
        before = m(xf, 25).clone()
        a = m.beam_search(xf, 3, 6)
        after = m(xf, 25).clone()
        b = m.beam_search(xf, 3, 6)
        c = m.beam_search(u8.to(DEV), 3, 6)
    torch.cuda.synchronize()
    assert torch.equal(before, after)                   # neither the replaced memory K / V nor the histories in the plan leak into forward
    for other in (b, c):                                # a second call reproduces every bit; raw pixels give the normalised crops' result
        assert torch.equal(a.tokens, other.tokens) and torch.equal(a.scores.view(torch.int32), other.scores.view(torch.int32))
        assert torch.equal(a.lengths, other.lengths) and torch.equal(a.finished, other.finished)
    assert a.tokens.shape == (5, 3, 7) and a.tokens.dtype == torch.int32 and a.scores.shape == (5, 3) and a.finished.dtype == torch.uint8
    beams = m.tokenizer.decode_beams(a)
    assert len(beams) == 5
    for alts in beams:
        assert len(alts) == 3 and all(isinstance(s, str) and lp <= 0 for s, lp in alts)
        assert all(x[1] >= y[1] for x, y in zip(alts, alts[1:]))
    toks, lens, fin = a.tokens.cpu(), a.lengths.cpu(), a.finished.cpu()
    for i in range(5):
        for w in range(3):
            n = int(lens[i, w])
            assert (toks[i, w, :n] != cfg.eos_id).all() and (toks[i, w, :n] < cfg.num_tokens - 2).all()
            if fin[i, w]:
                assert toks[i, w, n] == cfg.eos_id and (toks[i, w, n + 1:] == cfg.pad_id).all()
            else:
                assert n == 7


# -------------------------------------------------------------------------------------------------------------------
# 6. refusals
# -------------------------------------------------------------------------------------------------------------------
def _raw_call(m, images, W, num_steps=4, short=0, plan_rows=None):
    """parseq_forward_beam through ctypes on the model's plan; returns (status, outputs untouched?)."""
    nat, lib = native()
    B = images.shape[0]
    plan = m.model._plan(plan_rows or B * max(W, 1))
    rows = B * max(W, 1)
    outs = [torch.full((rows * num_steps,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), -7.0, dtype=torch.float32, device=DEV),
            torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), 7, dtype=torch.uint8, device=DEV)]
    need = lib.parseq_beam_workspace_bytes(plan, B, W, num_steps)
    ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=DEV)
    status = lib.parseq_forward_beam(plan, nat.ptr(images), nat.dtype_code(images.dtype), B, W, num_steps, nat.ptr(outs[0]), nat.ptr(outs[1]),
                                     nat.ptr(outs[2]), nat.ptr(outs[3]), None, nat.ptr(ws), (need - short) if short else ws.numel(),
                                     nat.stream_ptr(images))
    torch.cuda.synchronize()
    untouched = bool((outs[0] == -7).all() and (outs[1] == -7.0).all() and (outs[2] == -7).all() and (outs[3] == 7).all())
    return status, untouched, need


def test_refusals():
    from parseq_amd import create_model
    nat, lib = native()
    cfg = CONFIGS['parseq-tiny']
    x = synth_images(4, cfg, seed=3).to(DEV)
    m = _model('parseq-tiny', 'bf16x3')
    for W in (0, 17, -1):
        with pytest.raises(ValueError, match='beam_width'):
            m.beam_search(x, W)
        assert _raw_call(m, x, W)[:2] == (-1, True)
    # more beams than classes
    small = create_model('parseq-tiny', charset_train='0123456789', precision='bf16x3').eval().to(DEV)
    with pytest.raises(ValueError, match='beam_width'):
        small.beam_search(x, 12)
    assert _raw_call(small, x, 12)[:2] == (-1, True)
    assert _raw_call(small, x, 11)[0] == 0                      # 11 classes: the widest search this head admits
    # more rows than the plan holds (the Python surface takes a plan of B * W rows, so only a C caller can get here)
    fresh = create_model('parseq-tiny', precision='bf16x3').eval().to(DEV)      # its first plan: 8 rows
    assert _raw_call(fresh, x, 4, plan_rows=8)[:2] == (-1, True)
    assert b'rows' in lib.parseq_last_error()
    # a short workspace
    status, untouched, need = _raw_call(m, x, 2, short=1)
    assert need > 0 and (status, untouched) == (-1, True) and b'workspace' in lib.parseq_last_error()
    assert _raw_call(m, x, 2)[0] == 0
    # a deeper decoder
    deep = create_model('parseq-tiny', dec_depth=2, precision='bf16x3').eval().to(DEV)
    with pytest.raises(ValueError, match='dec_depth'):
        deep.beam_search(x, 2)
    assert _raw_call(deep, x, 2)[:2] == (-1, True) and b'dec_depth' in lib.parseq_last_error()
    assert lib.parseq_beam_workspace_bytes(deep.model._plan(8), 4, 2, 4) == 0
    # ViTSTR has no AR loop
    vit = create_model('vitstr', precision='bf16').eval().to(DEV)
    xv = torch.zeros(2, 3, *vit.hparams.img_size, device=DEV)
    with pytest.raises(ValueError, match='ViTSTR'):
        vit.beam_search(xv, 2)
    assert _raw_call(vit, xv, 2)[:2] == (-1, True) and b'ViTSTR' in lib.parseq_last_error()


# -------------------------------------------------------------------------------------------------------------------
# 7. read.py
# -------------------------------------------------------------------------------------------------------------------
def test_read_cli_nbest(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip('PIL.Image')
    import read as read_cli
    from oracle.make_resize_golden import make_input
    files = []
    for i, (h, w) in enumerate([(40, 150), (32, 128), (64, 200)]):
        f = tmp_path / f'crop{i}.png'
        Image.fromarray(make_input(h, w, 1 - i % 2), 'RGB').save(f)
        files.append(str(f))
    m = _model('parseq', 'bf16x3')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    plain = [f'{f}: {label}' for f, label, _ in read_cli.read_files(m, files, DEV)]
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV])
    out = capsys.readouterr().out.splitlines()
    assert out[1:] == plain                                     # without the flag: the lines it printed before, nothing else
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--nbest', '3'])
    out = capsys.readouterr().out.splitlines()[1:]
    assert len(out) == 4 * len(files)
    with torch.inference_mode():
        best = read_cli.read_files_nbest(m, files, 3, None, DEV)
    for k, (f, alts) in enumerate(best):
        block = out[4 * k:4 * k + 4]
        assert block[0] == plain[k] and len(alts) == 3
        assert all(line.startswith('    ') for line in block[1:])
        assert block[1] == f'    {alts[0][1]:9.4f}  {alts[0][0]}'
        assert [line.split(None, 1)[1] if len(line.split(None, 1)) > 1 else '' for line in block[1:]] == [a[0] for a in alts]
    # a wider beam than the list
    read_cli.main(['pretrained=parseq', '--images', files[0], '--device', DEV, '--nbest', '2', '--beam', '5'])
    assert len(capsys.readouterr().out.splitlines()[1:]) == 3
