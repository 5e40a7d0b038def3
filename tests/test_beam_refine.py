"""GPU tests of the cloze refinement of beam hypotheses: the selection alone through `parseq_op_beam_refine` against
the CPU restatement (tests/beam_refine_reference.py), the refined search's arithmetic against the oracle's refinement pass, its decisions
against a replay of the restatement from the traced logits, W = 1 against `forward`, the 'score' mode, the unchanged plain searches, the
refusals and read.py.

The score bound everywhere: 4e-5 per summed term (tests/test_beam.py derives it for one log-soft-max term at |score| < 64), i.e.
4e-5 * (last + 1) for a score summed over positions 0 .. last.  The states of section 1 keep |score| < 128 (asserted): a row's tokens are
among the 8 best classes of their position, whose log-probability is above -3.9 on these logits, over at most 32 positions; up to 128 an
fp32 addition rounds by at most 7.7e-6, which with the 1.5e-5 of the term itself still leaves the 4e-5 loose.  The ranking and the duplicate
rule are compared only where every margin is an exact tie or at least twice the bound of a full-length sum, 8e-5 * L.

Seeds of the whole-model tests: the crops, weights and <eos> bias of tests/test_beam.py (seed 101 / 105, 2.25).  Checked ON THE CPU with the
oracle alone (`_oracle_refined`, asserted again in test_refined_search_decisions): over the two 'edit' iterations no (image, iteration)
has a margin in (0, 4.8e-4) — the smallest non-zero one is above 1e-1 for both models — so these seeds were kept; all 24 live
readings change in the first iteration and 6 of them merge as duplicates.  The exact ties are real: two hypotheses that differ in their
last token only have the same decoder input, hence the same refined reading at the same score, and the lower row stays.
"""
import functools
import math

import pytest
import torch

import beam_refine_reference as RR
from gpu_util import DEV, make_model, native
from oracle.synth import CONFIGS, synth_images, synth_state_dict
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.lexicon import Lexicon
from parseq_amd.tokenizer import Tokenizer

pytestmark = pytest.mark.gpu

NEG_INF = float('-inf')
LDT = 32
TERM_BOUND = 4e-5
EOS_BIAS = 2.25
SEARCH_SEED = {'parseq-tiny': 101, 'parseq': 105}
SEARCH_B, SEARCH_W, SEARCH_MAXLEN, SEARCH_ITERS = 8, 3, 5, 2
WHOLE_SCORE_BAR = 8e-3
MODE_CODE = {'score': 1, 'edit': 2}
TOK = Tokenizer(CHARSET_94_FULL)


def score_bound(last):
    return TERM_BOUND * (last + 1)


# -------------------------------------------------------------------------------------------------------------------
# 1. the selection alone
# -------------------------------------------------------------------------------------------------------------------
KINDS = ('random', 'dead_middle', 'finished_early', 'no_eos', 'identical', 'tie', 'all_dead', 'eos_at_0')
TOP = 8      # a row's own tokens come from the TOP best classes of their position: |score| stays below 128 at 32 positions


def _state(kind, B, W, C, L, seed):
    """Logits [B * W, L, C]: per (row, position) a permutation of a 0.25 grid times a factor in [0.5, 1] (distinct values, |logit| <= 30,
    another top probability everywhere), arranged so that the refined reading's <eos> falls where the kind wants it; and the rows' own
    state: tokens among the TOP best classes of their position, AR scores, flags, lengths."""
    eos_id, pad_id = 0, C + 1
    g = torch.Generator().manual_seed(seed)
    rows = B * W

    def rnd(lo, hi):
        return int(torch.randint(lo, hi, (), generator=g))
    logits = torch.stack([(torch.randperm(C, generator=g).float() - C // 2) * 0.25 for _ in range(rows * L)]).view(rows, L, C)
    logits = logits * (0.5 + 0.5 * torch.rand(rows, L, 1, generator=g))
    assert logits.abs().max() <= 30

    def place(r, i, cls, rank):
        other = int(logits[r, i].argsort(descending=True)[rank])
        a, b = float(logits[r, i, cls]), float(logits[r, i, other])
        logits[r, i, cls], logits[r, i, other] = b, a
    tokens = torch.full((rows, L), pad_id, dtype=torch.int64)
    scores = torch.full((rows,), NEG_INF)
    finished = torch.zeros(rows, dtype=torch.int64)
    lengths = torch.zeros(rows, dtype=torch.int64)
    for r in range(rows):
        b, w = divmod(r, W)
        e = {'no_eos': L, 'eos_at_0': 0}.get(kind, rnd(0, L + 1))      # where the refined reading ends (L: nowhere)
        for i in range(L):
            if i == e:
                place(r, i, eos_id, 0)
            elif i < e and int(logits[r, i].argmax()) == eos_id:
                place(r, i, eos_id, rnd(1, TOP))
        n = {'finished_early': rnd(0, L // 2 + 1), 'no_eos': L}.get(kind, rnd(0, L + 1))      # where the row's own <eos> stands (L: nowhere)
        n = min(n, L - 1) if kind == 'finished_early' else n
        if n < L:
            if n != e and int((logits[r, n] > logits[r, n, eos_id]).sum()) >= TOP:
                place(r, n, eos_id, rnd(1, TOP))
            tokens[r, n], finished[r], lengths[r] = eos_id, 1, n
        else:
            lengths[r] = L
        for i in range(min(n, L)):
            best = [c for c in logits[r, i].argsort(descending=True)[:TOP + 1].tolist() if c != eos_id]
            tokens[r, i] = best[rnd(0, TOP)]
        dead = (kind == 'dead_middle' and w % 3 == 1) or (kind == 'all_dead' and b == 0)
        scores[r] = NEG_INF if dead else -1.0 - 7.0 * torch.rand((), generator=g).item()
    if kind == 'identical':      # rows 0 and 1 of every image: the same logits and state, another AR score
        for b in range(B):
            r = b * W
            logits[r + 1], tokens[r + 1], finished[r + 1], lengths[r + 1] = logits[r], tokens[r], finished[r], lengths[r]
    if kind == 'tie':            # rows 0 and 1: 0 at one class, -200 elsewhere — every log-soft-max is 0 / -200 exactly; two different strings
        for b in range(B):
            for r in (b * W, b * W + 1):
                logits[r] = -200.0
                for i in range(L):
                    c = 1 + (7 * i + 3 * (r - b * W) + b) % (C - 1)
                    logits[r, i, c] = 0.0
                    tokens[r, i] = c
                finished[r], lengths[r] = 0, L
            assert tokens[b * W].tolist() != tokens[b * W + 1].tolist()
    return logits, tokens, scores, finished, lengths


def _rows(tokens, scores, finished, lengths):
    n = len(scores)
    sc = [float(s) for s in scores]
    words = [40 + r if f else -1 for r, f in enumerate(finished.tolist())]
    return RR.Rows(tokens.tolist(), sc, finished.tolist(), lengths.tolist(), [100 + r for r in range(n)], words, [float(torch.tensor(s, dtype=torch.float32)) for s in sc])


def _run_refine(logits, rows, mode, B, W, C, L, ldt, eos_id, pad_id, bos_id):
    """The rows in the device's layout (<bos>, token i at position i + 1, the last token in picked), through parseq_op_beam_refine."""
    nat, lib = native()
    n = B * W
    t = torch.tensor(rows.tokens, dtype=torch.int32)
    tok = torch.full((n, ldt), pad_id, dtype=torch.int32)
    tok[:, 0] = bos_id
    k = min(L, ldt - 1)
    tok[:, 1:1 + k] = t[:, :k]
    d = dict(tok=tok.to(DEV), picked=t[:, L - 1].contiguous().to(DEV), scores=torch.tensor(rows.scores, dtype=torch.float32, device=DEV),
             finished=torch.tensor(rows.finished, dtype=torch.uint8, device=DEV), lengths=torch.tensor(rows.lengths, dtype=torch.int32, device=DEV),
             nodes=torch.tensor(rows.nodes, dtype=torch.int32, device=DEV), words=torch.tensor(rows.words, dtype=torch.int32, device=DEV),
             ar=torch.tensor(rows.ar_scores, dtype=torch.float32, device=DEV))
    lg = logits.to(DEV, torch.float32).contiguous()
    need = lib.parseq_op_beam_refine_workspace_bytes(B, W, L)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    with nat.guard(lg):
        nat.check(lib.parseq_op_beam_refine(nat.ptr(lg), B, W, C, L, MODE_CODE[mode], nat.ptr(d['tok']), ldt, nat.ptr(d['scores']), nat.ptr(d['finished']),
                                            nat.ptr(d['lengths']), nat.ptr(d['picked']), nat.ptr(d['nodes']), nat.ptr(d['words']), nat.ptr(d['ar']),
                                            eos_id, pad_id, nat.ptr(ws), need, nat.stream_ptr(lg)))
    torch.cuda.synchronize()
    out = {key: v.cpu() for key, v in d.items()}
    out['tokens'] = torch.cat([out['tok'][:, 1:1 + k], out['picked'][:, None]], 1)[:, :L] if k < L else out['tok'][:, 1:1 + L]
    return out


def _compare(got, want, W, L, bos_id, pad_id):
    """Everything but the scores identical; the scores within the bound of their sum.  Returns the worst error as a share of its bound."""
    worst = 0.0
    for b, img in enumerate(want):
        sl = slice(b * W, (b + 1) * W)
        assert got['tokens'][sl].tolist() == img.tokens
        assert got['picked'][sl].tolist() == [t[L - 1] for t in img.tokens]
        assert (got['tok'][sl, 0] == bos_id).all()
        assert got['lengths'][sl].tolist() == img.lengths and got['finished'][sl].tolist() == img.finished
        assert got['nodes'][sl].tolist() == img.nodes and got['words'][sl].tolist() == img.words
        assert got['ar'][sl].tolist() == img.ar_scores
        for g, w, last in zip(got['scores'][sl].tolist(), img.scores, img.last):
            if w == NEG_INF:
                assert g == NEG_INF
            else:
                assert abs(w) < 128
                assert abs(g - w) <= score_bound(last), f'score error {abs(g - w):.3e} > {score_bound(last):.3e}'
                worst = max(worst, abs(g - w) / score_bound(last))
    return worst


def _margins_ok(want, L, kind):
    gaps = [x for img in want for x in img.gaps]
    ties = sum(x == 0.0 for x in gaps)
    if ties and kind not in ('identical', 'tie'):
        return False
    return all(x == 0.0 or x >= 2 * score_bound(L - 1) for x in gaps)


@pytest.mark.parametrize('W', [1, 3, 16])
@pytest.mark.parametrize('C', [37, 95, 201])
def test_selection_matches_the_restatement(C, W):
    eos_id, bos_id, pad_id = 0, C, C + 1
    worst, least = 0.0, math.inf
    for B in (1, 3):
        for L in (1, 7, 26, 32):      # 32 = the row pitch: the last token lives in picked
            for kind in KINDS:
                if W == 1 and kind in ('identical', 'tie'):
                    continue
                # the state is re-drawn (on the CPU, before anything runs) until, in both modes, every margin is a deliberate tie or safe
                for attempt in range(200):
                    logits, tokens, scores, finished, lengths = _state(kind, B, W, C, L, 1000 * attempt + 31 * C + 7 * W + 3 * L + B)
                    rows = _rows(tokens, scores, finished, lengths)
                    want = {mode: RR.refine_rows(logits, mode, rows, B, W, eos_id, pad_id) for mode in RR.MODES}
                    if all(_margins_ok(want[mode], L, kind) for mode in RR.MODES):
                        break
                assert all(_margins_ok(want[mode], L, kind) for mode in RR.MODES), (kind, B, L)
                if kind in ('identical', 'tie'):      # (in 'edit' a third row may beat both identical ones to their reading)
                    assert all(0.0 in img.gaps for mode in (RR.MODES if kind == 'tie' else ('score',)) for img in want[mode]), kind
                if kind == 'eos_at_0':      # every live row reads the empty string: one survives
                    assert all(sum(s > NEG_INF for s in img.scores) == 1 and img.lengths[0] == 0 for img in want['edit'])
                if kind == 'no_eos':
                    assert all(f == 0 for img in want['edit'] for f in img.finished)
                least = min([least] + [x for mode in RR.MODES for img in want[mode] for x in img.gaps if x > 0])
                for mode in RR.MODES:
                    got = _run_refine(logits, rows, mode, B, W, C, L, LDT, eos_id, pad_id, bos_id)
                    worst = max(worst, _compare(got, want[mode], W, L, bos_id, pad_id))
                    again = _run_refine(logits, rows, mode, B, W, C, L, LDT, eos_id, pad_id, bos_id)
                    for key in got:
                        a, b = (got[key].view(torch.int32), again[key].view(torch.int32)) if got[key].dtype == torch.float32 else (got[key], again[key])
                        assert torch.equal(a, b), f'{key}: two runs differ'
    print(f'[beam refine selection C={C} W={W}] worst score error {worst:.3f} of the bound, least non-zero margin {least:.2e}')


# -------------------------------------------------------------------------------------------------------------------
# 2 - 3. the refined search: arithmetic and decisions
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
def _searches(name, precision):
    """The plain search and the traced refined one ('edit', two iterations) per (model, precision); everything on the host."""
    cfg = CONFIGS[name]
    images = synth_images(SEARCH_B, cfg, seed=SEARCH_SEED[name])
    m = _model(name, precision)
    with torch.inference_mode():
        plain = m.model.beam_search(m.tokenizer, images.to(DEV), SEARCH_W, SEARCH_MAXLEN)
        res = m.model.beam_search(m.tokenizer, images.to(DEV), SEARCH_W, SEARCH_MAXLEN, trace=True, refine='edit', refine_iters=SEARCH_ITERS)
    torch.cuda.synchronize()
    host = lambda r: {k: v.cpu() for k, v in vars(r).items() if v is not None}
    return images, host(plain), host(res)


@functools.lru_cache(maxsize=None)
def _oracle_refined(name):
    """The same search and refinement by the oracle alone (CPU): the beam search of tests/beam_reference.py, then the restatement over the
    oracle's refinement pass."""
    import beam_reference as R
    cfg = CONFIGS[name]
    images = synth_images(SEARCH_B, cfg, seed=SEARCH_SEED[name])
    steps = SEARCH_MAXLEN + 1
    ar = R.beam_search(R.oracle_step_logits(_weights(name), cfg, images, SEARCH_W), SEARCH_B, SEARCH_W, steps, cfg.bos_id, cfg.eos_id, cfg.pad_id)
    rows = RR.rows_of_search(ar.tokens, ar.scores, ar.finished, ar.lengths)
    f = RR.oracle_refine_logits(_weights(name), cfg, images, SEARCH_W, steps)
    return rows, RR.refine_search(lambda it, tgt_in: f(tgt_in), 'edit', SEARCH_ITERS, rows, SEARCH_B, SEARCH_W, cfg.bos_id, cfg.eos_id, cfg.pad_id)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_refined_search_arithmetic(name, precision):
    """Every iteration's traced logits are the oracle's refinement logits (decode + head under the cloze and the key padding masks) for the
    traced decoder inputs and the memory of image row // W.  fp32 / bf16x3: 1e-3; bf16: the rounding-aware oracle, 3e-2."""
    cfg = CONFIGS[name]
    images, _, res = _searches(name, precision)
    rounding, tol = (None, 1e-3) if precision != 'bf16' else ('bf16', 3e-2)
    steps, rows = SEARCH_MAXLEN + 1, SEARCH_B * SEARCH_W
    f = RR.oracle_refine_logits(_weights(name), cfg, images, SEARCH_W, steps, rounding)
    assert res['trace_refine_logits'].shape == (SEARCH_ITERS, rows, steps, cfg.num_tokens - 2)
    assert res['trace_refine_tokens_in'].shape == (SEARCH_ITERS, rows, steps)
    worst = 0.0
    for it in range(SEARCH_ITERS):
        tgt_in = res['trace_refine_tokens_in'][it].long()
        assert (tgt_in[:, 0] == cfg.bos_id).all() and (tgt_in >= 0).all() and (tgt_in < cfg.num_tokens).all()
        worst = max(worst, (res['trace_refine_logits'][it] - f(tgt_in)).abs().max().item())
    print(f'[beam refine arithmetic {name} {precision}] worst |dlogit| over {SEARCH_ITERS} iterations {worst:.3e} (bar {tol:.0e})')
    assert worst <= tol


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_refined_search_decisions(name, precision):
    """The restatement replayed from the traced logits reproduces every iteration: the readings and their order (the next iteration's decoder
    inputs, the final tokens), lengths, flags, ar_scores, and the scores within the bound.  An image drops out from the iteration at which a
    margin lies in (0, twice the bound); at most 2 % of the (image, iteration) pairs may (here: none)."""
    cfg = CONFIGS[name]
    B, W, L = SEARCH_B, SEARCH_W, SEARCH_MAXLEN + 1
    limit = 2 * score_bound(L - 1)
    # the seeds, on the CPU with the oracle alone: no unsafe margin, and the refinement does something
    start, ora = _oracle_refined(name)
    assert all(x == 0.0 or x >= limit for st in ora for img in st.gaps for x in img), 'pick another seed'
    live = [r for r in range(B * W) if start.scores[r] > NEG_INF]
    first = ora[0]
    moved = sum(1 for b in range(B) for r in range(W)
                if start.scores[b * W + first.src[b][r]] > NEG_INF
                and (first.scores[b * W + r] == NEG_INF or first.tokens[b * W + r] != start.tokens[b * W + first.src[b][r]]))
    assert moved >= len(live) / 4, (moved, len(live))

    _, plain, res = _searches(name, precision)
    rows = RR.rows_of_search(plain['tokens'], plain['scores'], plain['finished'], plain['lengths'])
    rep = RR.refine_search(lambda it, tgt_in: res['trace_refine_logits'][it], 'edit', SEARCH_ITERS, rows, B, W, cfg.bos_id, cfg.eos_id, cfg.pad_id)
    valid = torch.ones(B, dtype=torch.bool)
    skipped = 0
    alive = (plain['scores'] > NEG_INF).view(B, W)
    got_in = res['trace_refine_tokens_in'].long().view(SEARCH_ITERS, B, W, L)
    assert torch.equal(got_in[0][alive], RR.tgt_in_of(rows.tokens, cfg.bos_id).view(B, W, L)[alive])      # a dead row's history is whatever the search left
    for it in range(SEARCH_ITERS):
        for b in range(B):
            if valid[b] and any(0.0 < x < limit for x in rep[it].gaps[b]):
                valid[b] = False
                skipped += 1
        if it + 1 < SEARCH_ITERS:
            assert torch.equal(got_in[it + 1][valid], RR.tgt_in_of(rep[it].tokens, cfg.bos_id).view(B, W, L)[valid]), f'readings after iteration {it}'
    assert skipped <= 0.02 * B * SEARCH_ITERS
    last = rep[-1]
    assert torch.equal(res['tokens'].long()[valid], torch.tensor(last.tokens).view(B, W, L)[valid])
    assert torch.equal(res['lengths'].long()[valid], torch.tensor(last.lengths).view(B, W)[valid])
    assert torch.equal(res['finished'].long()[valid], torch.tensor(last.finished).view(B, W)[valid])
    want_ar = torch.tensor(last.ar_scores, dtype=torch.float64).view(B, W)
    assert torch.equal(res['ar_scores'].double()[valid], want_ar[valid])      # the search's own fp32 scores, bit for bit
    worst = 0.0
    for b in range(B):
        for r in range(W):
            if not valid[b]:
                continue
            g, w = res['scores'][b, r].item(), last.scores[b * W + r]
            if w == NEG_INF:
                assert g == NEG_INF
            else:
                bound = score_bound(last.last[b * W + r])
                assert abs(g - w) <= bound, f'score error {abs(g - w):.3e} > {bound:.3e}'
                worst = max(worst, abs(g - w) / bound)
    margins = [x for st in rep for img in st.gaps for x in img if x > 0]
    print(f'[beam refine decisions {name} {precision}] skipped {skipped} of {B * SEARCH_ITERS}, worst score error {worst:.3f} of the bound, '
          f'least non-zero margin {min(margins):.2e}, exact ties {sum(x == 0 for st in rep for img in st.gaps for x in img)}')


# -------------------------------------------------------------------------------------------------------------------
# 4. W = 1 against forward
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('iters', [1, 2])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_width_one_is_forward_with_refinement(name, precision, iters, golden):
    """W = 1, 'edit', k iterations: the tokens are the arg-max reading of `forward` (AR + k refinements) cut at <eos>, the score the sum of
    that reading's log-max-probabilities."""
    cfg = CONFIGS[name]
    g, _ = golden(name)
    x = g['images'].to(DEV)
    fwd = make_model(name, precision, decode_ar=True, refine_iters=iters)
    beam = make_model(name, precision, decode_ar=True, refine_iters=0)
    with torch.inference_mode():
        logits = fwd(x).cpu()
        res = beam.beam_search(x, 1, refine='edit', refine_iters=iters)
    B, L, _ = logits.shape
    assert res.tokens.shape == (B, 1, L)
    logp, ids = torch.log_softmax(logits.double(), -1).max(-1)
    worst = 0.0
    for b in range(B):
        picks = ids[b].tolist()
        n = picks.index(cfg.eos_id) if cfg.eos_id in picks else L
        last = n if n < L else L - 1
        want = [picks[i] if i <= last else cfg.pad_id for i in range(L)]
        assert res.tokens[b, 0].tolist() == want, b
        assert res.lengths[b, 0].item() == n and res.finished[b, 0].item() == int(n < L)
        err = abs(res.scores[b, 0].item() - logp[b, :last + 1].sum().item())
        worst = max(worst, err / score_bound(last))
        assert err <= score_bound(last), f'image {b}: score error {err:.3e} > {score_bound(last):.3e}'
    print(f'[beam refine W=1 {name} {precision} x{iters}] worst score error {worst:.3f} of the bound')


# -------------------------------------------------------------------------------------------------------------------
# 5. 'score'
# -------------------------------------------------------------------------------------------------------------------
def _pll(f, cfg, tokens, finished, lengths):
    """The oracle's teacher-forced pseudo-log-likelihood of hypotheses [n, L] (float64)."""
    tokens = torch.as_tensor(tokens).long()
    L = tokens.shape[1]
    logp = torch.log_softmax(f(RR.tgt_in_of(tokens, cfg.bos_id)).double(), -1)
    out = []
    for r in range(tokens.shape[0]):
        last = int(lengths[r]) if int(finished[r]) else L - 1
        out.append(sum(logp[r, i, int(tokens[r, i])].item() for i in range(last + 1)))
    return out


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_score_mode_rescoring(name, precision):
    cfg = CONFIGS[name]
    B, W, L = SEARCH_B, SEARCH_W, SEARCH_MAXLEN + 1
    images, plain, _ = _searches(name, precision)
    m = _model(name, precision)
    with torch.inference_mode():
        res = m.beam_search(images.to(DEV), W, SEARCH_MAXLEN, refine='score')
    assert res.trace_refine_logits is None and res.ar_scores.shape == (B, W)
    tok, sc, ar, ln, fi = res.tokens.cpu(), res.scores.cpu(), res.ar_scores.cpu(), res.lengths.cpu(), res.finished.cpu()
    assert (plain['scores'] > NEG_INF).all()      # W = 3 of 95 classes: no dead beam, every row is compared
    f = RR.oracle_refine_logits(_weights(name), cfg, images, W, L)
    want = torch.tensor(_pll(f, cfg, tok.view(B * W, L), fi.view(-1), ln.view(-1)), dtype=torch.float64).view(B, W)
    for b in range(B):
        key = lambda t, n, fl: [(tuple(t[w].tolist()), int(n[w]), int(fl[w])) for w in range(W)]
        mine, theirs = key(tok[b], ln[b], fi[b]), key(plain['tokens'][b], plain['lengths'][b], plain['finished'][b])
        assert sorted(mine) == sorted(theirs) and len(set(mine)) == W
        for w in range(W):      # the search's own score follows its hypothesis, bit for bit
            assert ar[b, w].view(torch.int32) == plain['scores'][b, theirs.index(mine[w])].view(torch.int32)
        assert all(x >= y for x, y in zip(sc[b].tolist(), sc[b].tolist()[1:]))
    worst = (sc.double() - want).abs().max().item()
    print(f'[beam refine score {name} {precision}] worst |dscore| against the oracle {worst:.3e} (bar {WHOLE_SCORE_BAR:.0e})')
    assert worst <= WHOLE_SCORE_BAR


EXH_B, EXH_W, EXH_MAXLEN, EXH_SEED = 8, 4, 5, 301      # the per-image four-word lexicons of tests/test_lexicon_beam.py


def _random_words(n, seed, longest):
    import random
    rng = random.Random(seed)
    return [''.join(rng.choice(CHARSET_94_FULL) for _ in range(rng.randint(1, longest))) for _ in range(n)]


@functools.lru_cache(maxsize=None)
def _lexicon_lists():
    lists = []
    for b in range(EXH_B):
        words = []
        for w in _random_words(12, 50 + b, EXH_MAXLEN):
            if w not in words and len(words) < EXH_W:
                words.append(w)
        assert len(words) == EXH_W
        lists.append(words)
    return lists


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_score_mode_under_a_lexicon(name, precision):
    """Per-image lexicons of four words: the constrained search is exhaustive, so every image returns its four words; rescored, the words
    still follow their rows, the scores are the oracle's pseudo-log-likelihoods and the order is the oracle's wherever its gaps exceed the bar."""
    cfg = CONFIGS[name]
    L = EXH_MAXLEN + 1
    images = synth_images(EXH_B, cfg, seed=EXH_SEED)
    lists = _lexicon_lists()
    lex, roots = Lexicon.forest(lists, TOK)
    m = _model(name, precision)
    with torch.inference_mode():
        plain = m.beam_search(images.to(DEV), EXH_W, EXH_MAXLEN, lexicon=lex.to(DEV), roots=roots)
        res = m.beam_search(images.to(DEV), EXH_W, EXH_MAXLEN, lexicon=lex.to(DEV), roots=roots, refine='score')
        beams = m.tokenizer.decode_beams(res, lex)
        chars = m.tokenizer.decode_beams(res)
    assert res.finished.cpu().tolist() == [[1] * EXH_W] * EXH_B
    words, sc = res.words.cpu().tolist(), res.scores.cpu().double()
    f = RR.oracle_refine_logits(_weights(name), cfg, images, EXH_W, L)
    want = torch.tensor(_pll(f, cfg, res.tokens.cpu().view(-1, L), res.finished.cpu().view(-1), res.lengths.cpu().view(-1)), dtype=torch.float64).view(EXH_B, EXH_W)
    compared = 0
    for b in range(EXH_B):
        assert sorted(words[b]) == list(range(b * EXH_W, (b + 1) * EXH_W))
        assert [lex.words[k] for k in words[b]] == [s for s, _ in beams[b]] == [s for s, _ in chars[b]]
        assert sorted(s for s, _ in beams[b]) == sorted(lists[b])
        pw = plain.words[b].cpu().tolist()
        for r, k in enumerate(words[b]):      # the search's own score of the same word
            assert res.ar_scores[b, r].cpu().view(torch.int32) == plain.scores[b, pw.index(k)].cpu().view(torch.int32)
        assert all(x >= y for x, y in zip(sc[b].tolist(), sc[b].tolist()[1:]))
        ranked = sorted(want[b].tolist(), reverse=True)
        if min(x - y for x, y in zip(ranked, ranked[1:])) > 2 * WHOLE_SCORE_BAR:
            assert want[b].tolist() == ranked      # want is in the device's row order: it is the oracle's order too
            compared += 1
    worst = (sc - want).abs().max().item()
    print(f'[beam refine score lexicon {name} {precision}] worst |dscore| {worst:.3e} (bar {WHOLE_SCORE_BAR:.0e}), order compared on {compared} of {EXH_B} images')
    assert worst <= WHOLE_SCORE_BAR and compared >= EXH_B // 2


# -------------------------------------------------------------------------------------------------------------------
# 6. no change without the flag
# -------------------------------------------------------------------------------------------------------------------
def test_plain_searches_are_what_they_were():
    from parseq_amd.model import BeamResult, LexiconBeamResult
    m = _model('parseq', 'bf16x3')
    x = synth_images(5, CONFIGS['parseq'], seed=11).to(DEV)
    lex = Lexicon(_random_words(30, 7, 5), TOK).to(DEV)
    with torch.inference_mode():
        a, al = m.beam_search(x, 3, 6), m.beam_search(x, 3, 6, lexicon=lex)
        fwd = m(x, 25).clone()
        e = m.beam_search(x, 3, 6, refine='edit', refine_iters=2)
        s = m.beam_search(x, 3, 6, lexicon=lex, refine='score')
        b, bl = m.beam_search(x, 3, 6), m.beam_search(x, 3, 6, lexicon=lex)
        c = m.beam_search(x, 3, 6, refine=None, refine_iters=1)
        fwd2 = m(x, 25).clone()
    torch.cuda.synchronize()
    assert type(a) is type(b) is type(c) is type(e) is BeamResult and type(al) is type(bl) is type(s) is LexiconBeamResult
    assert a.ar_scores is None and b.ar_scores is None and bl.ar_scores is None and b.trace_refine_logits is None
    assert e.ar_scores.shape == (5, 3) and s.ar_scores.shape == (5, 3) and s.words.shape == (5, 3) and e.trace_refine_logits is None
    for x0, x1 in ((a, b), (a, c), (al, bl)):
        assert torch.equal(x0.tokens, x1.tokens) and torch.equal(x0.scores.view(torch.int32), x1.scores.view(torch.int32))
        assert torch.equal(x0.lengths, x1.lengths) and torch.equal(x0.finished, x1.finished)
    assert torch.equal(al.words, bl.words) and torch.equal(fwd, fwd2)
    # a second refined call reproduces every bit
    with torch.inference_mode():
        e2 = m.beam_search(x, 3, 6, refine='edit', refine_iters=2)
    for k in ('tokens', 'lengths', 'finished'):
        assert torch.equal(getattr(e, k), getattr(e2, k))
    assert torch.equal(e.scores.view(torch.int32), e2.scores.view(torch.int32)) and torch.equal(e.ar_scores.view(torch.int32), e2.ar_scores.view(torch.int32))
    alts = m.tokenizer.decode_beams(e)
    assert len(alts) == 5 and all(1 <= len(v) <= 3 and all(x[1] >= y[1] for x, y in zip(v, v[1:])) for v in alts)


# -------------------------------------------------------------------------------------------------------------------
# 7. refusals
# -------------------------------------------------------------------------------------------------------------------
def test_library_refusals():
    nat, lib = native()
    name = 'parseq-tiny'
    cfg = CONFIGS[name]
    m = _model(name, 'bf16x3')
    x = synth_images(4, cfg, seed=3).to(DEV)
    B, W, steps = 4, 2, 4
    plan = m.model._plan(B * W)
    table = Lexicon(_random_words(30, 7, 3), TOK).table(DEV)

    def call(mode, iters, tb=None, short=0, width=W, ar_ok=True, misalign=0, nodes=None, num_steps=steps, images_ok=True):
        rows = B * max(width, 1)
        outs = [torch.full((rows * steps,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), -7.0, dtype=torch.float32, device=DEV),
                torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), 7, dtype=torch.uint8, device=DEV),
                torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), -7.0, dtype=torch.float32, device=DEV)]
        need = lib.parseq_beam_refine_workspace_bytes(plan, B, width, num_steps, int(tb is not None))
        ws = torch.empty(max(need, 1 << 20) + 64, dtype=torch.uint8, device=DEV)
        status = lib.parseq_forward_beam_refine(plan, nat.ptr(x) if images_ok else None, nat.dtype_code(x.dtype), B, width, num_steps, nat.ptr(outs[0]),
                                                nat.ptr(outs[1]), nat.ptr(outs[2]), nat.ptr(outs[3]), None, ws.data_ptr() + misalign,
                                                (need - short) if short else ws.numel() - 64, nat.stream_ptr(x), nat.ptr(tb) if tb is not None else None,
                                                (tb.shape[0] if nodes is None else nodes) if tb is not None else 0, None, nat.ptr(outs[4]),
                                                mode, iters, nat.ptr(outs[5]) if ar_ok else None, None)
        torch.cuda.synchronize()
        untouched = bool((outs[0] == -7).all() and (outs[1] == -7.0).all() and (outs[2] == -7).all() and (outs[3] == 7).all() and (outs[4] == -7).all()
                         and (outs[5] == -7.0).all())
        return status, untouched, need

    SCORE, EDIT = MODE_CODE['score'], MODE_CODE['edit']
    plain, plain_lex = lib.parseq_beam_workspace_bytes(plan, B, W, steps), lib.parseq_beam_lexicon_workspace_bytes(plan, B, W, steps)
    for mode, iters, tb in ((EDIT, 1, None), (EDIT, 3, None), (SCORE, 1, None), (SCORE, 1, table)):
        status, untouched, need = call(mode, iters, tb)
        assert status == 0 and not untouched
    C_ = cfg.num_tokens - 2
    pad = lambda n: (n + 255) // 256 * 256
    extra = pad(B * W * steps * C_ * 4) + 3 * pad(B * W * steps * 4) + pad(B * W * 4)      # logits, three statistics arrays, ar_score
    assert lib.parseq_beam_refine_workspace_bytes(plan, B, W, steps, 0) == plain + extra and plain % 256 == 0
    assert lib.parseq_beam_refine_workspace_bytes(plan, B, W, steps, 1) == plain_lex + extra
    for mode in (0, 3, -1):
        assert call(mode, 1)[:2] == (-1, True) and b'refine_mode' in lib.parseq_last_error()
    assert call(EDIT, 1, table)[:2] == (-1, True) and b'lexicon' in lib.parseq_last_error()
    assert call(SCORE, 2)[:2] == (-1, True) and b'score mode' in lib.parseq_last_error()
    for iters in (0, -1):
        assert call(EDIT, iters)[:2] == (-1, True) and b'refine_iters' in lib.parseq_last_error()
        assert call(SCORE, iters)[:2] == (-1, True)
    assert call(EDIT, 1, short=1)[:2] == (-1, True) and b'workspace' in lib.parseq_last_error()
    assert call(SCORE, 1, table, short=1)[:2] == (-1, True)
    assert call(EDIT, 1, misalign=4)[:2] == (-1, True) and b'aligned' in lib.parseq_last_error()
    assert call(EDIT, 1, ar_ok=False)[:2] == (-1, True) and b'ar_scores_out' in lib.parseq_last_error()
    # what the plain and the constrained search refuse
    assert call(EDIT, 1, width=17)[:2] == (-1, True) and lib.parseq_beam_refine_workspace_bytes(plan, B, 17, steps, 0) == 0
    assert call(EDIT, 1, width=0)[:2] == (-1, True)
    assert call(EDIT, 1, num_steps=0)[:2] == (-1, True) and call(EDIT, 1, num_steps=cfg.max_label_length + 2)[:2] == (-1, True)
    assert call(EDIT, 1, images_ok=False)[:2] == (-1, True)
    assert call(SCORE, 1, table, nodes=0)[:2] == (-1, True) and b'trie_nodes' in lib.parseq_last_error()
    from parseq_amd import create_model
    deep = create_model(name, dec_depth=2, precision='bf16x3').eval().to(DEV)
    with pytest.raises(ValueError, match='dec_depth'):
        deep.beam_search(x, 2, refine='edit')
    assert lib.parseq_beam_refine_workspace_bytes(deep.model._plan(8), 4, 2, 4, 0) == 0 and b'dec_depth' in lib.parseq_last_error()
    vit = create_model('vitstr', precision='bf16').eval().to(DEV)
    with pytest.raises(ValueError, match='ViTSTR'):
        vit.beam_search(torch.zeros(2, 3, *vit.hparams.img_size, device=DEV), 2, refine='score')
    # the operator hook
    z = torch.zeros(W * 4 * 95, device=DEV)
    i32 = torch.zeros(W * LDT, dtype=torch.int32, device=DEV)
    u8 = torch.zeros(W, dtype=torch.uint8, device=DEV)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    sc, ar = torch.zeros(W, device=DEV), torch.zeros(W, device=DEV)
    ln, pk = torch.zeros(W, dtype=torch.int32, device=DEV), torch.zeros(W, dtype=torch.int32, device=DEV)

    def hook(W_=W, C_=95, L=4, mode=EDIT, ldt=LDT, nbytes=1 << 16, eos=0):
        return lib.parseq_op_beam_refine(nat.ptr(z), 1, W_, C_, L, mode, nat.ptr(i32), ldt, nat.ptr(sc), nat.ptr(u8), nat.ptr(ln), nat.ptr(pk), None, None,
                                         nat.ptr(ar), eos, 96, nat.ptr(ws), nbytes, nat.stream_ptr(z))
    assert hook() == 0
    assert hook(W_=17) == -1 and hook(W_=0) == -1 and hook(L=0) == -1 and hook(L=65) == -1 and hook(L=5, ldt=4) == -1 and hook(ldt=65) == -1
    assert hook(mode=0) == -1 and hook(eos=95) == -1 and hook(nbytes=lib.parseq_op_beam_refine_workspace_bytes(1, W, 4) - 1) == -1
    assert lib.parseq_op_beam_refine_workspace_bytes(1, 17, 4) == 0
    torch.cuda.synchronize()


# -------------------------------------------------------------------------------------------------------------------
# 8. read.py
# -------------------------------------------------------------------------------------------------------------------
def test_read_cli_refined_nbest(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip('PIL.Image')
    import read as read_cli
    from oracle.make_resize_golden import make_input
    files = []
    for i, (h, w) in enumerate([(40, 150), (32, 128), (64, 200)]):
        f = tmp_path / f'crop{i}.png'
        Image.fromarray(make_input(h, w, 1 - i % 2), 'RGB').save(f)
        files.append(str(f))
    # Which reading comes first is decided by the refined scores, so the statement needs a model that is sure of its greedy reading, as a
    # trained one is; the synthetic weights are not (measured: the empty reading at -2.69 before the refined greedy one at -8.09).  The head
    # is therefore scaled by 4096: the arg-max of every position stays what it was, every log-max-probability becomes exactly 0 in fp32, the
    # greedy path is beam 0 at score 0, every refined reading scores 0 at most, and equal scores keep the lower row first.
    from parseq_amd import create_model
    sd = dict(synth_state_dict(CONFIGS['parseq'], 0))
    sd['head.weight'], sd['head.bias'] = sd['head.weight'] * 4096.0, sd['head.bias'] * 4096.0
    m = create_model('parseq', decode_ar=True, refine_iters=1, precision='bf16x3')
    m.model.load_state_dict(sd)
    m = m.eval().to(DEV)
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV])
    plain = capsys.readouterr().out.splitlines()
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--nbest', '3'])
    nbest = capsys.readouterr().out.splitlines()
    assert plain[1:] == [f'{f}: {label}' for f, label, _ in read_cli.read_files(m, files, DEV)]
    assert [line for line in nbest if not line.startswith('    ')] == plain      # without the new flag: what it printed
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--nbest', '3', '--refine-beams', 'edit'])
    out = capsys.readouterr().out.splitlines()[1:]
    with torch.inference_mode():
        best = read_cli.read_files_nbest(m, files, 3, None, DEV, 'edit', 1)
    k = 0
    for f, alts in best:
        assert out[k] == plain[1 + files.index(f)] and 1 <= len(alts) <= 3
        block = out[k + 1:k + 1 + len(alts)]
        assert block == [f'    {lp:9.4f}  {label}' for label, lp in alts]
        # the first alternative is the reading forward prints with refine_iters = 1
        print(f'[beam refine read.py] {out[k]!r}: alternatives {alts}')
        assert alts[0][1] == 0.0
        assert out[k] == f'{f}: {alts[0][0]}'
        k += 1 + len(alts)
    assert k == len(out)
    capsys.readouterr()      # (the lines printed above)
    read_cli.main(['pretrained=parseq', '--images', files[0], '--device', DEV, '--nbest', '2', '--beam', '4', '--refine-beams', 'score'])
    assert len(capsys.readouterr().out.splitlines()[1:]) == 3
