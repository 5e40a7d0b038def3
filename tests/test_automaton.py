"""GPU tests of the beam search over a weighted automaton: the weighted selection kernel alone against the CPU
restatement (tests/automaton_reference.py), the two bit-equalities of the definition (no prior: the lexicon search; a free one-state
automaton: the plain search) on the step and on the whole call, the whole search's decisions against a replay of the restatement from the
traced logits, the exhaustive property against the oracle with priors, patterns end to end, per-crop roots, the refusals and read.py.

The score bounds are section 18's, since the same arithmetic produces the model's scores: 4e-5 * (step + 1) for a step's scores against the
float64 restatement on the same logits, 8e-3 for a whole search's scores against the CPU oracle.  What the weights add to wsum and f:

    wsum' = fl(wsum + weight)                          one rounding, at most 2^-24 |wsum'|
    p     = fl(alpha wsum')                            one rounding, at most 2^-24 |alpha wsum'|
    q     = fl(p + fl(beta k))                         one rounding of the sum, at most 2^-24 |p + beta k|  (beta k is exact for the betas here)
    f     = fl(m + q)                                  one rounding, at most 2^-24 |f|

so with M the largest |f|, |wsum| or |alpha wsum| of the restated case, f and wsum are within 4 * 2^-24 * M of the restatement on top of the
score's own bound, and over the steps of a search, in which wsum is carried in fp32, within (step + 1) times that (`weight_bound`)."""
import functools
import random
import re

import pytest
import torch

import automaton_reference as AR
import beam_reference as R
import test_lexicon_beam as TL          # its synthetic weights, models, word lists and oracle sums, computed once for both files
from gpu_util import DEV, native
from oracle.synth import CONFIGS, synth_images
from parseq_amd.automaton import Automaton
from parseq_amd.tokenizer import Tokenizer

pytestmark = pytest.mark.gpu

NEG_INF = float('-inf')
LDT = TL.LDT
TOK = TL.TOK
WHOLE_SCORE_BAR = TL.WHOLE_SCORE_BAR
score_bound = TL.score_bound
ALPHAS, BETAS = (0.0, 0.5, 1.0), (0.0, 0.75)


def weight_bound(step, big):
    return score_bound(step) + 4 * 2.0 ** -24 * big * (step + 1)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# -------------------------------------------------------------------------------------------------------------------
# 1. the step kernel alone
# -------------------------------------------------------------------------------------------------------------------
def _run_step(st, B, W, C, eos_id, pad_id, alpha, beta, table=None, weight=None):
    nat, lib = native()
    d = dict(tok=st['tok'].to(DEV, torch.int32).contiguous(), scores=st['scores'].to(DEV, torch.float32).contiguous(),
             finished=st['finished'].to(DEV, torch.uint8).contiguous(), lengths=st['lengths'].to(DEV, torch.int32).contiguous(),
             parent=torch.full((B * W,), -7, dtype=torch.int32, device=DEV), picked=torch.full((B * W,), -7, dtype=torch.int32, device=DEV),
             nodes=st['nodes'].to(DEV, torch.int32).contiguous(), words=st['words'].to(DEV, torch.int32).contiguous(),
             wsums=st['wsums'].to(DEV, torch.float32).contiguous(), fused=torch.full((B * W,), -7.0, dtype=torch.float32, device=DEV))
    lg = st['logits'].to(DEV, torch.float32).contiguous()
    tb = (st['table'] if table is None else table).to(DEV, torch.int32).contiguous()
    wt = (st['weight'] if weight is None else weight).to(DEV, torch.float32).contiguous()
    assert wt.shape == tb.shape
    with nat.guard(lg):
        nat.check(lib.parseq_op_beam_step_automaton(nat.ptr(lg), B, W, C, st['step'], nat.ptr(d['tok']), LDT, nat.ptr(d['scores']), nat.ptr(d['finished']),
                                                    nat.ptr(d['lengths']), nat.ptr(d['parent']), nat.ptr(d['picked']), eos_id, pad_id, nat.stream_ptr(lg),
                                                    nat.ptr(tb), nat.ptr(wt), tb.shape[0], nat.ptr(d['nodes']), nat.ptr(d['words']), alpha, beta,
                                                    nat.ptr(d['wsums']), nat.ptr(d['fused'])))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def _image_args(st, b, W):
    rows = slice(b * W, (b + 1) * W)
    return (st['logits'][rows], [float(s) for s in st['scores'][rows]], [float(s) for s in st['wsums'][rows]], st['finished'][rows].tolist(),
            st['lengths'][rows].tolist(), st['tok'][rows].tolist(), st['nodes'][rows].tolist(), st['words'][rows].tolist())


def _reference_step(st, B, W, eos_id, pad_id, alpha, beta):
    table, weight = st['table'].tolist(), st['weight'].double().tolist()
    return [AR.step_image(*_image_args(st, b, W), table, weight, st['step'], eos_id, pad_id, alpha, beta) for b in range(B)]


def _compare_step(got, want, W, step, alpha):
    """Everything integral equal; score within the step bound; wsum and f within `weight_bound`.  Returns the worst errors over their bounds."""
    worst_s = worst_w = 0.0
    for b, st in enumerate(want):
        rows = slice(b * W, (b + 1) * W)
        assert got['parent'][rows].tolist() == st.parent
        assert got['picked'][rows].tolist() == st.picked
        assert got['tok'][rows].tolist() == st.hist
        assert got['finished'][rows].tolist() == st.finished
        assert got['lengths'][rows].tolist() == st.lengths
        assert got['nodes'][rows].tolist() == st.nodes
        assert got['words'][rows].tolist() == st.words
        live = [r for r in range(W) if st.parent[r] >= 0]
        big = max([abs(v) for r in live for v in (st.fused[r], st.wsums[r], alpha * st.wsums[r])], default=0.0)
        for r in range(W):
            g_s, g_w, g_f = (got[k][rows].tolist()[r] for k in ('scores', 'wsums', 'fused'))
            if st.parent[r] < 0:
                assert g_s == NEG_INF and g_f == NEG_INF and g_w == 0.0
                continue
            worst_s = max(worst_s, abs(g_s - st.scores[r]) / score_bound(step))
            worst_w = max(worst_w, abs(g_w - st.wsums[r]) / weight_bound(step, big), abs(g_f - st.fused[r]) / weight_bound(step, big))
    assert worst_s <= 1.0, f'score error {worst_s:.3f} of the bound'
    assert worst_w <= 1.0, f'wsum / f error {worst_w:.3f} of the bound'
    return worst_s, worst_w


KINDS = ('start', 'middle', 'only_eos', 'tie', 'heavy', 'nonfinite', 'bad_child', 'bad_root', 'cycle')


def _quarters(g, shape, lo, hi):
    """Multiples of 0.25 in [lo, hi]: exactly representable, as are their sums and their products with the alphas of the test."""
    return torch.randint(int(lo * 4), int(hi * 4) + 1, shape, generator=g).float() / 4


def _state(kind, B, W, C, seed, eos_id, pad_id, bos_id, alpha, beta):
    """test_lexicon_beam's inputs of one constrained step with a weight on every entry of the table (multiples of 0.25 in [-4, 0], also where
    the table has no arc: the table decides) and a weight sum per live beam, then what the kind asks for."""
    st = TL._state({'heavy': 'middle', 'nonfinite': 'middle', 'cycle': 'middle'}.get(kind, kind), B, W, C, seed, eos_id, pad_id, bos_id)
    lex, roots, lists = TL._step_forest(C, B)
    g = torch.Generator().manual_seed(seed + 1)
    table = st['table']
    st['weight'] = _quarters(g, tuple(table.shape), -4, 0)
    alive = st['scores'] > NEG_INF
    st['wsums'] = torch.where(alive, _quarters(g, (B * W,), -6, 0), torch.zeros(B * W)) if st['step'] > 0 else torch.zeros(B * W)
    step = st['step']
    if kind == 'tie' and W > 1:
        # beams 0 and 1 of every image finished at the same length with (score, wsum) = (-0.5, -2) and (-0.5 - alpha, -1): different in both
        # (in wsum alone at alpha = 0) and, every value being a multiple of 0.125, exactly equal in f — the image's best two
        for b in range(B):
            for w, (s, ws) in enumerate(((-0.5, -2.0), (-0.5 - alpha, -1.0))):
                r = b * W + w
                st['scores'][r], st['wsums'][r], st['finished'][r], st['lengths'][r] = s, ws, 1, 2
                st['tok'][r, 1:] = pad_id
                st['tok'][r, 1:4] = torch.tensor([3, 4, eos_id])
                st['nodes'][r] = TL._walk(table, roots[b], lists[b][14])
                st['words'][r] = int(table[st['nodes'][r], eos_id])
            for r in range(b * W + 2, (b + 1) * W):      # (the others well below: a character bonus of 0.75 * 4 does not lift them past the pair)
                if st['scores'][r] > NEG_INF:
                    st['scores'][r] -= 12.0
    if kind == 'cycle':
        # every live unfinished beam's state loops to itself along the three characters its row likes best (at weight -0.25, so that some
        # loop is taken) and along classes 1 .. 5, and shares a successor (the root) along the next three
        for r in range(B * W):
            n = int(st['nodes'][r])
            if n >= 0 and not st['finished'][r] and alive[r]:
                table[n, 1:6] = n
                table[n, 6:9] = roots[r // W]
                for c in [int(c) for c in st['logits'][r].topk(4).indices if c != eos_id][:3]:
                    table[n, c] = n
                    st['weight'][n, c] = -0.25
    if kind == 'nonfinite':
        # of every live beam's arcs, <eos> included: the first -inf, the second +inf, the third NaN, the fourth kept, and so on
        for r in range(B * W):
            n = int(st['nodes'][r])
            if n >= 0 and not st['finished'][r]:
                arcs = [c for c in range(C) if table[n, c] >= 0]
                for k, c in enumerate(arcs):
                    if k % 4 < 3:
                        st['weight'][n, c] = (NEG_INF, float('inf'), float('nan'))[k % 4]
    if kind == 'heavy' and alpha > 0:
        # the arc of every image's best fresh candidate gets a weight that throws it out of the best W (every live beam's state first gets
        # arcs along classes 1 .. 8 where it has none, so that more than W candidates exist)
        for r in range(B * W):
            n = int(st['nodes'][r])
            if n >= 0 and not st['finished'][r] and alive[r]:
                table[n, 1:9] = torch.where(table[n, 1:9] < 0, roots[r // W], table[n, 1:9])
        tb, wt = table.tolist(), st['weight'].double().tolist()
        st['heavy'] = []
        for b in range(B):
            cands = AR.rank_candidates(*_image_args(st, b, W)[:5], st['nodes'][b * W:(b + 1) * W].tolist(), tb, wt, step, eos_id, alpha, beta)
            best = next((c for c in cands if c[2] >= 0), None)
            if best is not None:
                node = int(st['nodes'][b * W + best[1]])
                st['weight'][node, best[2]] = -4096.0
                st['heavy'].append((b, best[1], best[2], len(cands)))
    return st


def _gaps(st, B, W, eos_id, alpha, beta, kind):
    """Every adjacent-rank gap in f among the best W + 1 candidates is >= 1e-3 — or, between the carries of beams 0 and 1 of 'tie' (the
    constructed pair, and no other), exactly 0."""
    table, weight = st['table'].tolist(), st['weight'].double().tolist()
    for b in range(B):
        args = _image_args(st, b, W)
        top = AR.rank_candidates(*args[:5], args[6], table, weight, st['step'], eos_id, alpha, beta)[:W + 1]
        for a, c in zip(top, top[1:]):
            d = a[0] - c[0]
            if not (d >= 1e-3 or (kind == 'tie' and d == 0.0 and a[1:3] == (0, -1) and c[1:3] == (1, -1))):
                return False
    return True


@pytest.mark.parametrize('W', [1, 3, 16])
@pytest.mark.parametrize('C', [37, 95, 201])
def test_step_kernel_matches_the_restatement(C, W):
    eos_id, bos_id, pad_id = 0, C, C + 1
    worst = [0.0, 0.0]
    dead_slots = ties = dropped = blocked = loops = 0
    for B in (1, 3):
        for kind in KINDS:
            for alpha in ALPHAS:
                for beta in BETAS:
                    # inputs are re-drawn (on the CPU, before anything runs) until the gaps are as _gaps wants them
                    for attempt in range(200):
                        st = _state(kind, B, W, C, 1000 * attempt + 17 * C + W + B, eos_id, pad_id, bos_id, alpha, beta)
                        if _gaps(st, B, W, eos_id, alpha, beta, kind):
                            break
                    else:
                        raise AssertionError(('no input with safe gaps', kind, B, alpha, beta))
                    want = _reference_step(st, B, W, eos_id, pad_id, alpha, beta)
                    if kind == 'tie' and W > 1:
                        assert all(s.gap == 0.0 and s.parent[:2] == [0, 1] and (s.scores[0] != s.scores[1] or alpha == 0) and s.wsums[0] != s.wsums[1]
                                   and s.fused[0] == s.fused[1] for s in want)
                        ties += 1
                    if kind == 'bad_root':
                        assert want[0].parent == [-1] * W and (B == 1 or want[1].parent == [-1] * W) and (B < 3 or want[2].parent[0] == 0)
                    if kind == 'only_eos' and W <= 3 and alpha == 0:
                        assert all(eos_id in s.picked for s in want)
                    for b, par, cls, n_cands in st.get('heavy', []):
                        if n_cands > W:
                            assert (par, cls) not in zip(want[b].parent, want[b].picked)
                            dropped += 1
                    if kind == 'nonfinite':
                        blocked += 1
                        for b, s in enumerate(want):      # no picked arc has a non-finite weight
                            for par, cls in zip(s.parent, s.picked):
                                if par >= 0 and cls != pad_id:
                                    assert torch.isfinite(st['weight'][int(st['nodes'][b * W + par]), cls])
                    if kind == 'cycle':
                        loops += sum(1 for b, s in enumerate(want) for par, node, fin in zip(s.parent, s.nodes, s.finished)      # (no trie has such an arc)
                                     if par >= 0 and not fin and node == int(st['nodes'][b * W + par]))
                    dead_slots += sum(p == -1 for s in want for p in s.parent)
                    got = _run_step(st, B, W, C, eos_id, pad_id, alpha, beta)
                    errs = _compare_step(got, want, W, st['step'], alpha)
                    worst = [max(a, b) for a, b in zip(worst, errs)]
                    again = _run_step(st, B, W, C, eos_id, pad_id, alpha, beta)
                    for k in got:
                        assert torch.equal(_bits(got[k]), _bits(again[k])), f'{k}: two runs differ'
    assert dead_slots > 0 and (W == 1 or ties == 2 * len(ALPHAS) * len(BETAS)) and dropped > 0 and blocked > 0 and loops > 0, (dead_slots, ties, dropped, blocked, loops)
    print(f'[automaton step C={C} W={W}] worst score error {worst[0]:.3f}, worst wsum / f error {worst[1]:.3f} of their bounds, {dead_slots} dead slots, '
          f'{dropped} heavy arcs dropped, {loops} self-loops taken')


def _run_plain_or_lexicon_step(st, B, W, C, eos_id, pad_id, table=None):
    if table is not None:
        return TL._run_step(st, B, W, C, eos_id, pad_id, table=table)
    nat, lib = native()
    d = dict(tok=st['tok'].to(DEV, torch.int32).contiguous(), scores=st['scores'].to(DEV, torch.float32).contiguous(),
             finished=st['finished'].to(DEV, torch.uint8).contiguous(), lengths=st['lengths'].to(DEV, torch.int32).contiguous(),
             parent=torch.full((B * W,), -7, dtype=torch.int32, device=DEV), picked=torch.full((B * W,), -7, dtype=torch.int32, device=DEV))
    lg = st['logits'].to(DEV, torch.float32).contiguous()
    with nat.guard(lg):
        nat.check(lib.parseq_op_beam_step(nat.ptr(lg), B, W, C, st['step'], nat.ptr(d['tok']), LDT, nat.ptr(d['scores']), nat.ptr(d['finished']),
                                          nat.ptr(d['lengths']), nat.ptr(d['parent']), nat.ptr(d['picked']), eos_id, pad_id, nat.stream_ptr(lg)))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in d.items()}


def _fused32(scores, wsums, lengths, alpha, beta):
    """score + (alpha wsum + beta length) with every operation rounded to fp32 on its own (torch's fp32 tensor arithmetic on the CPU fuses
    nothing), -inf for a dead beam; one zero."""
    a, b = torch.tensor(alpha, dtype=torch.float32), torch.tensor(beta, dtype=torch.float32)
    p = a * wsums.float()
    q = b * lengths.float()
    f = scores.float() + (p + q)
    return torch.where(scores > NEG_INF, f + 0.0, torch.full_like(f, NEG_INF))


@pytest.mark.parametrize('alpha,beta', [(0.37, 0.11), (1.7, -0.3), (-0.9, 0.013)])
def test_fused_value_is_the_new_state_fused_operation_by_operation(alpha, beta):
    """f is recomputed from (score, wsum, length), never accumulated and never contracted: on weights and factors that are no short binary
    fractions (a fused multiply-add would round differently on most of them) the fused value the kernel ranked a new beam by has the bits of
    its written-out score, wsum and length fused in fp32 one operation at a time — what the next step and the write-out compute again."""
    C, W, B, eos_id, bos_id, pad_id = 95, 16, 3, 0, 95, 96
    st = _state('middle', B, W, C, 23, eos_id, pad_id, bos_id, alpha, beta)
    g = torch.Generator().manual_seed(7)
    st['weight'] = -3.0 * torch.rand(tuple(st['table'].shape), generator=g)
    st['wsums'] = torch.where(st['scores'] > NEG_INF, -9.0 * torch.rand(B * W, generator=g), torch.zeros(B * W))
    got = _run_step(st, B, W, C, eos_id, pad_id, alpha, beta)
    want = _fused32(got['scores'], got['wsums'], got['lengths'], alpha, beta)
    live = got['parent'] >= 0
    assert int(live.sum()) >= 2 * W and torch.equal(live, got['scores'] > NEG_INF)
    assert torch.equal(_bits(got['fused']), _bits(want))
    # the products are inexact here: contracting them would have changed bits
    a32 = torch.tensor(alpha, dtype=torch.float32)
    exact = a32.double() * got['wsums'][live].double()
    assert ((a32 * got['wsums'][live]).double() != exact).sum() >= W


def test_step_drops_a_candidate_whose_fused_value_overflows():
    """A finite alpha can overflow alpha * wsum.  Such a candidate is not allowed: +inf does not win the ranking, -inf and NaN do not enter
    it.  Every weight and weight sum is 0 but for the arcs of each image's best candidate (weight +8: f would be +inf) and its second best
    (-8: -inf) at alpha = 1e38, so the step is the restatement's without those two, and every other value is the unweighted one."""
    C, W, B, eos_id, bos_id, pad_id = 95, 3, 3, 0, 95, 96
    alpha, beta = 1e38, 0.0
    st = _state('cycle', B, W, C, 31, eos_id, pad_id, bos_id, 0.0, 0.0)
    st['weight'] = torch.zeros(tuple(st['table'].shape))
    st['wsums'] = torch.zeros(B * W)
    table = st['table'].tolist()
    hit = []
    for b in range(B):
        args = _image_args(st, b, W)
        fresh = [c for c in AR.rank_candidates(*args[:5], args[6], table, st['weight'].double().tolist(), st['step'], eos_id, 0.0, 0.0) if c[2] >= 0]
        assert len(fresh) > W + 2
        for (_, par, cls, _, _), wt in zip(fresh[:2], (8.0, -8.0)):
            st['weight'][int(st['nodes'][b * W + par]), cls] = wt
            hit.append((b, par, cls))
    want = _reference_step(st, B, W, eos_id, pad_id, alpha, beta)
    for b, par, cls in hit:
        assert (par, cls) not in zip(want[b].parent, want[b].picked)
    assert all(s.gap >= 1e-3 for s in want)
    got = _run_step(st, B, W, C, eos_id, pad_id, alpha, beta)
    _compare_step(got, want, W, st['step'], alpha)
    assert torch.isfinite(got['fused'][got['parent'] >= 0]).all() and not got['wsums'].any()


@pytest.mark.parametrize('kind', ['start', 'middle', 'only_eos', 'bad_child', 'bad_root'])
def test_step_without_a_prior_is_the_lexicon_step_on_bits(kind):
    """alpha = beta = 0 over a lexicon's table, whatever finite weights it carries: parents, tokens, flags, lengths, nodes, words and the bits
    of the scores are parseq_op_beam_step_lexicon's, and f is the score."""
    C, W, B, eos_id, bos_id, pad_id = 95, 5, 3, 0, 95, 96
    st = _state(kind, B, W, C, 11, eos_id, pad_id, bos_id, 0.0, 0.0)
    got = _run_step(st, B, W, C, eos_id, pad_id, 0.0, 0.0)
    want = _run_plain_or_lexicon_step(st, B, W, C, eos_id, pad_id, table=st['table'])
    for k, v in want.items():
        assert torch.equal(_bits(got[k]), _bits(v)), k
    assert torch.equal(_bits(got['fused']), _bits(got['scores']))


@pytest.mark.parametrize('alpha', [0.0, 0.7, 1.0, -3.0])
def test_step_under_a_free_automaton_is_the_plain_step_on_bits(alpha):
    """One state, every class allowed at weight 0, any alpha: parseq_op_beam_step's outputs, bit for bit; the weight sums stay 0."""
    C, W, B, eos_id, bos_id, pad_id = 95, 5, 2, 0, 95, 96
    st = _state('middle', B, W, C, 5, eos_id, pad_id, bos_id, alpha, 0.0)
    st['nodes'] = torch.where(st['scores'] > NEG_INF, 0, -1)
    st['wsums'] = torch.zeros(B * W)
    free = torch.zeros(1, C, dtype=torch.int32)
    got = _run_step(st, B, W, C, eos_id, pad_id, alpha, 0.0, table=free, weight=torch.zeros(1, C))
    want = _run_plain_or_lexicon_step(st, B, W, C, eos_id, pad_id)
    for k, v in want.items():
        assert torch.equal(_bits(got[k]), _bits(v)), k
    assert torch.equal(_bits(got['fused']), _bits(got['scores'])) and not got['wsums'].any()


# -------------------------------------------------------------------------------------------------------------------
# 2. the whole call: the two bit-equalities
# -------------------------------------------------------------------------------------------------------------------
_model = TL._model


@functools.lru_cache(maxsize=None)
def _shared_words():
    """test_lexicon_beam's 40 shared words with a count each."""
    words = TL._random_words(40, 7, 7)
    rng = random.Random(8)
    return words, [float(rng.randint(1, 400)) for _ in words]


@functools.lru_cache(maxsize=None)
def _shared_automaton(kind):
    words, counts = _shared_words()
    return Automaton.from_lexicon(words, counts, TOK) if kind == 'trie' else Automaton.ngram(words, 3, TOK)


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_whole_call_bit_equalities(name, precision):
    cfg = CONFIGS[name]
    m = _model(name, precision)
    x = synth_images(5, cfg, seed=11).to(DEV)
    trie = _shared_automaton('trie')
    free = Automaton(torch.zeros(1, trie.num_classes, dtype=torch.int32), torch.zeros(1, trie.num_classes))
    with torch.inference_mode():
        lex = m.beam_search(x, 3, 6, lexicon=TL._shared_lexicon())
        no_prior = m.model.beam_search(m.tokenizer, x, 3, 6, automaton=trie, alpha=0.0, beta=0.0, trace=True)
        plain = m.model.beam_search(m.tokenizer, x, 3, 6, trace=True)
        unconstrained = m.model.beam_search(m.tokenizer, x, 3, 6, automaton=free, alpha=0.37, trace=True)
    torch.cuda.synchronize()
    assert torch.equal(trie.next, TL._shared_lexicon().next)
    for k in ('tokens', 'scores', 'lengths', 'finished', 'words'):
        assert torch.equal(_bits(getattr(no_prior, k)), _bits(getattr(lex, k))), k
    assert torch.equal(_bits(no_prior.model_scores), _bits(lex.scores))
    for k in ('tokens', 'scores', 'lengths', 'finished', 'trace_logits', 'trace_tokens_in', 'trace_parent', 'trace_score'):
        assert torch.equal(_bits(getattr(unconstrained, k)), _bits(getattr(plain, k))), k
    assert torch.equal(_bits(unconstrained.model_scores), _bits(plain.scores)) and not unconstrained.priors.any()
    live = plain.scores > NEG_INF
    assert torch.equal(unconstrained.words == 0, (plain.finished == 1) & live) and torch.equal(unconstrained.words == -1, ~((plain.finished == 1) & live))


# -------------------------------------------------------------------------------------------------------------------
# 3. the whole search, replayed from its traced logits
# -------------------------------------------------------------------------------------------------------------------
# The crops are test_lexicon_beam's (EOS_BIAS, SEARCH_SEED; B = 8, W = 3, max_length = 5).  Checked ON THE CPU with the oracle-driven restatement:
# under neither automaton does any (image, step) decision of 48 have a gap in f under twice the step bound; the smallest gaps are 6.7e-3 (trie) and
# 2.7e-3 (trigram) for parseq-tiny, 2.1e-2 and 6.9e-3 for parseq, 45 times the bound of their step at the least — test_whole_search_decisions
# asserts the property again.
SEARCH_ALPHA, SEARCH_BETA = 0.5, 0.25


def _step_limits(rep, steps, alpha):
    """Per step the bound on f: the score's and the weights', with M from the restated search's live beams after that step."""
    limits = []
    for i in range(steps):
        f = rep.step_scores[i]
        big = float(f[f > NEG_INF].abs().max()) if (f > NEG_INF).any() else 0.0
        limits.append(weight_bound(i, max(big, float(rep.priors.abs().max()), abs(alpha) * float(rep.priors.abs().max()))))
    return torch.tensor(limits, dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def _oracle_search(name, kind):
    cfg = CONFIGS[name]
    aut = _shared_automaton(kind)
    images = synth_images(TL.SEARCH_B, cfg, seed=TL.SEARCH_SEED[name])
    return AR.beam_search(R.oracle_step_logits(TL._weights(name), cfg, images, TL.SEARCH_W), TL.SEARCH_B, TL.SEARCH_W, TL.SEARCH_MAXLEN + 1, cfg.bos_id,
                          cfg.eos_id, cfg.pad_id, aut.next, aut.weight, SEARCH_ALPHA, SEARCH_BETA)


@pytest.mark.parametrize('kind', ['trie', 'ngram'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_whole_search_decisions(name, precision, kind):
    """test_lexicon_beam's method under a weighted trie of 40 words and under a trigram of the same words: the restatement replayed from the
    traced logits makes the decisions the device made, the traced and returned f within the step bound, model_scores and priors beside it.  A
    decision whose float64 gap in f does not exceed that bound is skipped and its image drops out from there on; at most 2 % may be."""
    cfg = CONFIGS[name]
    aut = _shared_automaton(kind)
    steps, B, W = TL.SEARCH_MAXLEN + 1, TL.SEARCH_B, TL.SEARCH_W
    ora = _oracle_search(name, kind)
    assert int((ora.gaps <= 2 * _step_limits(ora, steps, SEARCH_ALPHA)).sum()) == 0
    assert (ora.finished == 1).any() and (ora.priors < 0).any()

    images = synth_images(B, cfg, seed=TL.SEARCH_SEED[name])
    m = _model(name, precision)
    with torch.inference_mode():
        out = m.model.beam_search(m.tokenizer, images.to(DEV), W, TL.SEARCH_MAXLEN, trace=True, automaton=aut, alpha=SEARCH_ALPHA, beta=SEARCH_BETA)
    torch.cuda.synchronize()
    res = {k: getattr(out, k).cpu() for k in ('tokens', 'scores', 'lengths', 'finished', 'words', 'model_scores', 'priors', 'trace_logits', 'trace_tokens_in',
                                              'trace_parent', 'trace_score')}
    rep = AR.beam_search(lambda h: res['trace_logits'][h.shape[1] - 1], B, W, steps, cfg.bos_id, cfg.eos_id, cfg.pad_id, aut.next, aut.weight, SEARCH_ALPHA,
                         SEARCH_BETA)
    limits = _step_limits(rep, steps, SEARCH_ALPHA)
    valid = torch.ones(B, dtype=torch.bool)
    skipped, worst = 0, 0.0
    for i in range(steps):
        assert torch.equal(res['trace_tokens_in'][i].long().view(B, W, steps)[valid], rep.tokens_in[i].view(B, W, steps)[valid]), f'histories of step {i}'
        for b in range(B):
            if valid[b] and rep.gaps[b, i] <= limits[i]:
                valid[b] = False
                skipped += 1
        assert torch.equal(res['trace_parent'][i].long().view(B, W)[valid], rep.parents[i][valid]), f'parents of step {i}'
        got, want = res['trace_score'][i].view(B, W)[valid], rep.step_scores[i][valid]
        assert torch.equal(got == NEG_INF, want == NEG_INF)
        d = (got.double() - want).abs()
        d = d[~torch.isnan(d)]
        worst = max(worst, d.max().item() / limits[i].item())
        assert d.max().item() <= limits[i], f'step {i}: f error {d.max().item():.3e}'
    print(f'[automaton decisions {kind} {name} {precision}] skipped {skipped} of {B * steps}, worst f error {worst:.3f} of the bound, least gap {rep.gaps.min().item():.2e}')
    assert skipped <= 0.02 * B * steps
    for k in ('tokens', 'lengths', 'finished', 'words'):
        assert torch.equal(res[k].long()[valid], getattr(rep, k)[valid]), k
    assert torch.equal(_bits(res['scores'][valid]), _bits(res['trace_score'][-1].view(B, W)[valid]))
    live = rep.model_scores[valid] > NEG_INF
    assert torch.equal(res['model_scores'][valid] > NEG_INF, live)
    assert ((res['model_scores'][valid].double() - rep.model_scores[valid]).abs()[live] <= score_bound(steps - 1)).all()
    assert ((res['priors'][valid].double() - rep.priors[valid]).abs() <= limits[-1]).all()
    if kind == 'ngram':      # every state accepts with tag 0
        assert torch.equal(res['words'] == 0, (res['finished'] == 1) & (res['model_scores'] > NEG_INF))


# -------------------------------------------------------------------------------------------------------------------
# 4. exhaustive: per-image automata no larger than the beam, against the oracle
# -------------------------------------------------------------------------------------------------------------------
EXH_COUNTS = (1.0, 9.0, 40.0, 150.0)      # of an image's four words, by position in its list: unequal, so the priors order them


def _exhaustive_automata(lists):
    return Automaton.stack([Automaton.from_lexicon(ws, EXH_COUNTS, TOK) for ws in lists])


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_exhaustive_search_against_the_oracle(name, precision):
    """Per-image weighted tries of W = 4 words drop no candidate: every image returns exactly its words, finished; model_scores are the oracle's
    teacher-forced sums within 8e-3, priors the words' path sums in fp32, scores their fusion, and the order is the oracle's fused order
    wherever its gaps exceed the bar.  With alpha large enough for the priors to dominate — derived below from the oracle's spread of scores
    and the smallest gap between two priors — the order is the counts' order."""
    images, lists, want = TL._exhaustive_reference(name)
    B, W = TL.EXH_B, TL.EXH_W
    aut, roots = _exhaustive_automata(lists)
    m = _model(name, precision)
    # the priors of the four counts: log((count + 1) / (sum + 4)), the same for every image
    log_prior = [torch.log(torch.tensor((c + 1.0) / (sum(EXH_COUNTS) + len(EXH_COUNTS)), dtype=torch.float64)).item() for c in EXH_COUNTS]
    spread = max((want[b].max() - want[b].min()).item() for b in range(B))
    prior_gap = min(abs(a - b) for a, b in zip(log_prior, log_prior[1:]))
    dominating = (spread + 2 * WHOLE_SCORE_BAR) / prior_gap * 1.25        # alpha * prior_gap exceeds any difference of scores, the bar and a quarter more
    for alpha, beta in ((0.5, 0.3), (dominating, 0.0)):
        with torch.inference_mode():
            res = m.beam_search(images.to(DEV), W, TL.EXH_MAXLEN, automaton=aut.to(DEV), roots=roots, alpha=alpha, beta=beta)
            beams = m.tokenizer.decode_beams(res, aut)
            chars = m.tokenizer.decode_beams(res)
        assert res.finished.cpu().tolist() == [[1] * W] * B
        f, ms, pr, ln = res.scores.cpu().double(), res.model_scores.cpu().double(), res.priors.cpu().double(), res.lengths.cpu().double()
        words = res.words.cpu().tolist()
        worst, compared = 0.0, 0
        for b in range(B):
            assert sorted(words[b]) == list(range(b * W, (b + 1) * W))
            assert [aut.words[k] for k in words[b]] == [s for s, _ in beams[b]] == [s for s, _ in chars[b]]
            assert all(x >= y for x, y in zip(f[b].tolist(), f[b].tolist()[1:]))
            fused = []
            for r, k in enumerate(words[b]):
                k -= b * W
                worst = max(worst, abs(ms[b, r].item() - want[b, k].item()))
                # the fp32 weights of the stacked table summed in fp32 along the word and its <eos>, from 0, in the kernel's order
                path, state = torch.zeros((), dtype=torch.float32), int(roots[b])
                for c in TOK._tok2ids(lists[b][k]) + [TOK.eos_id]:
                    path = path + aut.weight[state, c]
                    state = int(aut.next[state, c])
                assert path.dtype == torch.float32 and state == words[b][r]
                assert abs(pr[b, r].item() - path.item()) <= 4 * 2.0 ** -24 * abs(pr[b, r].item())
                # ... which is the log of the word's share of the counts: every weight rounded once (2^-24 of it; the weights of a path, all
                # negative, add up to the prior: 2^-24 of the prior together), one rounding per sum after the first (2^-24 of a partial sum,
                # none larger than the prior: len of them), and one more 2^-24 to spare for those bounds' own rounding
                assert abs(path.item() - log_prior[k]) <= (len(lists[b][k]) + 2) * 2.0 ** -24 * abs(log_prior[k])
                terms = (ms[b, r].item(), alpha * pr[b, r].item(), beta * ln[b, r].item())
                assert abs(f[b, r].item() - (terms[0] + (terms[1] + terms[2]))) <= 3 * 2.0 ** -24 * max(abs(t) for t in terms + (f[b, r].item(),))
            # and on bits: the carried (score, wsum, length) fused operation by operation in fp32, no product contracted into a sum
            assert torch.equal(_bits(res.scores.cpu()[b]), _bits(_fused32(res.model_scores.cpu()[b], res.priors.cpu()[b], res.lengths.cpu()[b], alpha, beta)))
            oracle_f = [want[b, k].item() + (alpha * log_prior[k] + beta * len(lists[b][k])) for k in range(W)]
            order = sorted(range(W), key=lambda k: -oracle_f[k])
            ranked = [oracle_f[k] for k in order]
            if min(x - y for x, y in zip(ranked, ranked[1:])) > WHOLE_SCORE_BAR * (1 + abs(alpha) * 1e-3):
                assert [k - b * W for k in words[b]] == order
                compared += 1
            if alpha == dominating:
                assert [k - b * W for k in words[b]] == [3, 2, 1, 0]
        print(f'[automaton exhaustive {name} {precision} alpha={alpha:.3g}] worst |dscore| {worst:.3e} (bar {WHOLE_SCORE_BAR:.0e}), order compared on '
              f'{compared} of {B} images')
        assert worst <= WHOLE_SCORE_BAR and compared >= B // 2


# -------------------------------------------------------------------------------------------------------------------
# 5. patterns end to end, per-crop roots
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_patterns_end_to_end(name, precision):
    cfg = CONFIGS[name]
    m = _model(name, precision)
    x = synth_images(6, cfg, seed=TL.SEARCH_SEED[name]).to(DEV)
    patterns = [r'[0-9]{3}', r'[a-z]+[0-9]?', r'(ab|[A-C])*\.\w{1,2}']
    automata = [Automaton.pattern(p, TOK) for p in patterns]
    finished_readings = 0
    for p, aut in zip(patterns, automata):
        with torch.inference_mode():
            res = m.beam_search(x, 4, 5, automaton=aut, alpha=1.0, beta=0.5)
        fin, pri, tags = res.finished.cpu().tolist(), res.priors.cpu(), res.words.cpu().tolist()
        for alts, fl, tg in zip(m.tokenizer.decode_beams(res, aut), fin, tags):      # (no words: the characters)
            for (text, _), f, t in zip(alts, fl, tg):
                if f:
                    assert re.fullmatch(p, text) and t == 0, (p, text)
                    assert p != patterns[0] or len(text) == 3
                    finished_readings += 1
                else:
                    assert t == -1 and aut.walk(TOK._tok2ids(text))[2] == 0.0        # an unfinished reading is a live prefix
        assert not pri.any()
    assert finished_readings >= 12
    # every crop its own pattern
    both, roots = Automaton.stack(automata)
    per_crop = roots[torch.arange(6) % 3]
    with torch.inference_mode():
        res = m.beam_search(x, 4, 5, automaton=both, roots=per_crop, beta=0.5)
        alone = [m.beam_search(x, 4, 5, automaton=aut, beta=0.5) for aut in automata]
    for b in range(6):
        for k in ('tokens', 'scores', 'lengths', 'finished', 'words', 'model_scores', 'priors'):
            assert torch.equal(_bits(getattr(res, k)[b]), _bits(getattr(alone[b % 3], k)[b])), (b, k)


def test_decode_beams_returns_the_words_of_an_automaton():
    m = _model('parseq-tiny', 'bf16x3')
    x = synth_images(4, CONFIGS['parseq-tiny'], seed=3).to(DEV)
    tok = m.tokenizer
    aut = Automaton.from_lexicon(['Hello', 'HELP', 'world'], [5, 1, 9], Tokenizer('abcdefghijklmnopqrstuvwxyz'), fold_case=True)
    wide = Automaton.from_lexicon(_shared_words()[0], _shared_words()[1], TOK)
    with torch.inference_mode():
        res = m.beam_search(x, 3, 8, automaton=wide)
    for alts, raw, fl, tg in zip(tok.decode_beams(res, wide), tok.decode_beams(res), res.finished.cpu().tolist(), res.words.cpu().tolist()):
        for (label, f), (chars, f2), fin, t in zip(alts, raw, fl, tg):
            assert f == f2 and ((label == wide.words[t] == chars) if fin else (t == -1 and label == chars))
    assert aut.words == ['Hello', 'HELP', 'world'] and aut.walk([8, 5, 12, 12, 15])[0] == 0
    with pytest.raises(ValueError, match='no `words`'):
        tok.decode_beams(m.beam_search(x, 3, 8), wide)


# -------------------------------------------------------------------------------------------------------------------
# 6. refusals, read.py
# -------------------------------------------------------------------------------------------------------------------
def test_library_refusals():
    nat, lib = native()
    name = 'parseq-tiny'
    cfg = CONFIGS[name]
    m = _model(name, 'bf16x3')
    x = synth_images(4, cfg, seed=3).to(DEV)
    B, W, steps = 4, 2, 4
    plan = m.model._plan(B * W)
    table, weight = _shared_automaton('trie').table(DEV)

    def call(tb=table, wt=weight, states=table.shape[0], alpha=1.0, beta=0.0, missing=None, short=0, width=W):
        rows = B * max(width, 1)
        outs = [torch.full((rows * steps,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), -7.0, dtype=torch.float32, device=DEV),
                torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), 7, dtype=torch.uint8, device=DEV),
                torch.full((rows,), -7, dtype=torch.int32, device=DEV), torch.full((rows,), -7.0, dtype=torch.float32, device=DEV),
                torch.full((rows,), -7.0, dtype=torch.float32, device=DEV)]
        need = lib.parseq_beam_automaton_workspace_bytes(plan, B, width, steps)
        ws = torch.empty(max(need, 1 << 20), dtype=torch.uint8, device=DEV)
        ptrs = [None if missing == k else nat.ptr(o) for k, o in enumerate(outs)]
        status = lib.parseq_forward_beam_automaton(plan, nat.ptr(x), nat.dtype_code(x.dtype), B, width, steps, *ptrs[:4], None, nat.ptr(ws),
                                                   (need - short) if short else ws.numel(), nat.stream_ptr(x), nat.ptr(tb) if tb is not None else None,
                                                   nat.ptr(wt) if wt is not None else None, states, None, alpha, beta, *ptrs[4:])
        torch.cuda.synchronize()
        canaries = (-7, -7.0, -7, 7, -7, -7.0, -7.0)
        return status, all(bool((o == c).all()) for o, c in zip(outs, canaries)), need

    lexicon_bytes = lib.parseq_beam_lexicon_workspace_bytes(plan, B, W, steps)
    status, untouched, need = call()
    assert status == 0 and not untouched and lexicon_bytes < need <= lexicon_bytes + 256 * ((B * W * 4 + 255) // 256)
    assert call(wt=None)[:2] == (-1, True) and b'weights' in lib.parseq_last_error()
    assert call(tb=None)[:2] == (-1, True) and b'trie' in lib.parseq_last_error()
    assert call(states=0)[:2] == (-1, True) and b'trie_nodes' in lib.parseq_last_error()
    for alpha, beta in ((float('nan'), 0.0), (float('inf'), 0.0), (1.0, float('-inf')), (1.0, float('nan'))):
        assert call(alpha=alpha, beta=beta)[:2] == (-1, True) and b'finite' in lib.parseq_last_error()
    for missing in (0, 1, 4, 5, 6):
        assert call(missing=missing)[:2] == (-1, True)
    assert call(short=1)[:2] == (-1, True) and b'workspace' in lib.parseq_last_error()
    assert call(width=17)[:2] == (-1, True) and lib.parseq_beam_automaton_workspace_bytes(plan, B, 17, steps) == 0
    # the operator hook
    z = torch.zeros(W, 95, device=DEV)
    i32 = torch.zeros(W * LDT, dtype=torch.int32, device=DEV)
    u8 = torch.zeros(W, dtype=torch.uint8, device=DEV)

    def step(tb=table, wt=weight, n=table.shape[0], alpha=1.0, beta=0.0, wsums=z):
        return lib.parseq_op_beam_step_automaton(nat.ptr(z), 1, W, 95, 0, nat.ptr(i32), LDT, nat.ptr(z), nat.ptr(u8), nat.ptr(i32), None, nat.ptr(i32), 0, 96,
                                                 nat.stream_ptr(z), nat.ptr(tb) if tb is not None else None, nat.ptr(wt) if wt is not None else None, n,
                                                 nat.ptr(i32), nat.ptr(i32), alpha, beta, nat.ptr(wsums) if wsums is not None else None, None)
    assert step() == 0
    torch.cuda.synchronize()
    for kw in (dict(tb=None), dict(wt=None), dict(n=0), dict(alpha=float('nan')), dict(beta=float('inf')), dict(wsums=None)):
        assert step(**kw) == -1, kw


def test_python_surface_refusals():
    from parseq_amd import create_model
    m = _model('parseq-tiny', 'bf16x3')
    x = synth_images(4, CONFIGS['parseq-tiny'], seed=3).to(DEV)
    aut = _shared_automaton('trie')
    for refine in ('score', 'edit'):
        with pytest.raises(ValueError, match='refine= under a weighted automaton'):
            m.beam_search(x, 2, automaton=aut, refine=refine)
    with pytest.raises(ValueError, match='exclude each other'):
        m.beam_search(x, 2, automaton=aut, lexicon=TL._shared_lexicon())
    with pytest.raises(ValueError, match='finite'):
        m.beam_search(x, 2, automaton=aut, alpha=float('nan'))
    with pytest.raises(ValueError, match='finite'):
        m.beam_search(x, 2, automaton=aut, beta=float('inf'))
    with pytest.raises(ValueError, match='without an automaton'):
        m.beam_search(x, 2, alpha=0.5)
    with pytest.raises(ValueError, match='automaton tables'):
        m.beam_search(x, 2, automaton=Automaton.pattern('[0-9]+', Tokenizer('0123456789')))
    with pytest.raises(ValueError, match=r'roots must be \[batch\]'):
        m.beam_search(x, 2, automaton=aut, roots=torch.zeros(3, dtype=torch.int32))
    vit = create_model('vitstr', precision='bf16').eval().to(DEV)
    with pytest.raises(ValueError, match='ViTSTR'):
        vit.beam_search(x, 2, automaton=aut)
    deep = create_model('parseq-tiny', dec_depth=2, precision='bf16x3').eval().to(DEV)
    with pytest.raises(ValueError, match='dec_depth'):
        deep.beam_search(x, 2, automaton=aut)
    # a root outside the table starts its crop dead
    roots = torch.tensor([0, aut.num_states, -1, 0], dtype=torch.int32)
    with torch.inference_mode():
        res = m.beam_search(x, 2, 4, automaton=aut, roots=roots)
    dead = torch.tensor([False, True, True, False])
    assert (res.scores.cpu()[dead] == NEG_INF).all() and (res.model_scores.cpu()[dead] == NEG_INF).all() and not res.priors.cpu()[dead].any()
    assert (res.words.cpu()[dead] == -1).all() and (res.scores.cpu()[~dead, 0] > NEG_INF).all()


def test_read_cli_automata(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip('PIL.Image')
    import read as read_cli
    from oracle.make_resize_golden import make_input
    files = []
    for i, (h, w) in enumerate([(40, 150), (32, 128)]):
        f = tmp_path / f'crop{i}.png'
        Image.fromarray(make_input(h, w, 1 - i % 2), 'RGB').save(f)
        files.append(str(f))
    words = [w for w in dict.fromkeys(TL._random_words(30, 21, 6)) if not any(ch.isspace() for ch in w)]
    listing = tmp_path / 'counts.txt'
    listing.write_text(''.join(f'{w} {3 * k + 1}\n' for k, w in enumerate(words)))
    corpus = tmp_path / 'corpus.txt'
    corpus.write_text('\n'.join(words) + '\n')
    m = _model('parseq', 'bf16x3')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    base = ['pretrained=parseq', '--images', *files, '--device', DEV]

    def run(*flags):
        read_cli.main(base + list(flags))
        return capsys.readouterr().out.splitlines()[1:]

    def alternatives(block, n):
        """The n alternatives under each of the two images: (fused, model log-probability, prior, label) and the headline's label."""
        assert len(block) == 2 * (n + 1)
        out = []
        for k, f in zip((0, n + 1), files):
            assert block[k].startswith(f + ': ')
            rows = [re.fullmatch(r' {4}\s*(\S+)  lp=\s*(\S+) prior=\s*(\S+)  (.*)', line) for line in block[k + 1:k + 1 + n]]
            assert all(rows) and rows[0].group(4) == block[k][len(f) + 2:]
            vals = [(float(r.group(1)), float(r.group(2)), float(r.group(3)), r.group(4)) for r in rows]
            assert all(a[0] >= b[0] for a, b in zip(vals, vals[1:]))
            out.append(vals)
        return out

    out = run('--lexicon', str(listing), '--priors')
    assert len(out) == 2 and all(line.startswith(f + ': ') and line[len(f) + 2:] in words for f, line in zip(files, out))
    block = run('--lexicon', str(listing), '--priors', '--nbest', '3', '--beam', '6', '--lm-weight', '0.5')
    for vals in alternatives(block, 3):
        assert all(any(w.startswith(label) for w in words) for *_, label in vals)
        assert all(abs(f - (lp + 0.5 * prior)) <= 2e-4 and prior < 0 for f, lp, prior, _ in vals)
    block = run('--lm', str(corpus), '--lm-order', '2', '--nbest', '2', '--lm-weight', '0.25', '--char-bonus', '0.5')
    for vals in alternatives(block, 2):
        assert all(abs(f - (lp + 0.25 * prior + 0.5 * len(label))) <= 2e-4 and prior < 0 for f, lp, prior, label in vals)
    block = run('--pattern', '[0-9]{2}[a-c]?', '--nbest', '4')
    for vals in alternatives(block, 4):
        assert all(re.fullmatch('[0-9]{2}[a-c]?', label) and prior == 0 and abs(f - lp) <= 1e-4 for f, lp, prior, label in vals)
    assert run('--pattern', '[0-9]{2}[a-c]?') == [block[0], block[5]]
