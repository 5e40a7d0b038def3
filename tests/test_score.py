"""GPU tests of scoring given readings: the two kernels after the decoder pass through `parseq_op_score_rows` /
`parseq_op_score_rank` against the float64 restatement (tests/score_reference.py) and against section 20's statistics bit for bit, then
the whole call `parseq_score` against the restatement on the CPU oracle, its identities on the device and its refusals.

Bounds.  One log-soft-max term: 4e-5 (tests/test_beam.py derives it for |score| < 128; the states below keep every summed target among
the eight best classes of its position, asserted).  The whole call: the logits gate of tests/test_hip_parity.py for the plan precision
(1e-3 for fp32 and bf16x3, 6e-2 for bf16) moves a log-soft-max by at most twice the logits' sup-norm error, so a score of `terms` summed
positions is held to (2 * gate + 4e-5) * terms.

Whole-call seeds: the crops synth_images(3, cfg, seed=WHOLE_SEED[name]) with the synthetic weights of seed 0.  Checked on the CPU with the
oracle alone (asserted again in every test that compares ranks): for both models and every crop the six candidates' forward, mirrored and
mixed scores are at least 0.1 apart (0.124 for PARSeq-Ti, 0.47 for PARSeq-S; the closest pair is [5, 9, 11] and
[5, 9, 12] or [5, 9] and [5, 9, 12]); the scores range from -2.9 to -58.
"""
import functools
import math

import numpy as np
import pytest
import torch

import score_reference as R
from gpu_util import DEV, make_model, native
from oracle.synth import CONFIGS, synth_images, synth_state_dict
from parseq_amd import score as S

pytestmark = pytest.mark.gpu

NEG_INF = float('-inf')
TERM_BOUND = 4e-5
TOP = 8
GATE = {'fp32': 1e-3, 'bf16x3': 1e-3, 'bf16': 6e-2}
WHOLE_SEED = {'parseq-tiny': 8, 'parseq': 7}
WHOLE_CANDS = [[5, 9, 11], [5, 9], [40, 2, 2, 7, 30, 1], [], [3] * 10, [5, 9, 12]]
WHOLE_B, WHOLE_T = 3, 10
BF16_PAIRS_LEFT_OUT = {'parseq-tiny': 3, 'parseq': 0}      # of the 3 * 5 adjacent pairs of the oracle's mixed keys, those closer than twice the bf16 bound


def whole_bound(precision, terms):
    return (2 * GATE[precision] + TERM_BOUND) * terms


# -------------------------------------------------------------------------------------------------------------------
# 1. the kernels alone
# -------------------------------------------------------------------------------------------------------------------
def _state(B, N, L, C, K, seed):
    """Logits [K][B * N, L, C] as tests/test_beam_refine.py::_state makes them (per row and position a permutation of a 0.25 grid times a
    factor in [0.5, 1]: distinct values, |logit| <= 30) and the rows' candidates: row 1 absent, row 7 invalid, the others of every length
    0 .. L - 1 in turn, each summed target among the TOP best classes of its position under every order."""
    eos_id = 0
    g = torch.Generator().manual_seed(seed)
    rows = B * N
    logits = torch.stack([(torch.randperm(C, generator=g).float() - C // 2) * 0.25 for _ in range(K * rows * L)]).view(K, rows, L, C)
    logits = logits * (0.5 + 0.5 * torch.rand(K, rows, L, 1, generator=g))
    assert logits.abs().max() <= 30
    targets = torch.full((rows, L), -1, dtype=torch.int32)
    lengths = torch.zeros(rows, dtype=torch.int32)
    valid = torch.ones(rows, dtype=torch.uint8)
    for r in range(rows):
        if r in (1, 7):
            valid[r] = 0
            targets[r] = C + 3 if r == 7 else -1      # what an invalid row might hold: never read
            continue
        n = (r * 5 + 3) % L if r != 2 else L - 1
        lengths[r] = n
        for i in range(n + 1):
            t = eos_id if i == n else 1 + int(torch.randint(0, C - 1, (), generator=g))
            targets[r, i] = t
            for k in range(K):      # lift the target among the TOP best of its position by swapping it with the class that stands there
                other = int(logits[k, r, i].argsort(descending=True)[int(torch.randint(0, TOP, (), generator=g))])
                a, b = float(logits[k, r, i, t]), float(logits[k, r, i, other])
                logits[k, r, i, t], logits[k, r, i, other] = b, a
    return logits, targets, lengths, valid


def _run_rows(logits, targets, lengths, valid, K):
    rows, L = targets.shape
    order_scores = torch.full((rows, K), 777.0, dtype=torch.float32, device=DEV)
    char_lp = torch.full((rows, K, L), 777.0, dtype=torch.float32, device=DEV)
    t, n, v = targets.to(DEV), lengths.to(DEV), valid.to(DEV)
    for k in range(K):
        S.score_rows(logits[k].to(DEV).contiguous(), t, n, v, K, k, order_scores, char_lp)
    torch.cuda.synchronize()
    return order_scores.cpu(), char_lp.cpu()


@pytest.mark.parametrize('L,C,K', [(2, 36, 1), (7, 95, 2), (26, 201, 6), (26, 36, 2), (7, 201, 1)])
def test_score_rows_against_float64(L, C, K):
    B, N = 3, 5
    logits, targets, lengths, valid = _state(B, N, L, C, K, seed=100 + L + C)
    got_s, got_lp = _run_rows(logits, targets, lengths, valid, K)
    worst = 0.0
    for k in range(K):
        want_lp, want_s = R.rows_reference(logits[k], targets, lengths, valid)
        assert want_s[valid.bool()].abs().max() < 128
        for r in range(B * N):
            n = int(lengths[r])
            if not valid[r]:
                assert got_s[r, k] == NEG_INF and (got_lp[r, k] == 0).all()
                continue
            assert (got_lp[r, k, n + 1:] == 0).all()
            err_lp = (got_lp[r, k, :n + 1].double() - want_lp[r, :n + 1]).abs().max().item()
            err = abs(float(got_s[r, k]) - float(want_s[r]))
            print(f'L {L} C {C} order {k} row {r} terms {n + 1}: |d score| {err:.2e} (bound {TERM_BOUND * (n + 1):.2e}), worst term {err_lp:.2e}')
            assert err_lp <= TERM_BOUND and err <= TERM_BOUND * (n + 1)
            worst = max(worst, err / (TERM_BOUND * (n + 1)))
            # the sum is the fp32 sum of the stored terms in ascending position
            s = torch.zeros((), dtype=torch.float32)
            for i in range(n + 1):
                s = s + got_lp[r, k, i]
            assert float(s) == float(got_s[r, k])
    print(f'score_rows L {L} C {C} K {K}: worst error {worst:.3f} of its bound')


@pytest.mark.parametrize('L,C', [(2, 36), (7, 95), (26, 201)])
def test_score_rows_bits_equal_the_refinement_statistics(L, C):
    """On the same logits the sums are the bits `parseq_op_beam_refine` (score mode) gives the same rows: it sums lp_tok of
    beam_refine_stats_kernel over positions 0 .. length and ranks the rows of an image by the result, so per image the sorted scores agree."""
    nat, lib = native()
    B, N, ldt = 3, 5, 32
    eos_id, pad_id, bos_id = 0, C + 1, C
    logits, targets, lengths, valid = _state(B, N, L, C, 1, seed=300 + L)
    got_s, _ = _run_rows(logits, targets, lengths, valid, 1)
    rows = B * N
    tok = torch.full((rows, ldt), pad_id, dtype=torch.int32)
    tok[:, 0] = bos_id
    for r in range(rows):
        if valid[r]:
            tok[r, 1:int(lengths[r]) + 2] = targets[r, :int(lengths[r]) + 1]
    d = dict(tok=tok.to(DEV), picked=tok[:, L].contiguous().to(DEV),
             scores=torch.where(valid.bool(), torch.full((rows,), -1.0), torch.full((rows,), NEG_INF)).to(DEV),
             finished=valid.clone().to(DEV), lengths=lengths.to(DEV), ar=torch.zeros(rows, device=DEV))
    lg = logits[0].to(DEV).contiguous()
    need = lib.parseq_op_beam_refine_workspace_bytes(B, N, L)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    with nat.guard(lg):
        nat.check(lib.parseq_op_beam_refine(nat.ptr(lg), B, N, C, L, 1, nat.ptr(d['tok']), ldt, nat.ptr(d['scores']), nat.ptr(d['finished']),
                                            nat.ptr(d['lengths']), nat.ptr(d['picked']), None, None, nat.ptr(d['ar']), eos_id, pad_id, nat.ptr(ws), need,
                                            nat.stream_ptr(lg)))
    torch.cuda.synchronize()
    refined = d['scores'].cpu().view(B, N)
    mine = got_s.view(B, N)
    for b in range(B):
        assert sorted(mine[b].tolist(), reverse=True) == refined[b].tolist()
    assert int((refined > NEG_INF).sum()) == int(valid.sum())


def test_score_rank_planted_keys():
    """An exact tie, a NaN, a crop with every candidate absent, -inf among finite keys, under both combinations and the length norm."""
    nan = float('nan')
    order_scores = torch.tensor([
        [[-3.0, -5.0], [-3.0, -5.0], [-1.0, -9.0], [-2.0, -2.0], [-40.0, -41.0], [-0.5, -30.0]],      # rows 0 and 1 tie exactly
        [[-3.0, nan], [nan, nan], [-7.0, -7.0], [NEG_INF, -2.0], [NEG_INF, NEG_INF], [-6.0, -8.0]],    # NaN reads as -inf
        [[-1.0, -1.0]] * 6,                                                                                # every candidate absent
        [[-4.0, -4.0], [-4.0, -4.0], [-4.0, -4.0], [-4.0, -4.0], [-4.0, -4.0], [-4.0, -4.0]],          # all tied: index order
    ], dtype=torch.float32)
    lengths = torch.tensor([[3, 3, 1, 7, 0, 2], [2, 2, 6, 1, 1, 3], [0] * 6, [5, 1, 3, 0, 2, 4]], dtype=torch.int32)
    valid = torch.ones(4, 6, dtype=torch.uint8)
    valid[2] = 0
    valid[0, 3] = 0
    for combine in ('mix', 'mean'):
        for normalize in (False, True):
            got_s, got_r = S.score_rank(order_scores.to(DEV), lengths.to(DEV), valid.to(DEV), combine, normalize)
            torch.cuda.synchronize()
            got_s, got_r = got_s.cpu().numpy(), got_r.cpu().numpy()
            want_s = R.combine(order_scores.numpy(), mean=combine == 'mean')
            want_s = np.where(valid.numpy().astype(bool), want_s, np.float32(NEG_INF))
            assert not np.isnan(got_s).any()
            fin = np.isfinite(want_s)
            assert np.array_equal(np.isfinite(got_s), fin) and np.array_equal(got_s[~fin], want_s[~fin])
            assert np.abs(got_s[fin].astype(np.float64) - want_s[fin]).max() <= 1e-6      # two fp64 exp / log against libm's, rounded to fp32 at |score| < 64
            for b in range(4):
                assert sorted(got_r[b].tolist()) == list(range(6))
            assert np.array_equal(got_r, R.rank(got_s, lengths.numpy(), valid.numpy(), normalize)), (combine, normalize)
            assert got_r[2].tolist() == list(range(6))
            assert got_s[0, 0] == got_s[0, 1] and list(got_r[0]).index(0) + 1 == list(got_r[0]).index(1)
            if not normalize:
                assert got_r[3].tolist() == list(range(6))
    # the planted order under the mixture, by hand: crop 0 keys = log-mean-exp of the pairs; row 3 is not valid
    got_s, got_r = S.score_rank(order_scores.to(DEV), lengths.to(DEV), valid.to(DEV))
    assert got_r.cpu()[0].tolist() == [5, 2, 0, 1, 4, 3]
    assert got_r.cpu()[1].tolist() == [3, 0, 5, 2, 1, 4]
    # one order: the order's own bits
    one = order_scores[:, :, :1].contiguous()
    for combine in ('mix', 'mean'):
        s1, _ = S.score_rank(one.to(DEV), lengths.to(DEV), torch.ones(4, 6, dtype=torch.uint8, device=DEV), combine)
        want = torch.where(torch.isnan(one[:, :, 0]), torch.full((), NEG_INF), one[:, :, 0])
        assert torch.equal(s1.cpu(), want)


# -------------------------------------------------------------------------------------------------------------------
# 2. the whole call
# -------------------------------------------------------------------------------------------------------------------
def _perms(T, which):
    return {'forward': S.parse_orders('forward', T), 'both': S.parse_orders('both', T)}[which]


@functools.lru_cache(maxsize=None)
def _oracle(name, mean=False, normalize=False):
    cfg = CONFIGS[name]
    images = synth_images(WHOLE_B, cfg, seed=WHOLE_SEED[name])
    with torch.inference_mode():
        return R.score(synth_state_dict(cfg, 0), cfg, images, [WHOLE_CANDS] * WHOLE_B, _perms(WHOLE_T, 'both'), mean=mean, normalize=normalize)


def _device(name, precision, cands=None, which='both', flags=0):
    cfg = CONFIGS[name]
    m = make_model(name, precision)
    images = synth_images(WHOLE_B, cfg, seed=WHOLE_SEED[name]).to(DEV)
    cands = [WHOLE_CANDS] * WHOLE_B if cands is None else cands
    rows = torch.from_numpy(R.candidate_rows(cands, WHOLE_T + 1, cfg.eos_id, cfg.pad_id)).to(DEV)
    masks = S.query_masks(_perms(WHOLE_T, which)).to(DEV)
    with torch.inference_mode():
        out = m.model.score(m.tokenizer, images, rows, masks, flags)
    torch.cuda.synchronize()
    return m, [t.cpu() for t in out]


def _gaps_allow(want, bound_of_terms):
    """Per crop, the adjacent pairs of the oracle's ranking whose keys are more than twice the bound apart."""
    ok, left_out = [], 0
    for b in range(WHOLE_B):
        order = want['rank'][b]
        for a, c in zip(order[:-1], order[1:]):
            sa, sc = float(want['scores'][b, a]), float(want['scores'][b, c])
            terms = max(int(want['lengths'][b, a]), int(want['lengths'][b, c])) + 1
            if sa - sc > 2 * bound_of_terms(terms):
                ok.append((b, a, c))
            else:
                left_out += 1
    return ok, left_out


def _check_against_oracle(name, precision, got, want):
    scores, order_scores, char_lp, rank, lengths, valid = got
    assert np.array_equal(lengths.numpy(), want['lengths']) and np.array_equal(valid.numpy().astype(bool), want['valid'])
    worst = 0.0
    for b in range(WHOLE_B):
        for j in range(len(WHOLE_CANDS)):
            terms = len(WHOLE_CANDS[j]) + 1
            bound = whole_bound(precision, terms)
            for k in range(2):
                err = abs(float(order_scores[b, j, k]) - float(want['order_scores'][b, j, k]))
                print(f'{name} {precision} crop {b} candidate {j} order {k}: {float(order_scores[b, j, k]):.4f} want {float(want["order_scores"][b, j, k]):.4f} |d| {err:.2e} bound {bound:.2e}')
                assert err <= bound
                worst = max(worst, err / terms)
                assert np.abs(char_lp[b, j, k, :terms].numpy() - want['char_lp'][b, j, k, :terms]).max() <= whole_bound(precision, 1)
            err = abs(float(scores[b, j]) - float(want['scores'][b, j]))
            assert err <= bound, (b, j, err, bound)
        assert sorted(rank[b].tolist()) == list(range(len(WHOLE_CANDS)))
    print(f'{name} {precision}: worst |d order score| per term {worst:.3e}')
    return worst


@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
def test_score_against_the_oracle(name, precision):
    want = _oracle(name)
    assert want['valid'].all() and want['scores'].min() > -80 and want['scores'].max() < -1
    ok, left_out = _gaps_allow(want, lambda terms: whole_bound(precision, terms))
    assert left_out == 0, 'the oracle keys of this fixture are closer than twice the bound: choose other crops'
    _, got = _device(name, precision)
    _check_against_oracle(name, precision, got, want)
    assert np.array_equal(got[3].numpy(), want['rank'])


@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_score_bf16_plan(name):
    want = _oracle(name)
    _, got = _device(name, 'bf16')
    scores, rank = got[0], got[3]
    assert torch.isfinite(scores).all()
    _check_against_oracle(name, 'bf16', got, want)
    ok, left_out = _gaps_allow(want, lambda terms: whole_bound('bf16', terms))
    print(f'{name} bf16: {left_out} adjacent pairs left out of the rank comparison')
    assert left_out <= BF16_PAIRS_LEFT_OUT[name]
    pos = [{j: i for i, j in enumerate(rank[b].tolist())} for b in range(WHOLE_B)]
    for b, a, c in ok:
        assert pos[b][a] < pos[b][c], (b, a, c)


@pytest.mark.parametrize('flags', [S.COMBINE['mean'], S.LENGTH_NORM, S.COMBINE['mean'] | S.LENGTH_NORM])
def test_score_mean_and_length_norm(flags):
    """The other combination and the other key, on the device's own order scores: the rank kernel's result inside the whole call."""
    _, got = _device('parseq-tiny', 'bf16x3', flags=flags)
    scores, order_scores, _, rank, lengths, valid = got
    want_s = R.combine(order_scores.numpy(), mean=bool(flags & 1))
    assert np.abs(scores.numpy().astype(np.float64) - want_s).max() <= 1e-5
    assert np.array_equal(rank.numpy(), R.rank(scores.numpy(), lengths.numpy(), valid.numpy(), bool(flags & 2)))


@pytest.mark.parametrize('name,precision', [('parseq-tiny', 'bf16x3'), ('parseq', 'fp32')])
def test_own_greedy_reading_scores_its_confidence(name, precision):
    """score(images, [[the greedy AR reading]], 'forward') is the log of the confidence `forward(refine_iters=0)` gives that reading."""
    cfg = CONFIGS[name]
    m = make_model(name, precision, decode_ar=True, refine_iters=0)
    images = synth_images(4, cfg, seed=21).to(DEV)
    with torch.inference_mode():
        logits = m(images, cfg.max_label_length)
        labels, conf = m.tokenizer.read(logits)
        assert all(len(s) <= cfg.max_label_length for s in labels)
        res = m.score(images, [[s] for s in labels], 'forward')
    torch.cuda.synchronize()
    assert res.valid.cpu().all() and res.lengths.cpu()[:, 0].tolist() == [len(s) for s in labels]
    for b, s in enumerate(labels):
        want, got = math.log(float(conf[b])), float(res.scores[b, 0])
        print(f'{name} {precision} crop {b} {s!r}: score {got:.5f} log confidence {want:.5f}')
        assert abs(got - want) <= whole_bound(precision, len(s) + 1)
    assert res.best()[0].cpu().tolist() == [0] * 4
    dec = m.tokenizer.decode_scores(res, [[s] for s in labels])
    assert [d[0][0] for d in dec] == labels and all(len(d[0][2]) == 1 and len(d[0][2][0]) == len(d[0][0]) + 1 for d in dec)


def test_order_scores_sum_to_the_permutation_loss(golden):
    """Single candidates = the labels of the training golden, its first two orderings: minus the sum of the order scores over the batch is
    `permutation_loss`'s per-permutation loss times its count of targets (both keep the <eos> targets in these two)."""
    from parseq_amd.system import permutation_loss
    g, meta = golden('parseq_train')
    m = make_model('parseq', 'fp32')
    images, perms = g['images'].to(DEV), g['perms'].long()[:2]
    with torch.inference_mode():
        _, per_perm, counts, _ = permutation_loss(m, images, meta['labels'], perms)
        res = m.score(images, [[s] for s in meta['labels']], perms)
    torch.cuda.synchronize()
    assert torch.equal(res.perms, perms)
    for k in range(2):
        want = float(per_perm[k]) * int(counts[k])
        got = -float(res.order_scores[:, 0, k].double().sum())
        print(f'order {k}: -sum of scores {got:.5f}, loss x count {want:.5f}')
        assert abs(got - want) <= 1e-4 * want


def test_two_streams_and_candidate_permutation():
    cfg = CONFIGS['parseq-tiny']
    m = make_model('parseq-tiny', 'bf16x3')
    images = synth_images(WHOLE_B, cfg, seed=WHOLE_SEED['parseq-tiny']).to(DEV)
    masks = S.query_masks(_perms(WHOLE_T, 'both')).to(DEV)

    def run(cands):
        rows = torch.from_numpy(R.candidate_rows(cands, WHOLE_T + 1, cfg.eos_id, cfg.pad_id)).to(DEV)
        with torch.inference_mode():
            return m.model.score(m.tokenizer, images, rows, masks, 0)
    base = run([WHOLE_CANDS] * WHOLE_B)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        other = run([WHOLE_CANDS] * WHOLE_B)
    side.synchronize()
    for a, b in zip(base, other):
        assert torch.equal(a.cpu(), b.cpu())
    shuffle = [4, 0, 5, 3, 1, 2]
    got = run([[WHOLE_CANDS[j] for j in shuffle]] * WHOLE_B)
    torch.cuda.synchronize()
    scores, rank = base[0].cpu(), base[3].cpu()
    for b in range(WHOLE_B):
        for i, j in enumerate(shuffle):
            assert abs(float(got[0][b, i]) - float(scores[b, j])) <= 1e-5 * (len(WHOLE_CANDS[j]) + 1)
        assert [shuffle[i] for i in got[3][b].cpu().tolist()] == rank[b].tolist()


def test_invalid_and_absent_rows():
    """An out-of-range token, an inner <eos>, a row without <eos> and an absent row come back valid = 0, score -inf, ranked last in index
    order; the rows beside them keep their bits."""
    cfg = CONFIGS['parseq-tiny']
    C = cfg.num_tokens - 2
    _, base = _device('parseq-tiny', 'bf16x3')
    cands = [list(WHOLE_CANDS) for _ in range(WHOLE_B)]
    cands[0][1] = [5, C + 7]          # the token of <bos> + 6: outside the classes and outside the embedding table
    cands[1][0] = [5, -3, 11]
    cands[1][4] = None                # absent
    cands[2][2] = [40, cfg.eos_id, 2]  # an inner <eos>
    m, got = _device('parseq-tiny', 'bf16x3', cands=cands)
    # a row that is full of characters, no <eos>: written by hand
    rows = R.candidate_rows(cands, WHOLE_T + 1, cfg.eos_id, cfg.pad_id)
    rows[2, 5, :] = 9
    masks = S.query_masks(_perms(WHOLE_T, 'both')).to(DEV)
    images = synth_images(WHOLE_B, cfg, seed=WHOLE_SEED['parseq-tiny']).to(DEV)
    with torch.inference_mode():
        got2 = [t.cpu() for t in m.model.score(m.tokenizer, images, torch.from_numpy(rows).to(DEV), masks, 0)]
    bad = {(0, 1), (1, 0), (1, 4), (2, 2)}
    for out, extra in ((got, set()), (got2, {(2, 5)})):
        scores, order_scores, char_lp, rank, lengths, valid = out
        for b in range(WHOLE_B):
            dead = sorted(j for (bb, j) in bad | extra if bb == b)
            for j in range(6):
                if (b, j) in bad | extra:
                    assert valid[b, j] == 0 and scores[b, j] == NEG_INF and lengths[b, j] == 0
                    assert (order_scores[b, j] == NEG_INF).all() and (char_lp[b, j] == 0).all()
                else:
                    assert valid[b, j] == 1 and torch.equal(scores[b, j], base[0][b, j]) and torch.equal(order_scores[b, j], base[1][b, j])
                    assert torch.equal(char_lp[b, j], base[2][b, j])
            assert rank[b].tolist()[6 - len(dead):] == dead
            assert [j for j in rank[b].tolist() if j not in dead] == [j for j in base[3][b].tolist() if j not in dead]


def test_refusals_leave_the_outputs_untouched():
    nat, lib = native()
    cfg = CONFIGS['parseq-tiny']
    m = make_model('parseq-tiny', 'bf16x3')
    B, N, L, K = 2, 4, 6, 2
    images = synth_images(B, cfg, seed=3).to(DEV)
    plan = m.model._plan(B * N)
    cap = m.model._native_state.plans[(nat.PARSEQ_BF16X3, 0)][1]
    assert cap == 8
    cand = torch.full((B, N, L), cfg.pad_id, dtype=torch.int32, device=DEV)
    cand[:, :, 0], cand[:, :, 1] = 5, cfg.eos_id
    masks = S.query_masks(S.parse_orders('both', L - 1)).to(DEV)
    need = lib.parseq_score_workspace_bytes(plan, B, N, L, K)
    assert need > 0
    ws = torch.empty(need + 16, dtype=torch.uint8, device=DEV)
    outs = dict(scores=torch.full((B, N), 5.0, device=DEV), order=torch.full((B, N, K), 5.0, device=DEV), lp=torch.full((B, N, K, L), 5.0, device=DEV),
                rank=torch.full((B, N), 5, dtype=torch.int32, device=DEV), lengths=torch.full((B, N), 5, dtype=torch.int32, device=DEV),
                valid=torch.full((B, N), 5, dtype=torch.uint8, device=DEV))

    def call(plan=plan, images=images, batch=B, cand=cand, n=N, steps=L, masks=masks, orders=K, flags=0, ws=ws, ws_bytes=need, drop=None):
        o = {k: (None if k == drop else v) for k, v in outs.items()}
        return lib.parseq_score(plan, nat.ptr(images), nat.dtype_code(images.dtype) if images is not None else 0, batch, nat.ptr(cand), n, steps, nat.ptr(masks),
                                orders, flags, nat.ptr(o['scores']), nat.ptr(o['order']), nat.ptr(o['lp']), nat.ptr(o['rank']), nat.ptr(o['lengths']),
                                nat.ptr(o['valid']), nat.ptr(ws), ws_bytes, nat.stream_ptr(DEV))
    refused = [dict(plan=None), dict(images=None), dict(cand=None), dict(masks=None), dict(ws=None), dict(drop='scores'), dict(drop='order'), dict(drop='rank'),
               dict(drop='lengths'), dict(drop='valid'), dict(n=0), dict(n=17), dict(orders=0), dict(orders=17), dict(batch=3, n=3), dict(steps=1),
               dict(steps=cfg.max_label_length + 2), dict(ws_bytes=need - 1), dict(ws=ws[4:]), dict(flags=4), dict(flags=-1)]
    for kw in refused:
        assert call(**kw) != 0, kw
        assert lib.parseq_last_error()
    assert lib.parseq_score_workspace_bytes(plan, 3, 3, L, K) == 0 and lib.parseq_score_workspace_bytes(plan, B, N, 1, K) == 0
    # ViTSTR and a deeper decoder
    from parseq_amd import create_model
    v = create_model('vitstr', precision='bf16x3').eval().to(DEV)
    assert call(plan=v.model._plan(8)) != 0 and b'ViTSTR' in lib.parseq_last_error()
    deep = create_model('parseq-tiny', dec_depth=2, precision='bf16x3').eval().to(DEV)
    assert call(plan=deep.model._plan(8)) != 0 and b'dec_depth' in lib.parseq_last_error()
    torch.cuda.synchronize()
    for t in outs.values():
        assert (t == 5).all()
    # batch * n == max_batch runs
    assert call() == 0
    torch.cuda.synchronize()
    assert (outs['valid'] == 1).all() and torch.isfinite(outs['scores']).all() and (outs['lengths'] == 1).all()
    with pytest.raises(ValueError, match='dec_depth'):
        deep.score(images, [['ab']] * B)
    with pytest.raises(ValueError, match='charset'):
        m.score(images, [['ab', 'aé']] * B)
