"""CPU proof that the operator tests of the training attention (tests/test_train_attn.py) can fail and need not: for every case that
runs on the GPU, a float32 emulation of the route's algorithm with its rounding points, in two different summation orders, lies inside
the derived bound of oracle/train_attn_ref.py, and every deliberate error in the reference that applies to the case — a lost key tile,
a key taken for padding, a dropout index with the padded key count, a pass reading pass 0's site or mask, shared K / V ignored, the
accumulate flag ignored either way, a pass walk that keeps the last pass, a missing scale, unrounded operands, dq summed over the
batch — lies outside it."""
import pytest
import torch

from oracle import train_attn_ref as A

CASES = A.attn_cases()


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_float32_emulation_inside_and_mutants_outside(case):
    t = A.make_inputs(case)
    want = A.reference(case, t)
    for name, (v, b) in want.items():
        assert torch.isfinite(v).all() and torch.isfinite(b).all() and (b >= 0).all(), name
    for shuffled in (False, True):
        r = A.worst_ratio(A.emulate_f32(case, t, shuffled), want)
        print(f'{case.name}: float32 emulation, {"shuffled keys and queries" if shuffled else "torch order"}: worst error / bound {r:.3f}')
        assert r <= 1.0
    for mutant in A.mutants_of(case):
        mut = {k: v for k, (v, _) in A.reference(case, t, mutant).items()}
        r = A.worst_ratio(mut, want)
        print(f'{case.name}: mutant {mutant} worst error / bound {r:.3g}')
        assert r > 1.0, f'{mutant} hides inside the bound'


def test_every_mutant_and_every_route_is_exercised():
    seen = set()
    for c in CASES:
        seen.update(A.mutants_of(c))
    assert seen == set(A.MUTANTS)
    assert {c.route for c in CASES} == set(A.ROUTES) - {'none'}
    assert {c.kt for c in CASES if c.route == 'dec_bf16'} == {2, 8}
    dec8 = [c for c in CASES if c.kt == 8]
    assert {c.pass_loop for c in dec8} == {False, True} and all(c.kv_shared and c.P > 1 for c in dec8 if c.pass_loop)
    assert {c.kv_accumulate for c in dec8} == {False, True} and {c.q_shared for c in dec8} == {False, True}
    for flag in ('kv_shared', 'kv_accumulate', 'q_shared', 'qmask', 'kmask'):
        assert {getattr(c, flag) for c in CASES} == {False, True}, flag
    assert {bool(c.dropout) for c in CASES} == {False, True}
    for route in ('dec_bf16', 'hd32', 'hd64'):      # the routes that take masks and dropout: with and without
        mine = [c for c in CASES if c.route == route]
        assert {bool(c.dropout) for c in mine} == {c.qmask for c in mine} == {False, True}, route
    assert any(c.q_shared for c in CASES if c.route == 'mfma')
    assert any(c.out16 for c in CASES if c.route == 'enc_bf16') and any(c.kv_accumulate for c in CASES if c.route == 'enc_bf16')
    assert any(c.bf16_ops for c in CASES if c.route == 'hd32')
    # a second block of 32 queries, so that dK / dV are carried across blocks
    for route in ('hd32', 'mfma', 'hd64'):
        assert any(c.Lq > 32 for c in CASES if c.route == route), route
    # the capacity edge of the VALU route: the largest key count whose backward is admitted, where the forward still has room
    edge = A.largest_backward_keys(32, 32)
    assert edge == 223 and A.admitted(32, edge, 32, True) and not A.admitted(32, edge + 1, 32, True) and A.admitted(32, 256, 32, False)
    assert not A.admitted(32, 257, 32, False)
    assert any(c.route == 'hd32' and (c.Lq, c.Lk) == (32, edge) for c in CASES)
    assert all(2 <= c.B <= 3 and 2 <= c.H <= 3 and 1 <= c.P <= 3 for c in CASES)


def test_inputs_keep_a_key_in_every_row_and_the_reference_is_autograd():
    """make_inputs asserts the kernels' precondition; and the reference's closed-form backward is float64 autograd of its forward."""
    c = next(c for c in CASES if c.kt == 8 and c.Lq > 1 and c.kv_shared and c.dropout and not (c.pass_loop or c.kv_accumulate or c.q_shared))
    t = A.make_inputs(c)
    want = A.reference(c, t)
    q = A.bf16_round(t['q']).double().requires_grad_(True)
    k = A.bf16_round(t['k']).double().requires_grad_(True)
    v = A.bf16_round(t['v']).double().requires_grad_(True)
    qh, kh, vh = A._heads(q, c, q.shape[0]), A._heads(k, c, k.shape[0]), A._heads(v, c, v.shape[0])
    s = (c.scale * (qh @ kh.transpose(-1, -2))).masked_fill(A._masked(c, t).expand(-1, -1, c.H, -1, -1), float('-inf'))
    o = A._rows((s.softmax(-1) * A._factors(c)) @ vh, c)
    o.backward(A.bf16_round(t['dO']).double())
    assert float((o.detach() - want['o'][0]).abs().max()) <= 1e-12
    # K / V are shared by the passes and q is per image in this case: autograd's dk / dv are the sums over the passes
    assert float((q.grad - want['dq'][0]).abs().max()) <= 1e-11
    for grad, name in ((k.grad, 'dk'), (v.grad, 'dv')):
        assert float((grad - want[name][0].reshape(c.P, c.B, c.Lk, c.H, c.hd).sum(0)).abs().max()) <= 1e-10, name


def test_the_exponent_constant_covers_float32_exp2():
    """E_EXP was chosen against torch's float32 exp2 / exp on the CPU: both stay below one ulp of the float64 value over the arguments a
    soft-max row produces, and E_EXP leaves room above that (its reasoning is in the oracle's docstring)."""
    a = -torch.rand(1 << 20, generator=torch.Generator().manual_seed(3)) * 60.0
    for fn, ref in ((torch.exp2, torch.exp2(a.double())), (torch.exp, torch.exp(a.double()))):
        got = fn(a).double()
        ulps = ((got - ref).abs() / (2.0 ** torch.floor(torch.log2(ref)) * 2.0 ** -23)).max()
        print(f'{fn.__name__}: worst error {float(ulps):.3f} ulp')
        assert float(ulps) <= 1.0 < A.E_EXP
