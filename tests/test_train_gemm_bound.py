"""CPU proof that the operator tests of the training products (tests/test_train_gemm.py) can fail and need not: for every case that
runs on the GPU, float32 evaluations of the product in two different summation orders lie inside the derived bound of
oracle/train_gemm_ref.py, and every deliberate error in the reference — a dropped part of the contraction, a row written from its
neighbour, operands not rounded / rounded twice, the residual's wrap-around ignored, the old C not added, row sums taken from rounded
values — lies outside it."""
import pytest
import torch

from oracle import train_gemm_ref as G

CASES = G.gemm_cases()


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_float32_inside_and_mutants_outside(case):
    torch.set_num_threads(8)
    t = G.make_inputs(case)
    want = G.expected(case, t)
    for shuffled in (False, True):
        r = G.worst_ratio(G.emulate_f32(case, t, shuffled), want)
        print(f'{case.name}: float32 {"shuffled chunks" if shuffled else "torch order"} worst error / bound {r:.3f}')
        assert r <= 1.0
    for mutant in G.mutants_of(case):
        mut = {k: v for k, (v, _) in G.expected(case, t, mutant).items()}
        r = G.worst_ratio(mut, want)
        print(f'{case.name}: mutant {mutant} worst error / bound {r:.3g}')
        assert r > 1.0, f'{mutant} hides inside the bound'


def test_every_mutant_and_every_kernel_is_exercised():
    seen = set()
    for c in CASES:
        seen.update(G.mutants_of(c))
    assert seen == {'drop_chunk', 'last_row', 'not_rounded', 'rounded_twice', 'rper_ignored', 'no_accumulate', 'asum_rounded'}
    assert {c.kernel for c in CASES} == set(G.KERNELS)
    for k in G.KERNELS:
        assert {c.plan()[0] > 1 for c in CASES if c.kernel == k} == ({False} if k == 'valu' else {False, True}), k
    for k in G.HAS_WHOLE:
        assert {c.whole for c in CASES if c.kernel == k} == {False, True}, k


@pytest.mark.parametrize('E', [192, 384, 768])
@pytest.mark.parametrize('rows', [1, 3, 4, 5, 1000, 2048 * G.LNB_ROWS + 7])
@pytest.mark.parametrize('riders', [False, True], ids=['plain', 'add-dx16'])
def test_layernorm_bound_holds_float32_and_bites(E, rows, riders):
    """the shapes, seeds and inputs of the GPU test: with the riders an `add` and a row mean far from zero, without them neither"""
    torch.set_num_threads(8)
    g = torch.Generator().manual_seed(E * 7 + rows)
    x = torch.randn(rows, E, generator=g) * 2 + (30.0 if riders else 0.0)
    gamma, beta = torch.randn(E, generator=g), torch.randn(E, generator=g)
    dy = torch.randn(rows, E, generator=g)
    dy[-1] *= 64.0      # the last row (alone in its chunk of four, or nearly) outweighs the bound of the sums over all rows: losing it shows
    add = torch.randn(rows, E, generator=g) if riders else None
    dg0, db0 = torch.randn(E, generator=g) * rows ** 0.5, torch.randn(E, generator=g) * rows ** 0.5
    want = G.layernorm_reference(x, gamma, beta, 1e-5, dy, add, dg0, db0)
    xr = x.clone().requires_grad_(True)
    gr, br = gamma.clone().requires_grad_(True), beta.clone().requires_grad_(True)
    y = torch.nn.functional.layer_norm(xr, (E,), gr, br, 1e-5)
    dx, dg, db = torch.autograd.grad(y, (xr, gr, br), dy)
    got = {'y': y.detach(), 'dx': dx + add if riders else dx, 'dgamma': dg0 + dg, 'dbeta': db0 + db}
    r = G.worst_ratio(got, want)
    print(f'layernorm E={E} rows={rows}: float32 autograd worst error / bound {r:.3f}')
    assert r <= 1.0
    # mutants: the last row's gradient left out of the affine sums; the old dgamma overwritten; the variance divided by E - 1; `add` forgotten
    xs = x.double()
    y_short = (xs - xs.mean(1, keepdim=True)) / torch.sqrt(xs.var(1, unbiased=True, keepdim=True) + 1e-5) * gamma.double() + beta.double()
    mutants = [('last_row_dropped', dict(got, dbeta=got['dbeta'] - dy[-1])), ('overwritten', dict(got, dgamma=dg))]
    # (with a row mean of 30 the forward's bound carries the cancellation in x - mean and is wider than 1 / 2E: that mutant is for the plain rows)
    mutants.append(('add_forgotten', dict(got, dx=dx)) if riders else ('variance_over_E_minus_1', dict(got, y=y_short)))
    for name, mut in mutants:
        assert G.worst_ratio(mut, want) > 1.0, name


# ---- the optimiser step and the gradient norm ---------------------------------------------------------------------------
HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, step=3)


def _adamw_f32(p, g, m, v, decay, lr, beta1, beta2, eps, weight_decay, step, norm=None, max_norm=0.0):
    f = lambda x: torch.tensor(x, dtype=torch.float32)      # noqa: E731
    grad = g * torch.minimum(f(max_norm) / (f(norm) + f(1e-6)), f(1.0)) if norm is not None else g
    p1 = p * (1.0 - f(lr) * torch.where(decay, f(weight_decay), f(0.0)))
    mi = m + (grad - m) * (1.0 - f(beta1))
    vi = v * f(beta2) + (1.0 - f(beta2)) * grad * grad
    bc1, bc2s = 1.0 - f(beta1) ** step, torch.sqrt(1.0 - f(beta2) ** step)
    return {'p': p1 - (f(lr) / bc1) * (mi / (vi.sqrt() / bc2s + f(eps))), 'm': mi, 'v': vi}


@pytest.mark.parametrize('clip', ['no-clip-scalar', 'clip-active', 'clip-inactive'])
def test_adamw_reference_is_torch_adamw_and_its_bound_bites(clip):
    numels = [192 * 192, 192, 192, 95 * 192, 95, 1, 4 * 192 * 192, 768]
    p, g, m, v, flags, decay = G.adamw_inputs(numels, seed=5)
    norm = G._f32(float(g.double().norm()))
    max_norm = {'no-clip-scalar': 0.0, 'clip-active': norm / 4, 'clip-inactive': norm * 2}[clip]
    kw = dict(HP, norm=None if clip == 'no-clip-scalar' else norm, max_norm=max_norm)
    want = G.adamw_reference(p, g, m, v, decay, **kw)
    # torch.optim.AdamW in float64 from the same state, the hyper-parameters as the floats that cross the ABI
    hp = {k: G._f32(x) for k, x in HP.items() if k != 'step'}
    ps = [t.clone().requires_grad_(True) for t in p.double().split(numels)]
    groups = [{'params': [t for t, f in zip(ps, flags) if f == on], 'weight_decay': hp['weight_decay'] if on else 0.0} for on in (1, 0)]
    opt = torch.optim.AdamW(groups, lr=hp['lr'], betas=(hp['beta1'], hp['beta2']), eps=hp['eps'])
    coef = 1.0 if clip == 'no-clip-scalar' else min(G._f32(max_norm) / (norm + G._f32(1e-6)), 1.0)
    for t, gi, mi, vi in zip(ps, g.double().split(numels), m.double().split(numels), v.double().split(numels)):
        t.grad = gi * coef
        opt.state[t] = {'step': torch.tensor(float(HP['step'] - 1)), 'exp_avg': mi.clone(), 'exp_avg_sq': vi.clone()}
    opt.step()
    torch_p = torch.cat([t.detach() for t in ps])
    assert float((torch_p - want['p'][0]).abs().max()) <= 1e-13
    assert float((torch.cat([opt.state[t]['exp_avg_sq'] for t in ps]) - want['v'][0]).abs().max()) <= 1e-15
    r = G.worst_ratio(_adamw_f32(p, g, m, v, decay, **kw), want)
    print(f'adamw {clip}: float32 worst error / bound {r:.3f}')
    assert r <= 1.0
    mutants = ['no_decay', 'decay_everywhere', 'no_bias_correction'] + (['no_clip'] if clip == 'clip-active' else [])
    for mutant in mutants:
        mut = {k: val for k, (val, _) in G.adamw_reference(p, g, m, v, decay, mutant=mutant, **kw).items()}
        r = G.worst_ratio(mut, want)
        print(f'adamw {clip}: mutant {mutant} worst error / bound {r:.3g}')
        assert r > 1.0, mutant


@pytest.mark.parametrize('n', [1, 255, 1024, 1025, 3 * (1 << 20) + 3])
def test_grad_norm_bound_holds_float32_and_sees_a_lost_tail(n):
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
    g[-3:] = torch.tensor([2000.0, -2500.0, 3000.0])[-min(n, 3):]
    want = float(g.double().norm())
    bound = G.grad_norm_bound(n, want)
    parts = torch.stack([(c * c).sum() for c in g.split(-(-n // 1024))]).sum().sqrt()      # 1024 partial sums in float32, then their sum
    assert abs(float(g.norm()) - want) <= bound and abs(float(parts) - want) <= bound
    assert abs(float(g[:-1].double().norm()) - want) > bound      # one element short
    if n > 256 and n % 256:
        assert abs(float(g[:n // 256 * 256].double().norm()) - want) > bound      # the part past the last whole block of 256 lost
