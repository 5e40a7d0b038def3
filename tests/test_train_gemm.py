"""The training step's products and row kernels ONE OPERATOR AT A TIME, through parseq_op_train_gemm / _linear / _layernorm (ABI 12).

Every case: seeded inputs; operand buffers with a NaN tail right behind the last valid element (an over-the-edge read that leaks into a
stored value shows up as NaN); outputs pre-filled with NaN and fenced by NaN guards in front and behind (rows are dense, ld = N, so a write
past a row's end lands in the next row and is judged there); all memory from torch's caching allocator; the reported route equals the route the
case was written for; every stored element within the DERIVED bound of oracle/train_gemm_ref.py (float64 reference; the bound's formula, its
constant and the proof that it bites are there and in tests/test_train_gemm_bound.py); guards untouched; a second run bit-identical.
The observed worst error / bound per kernel of one run is recorded in profiles/train_gemm_bound_ratios.md."""
import ctypes as C

import pytest
import torch

from oracle import train_gemm_ref as G

pytestmark = pytest.mark.gpu
DEV = 'cuda'
GUARD = 256          # elements in front of and behind every output (keeps 16-byte alignment for fp32 and bf16)
TAIL = 64            # NaN elements behind every operand
CASES = G.gemm_cases()
E_INVALID, E_STATE = -1, -3
RATIOS = {}          # kernel name -> worst error / bound seen (printed by the coverage test)


def _nat():
    from parseq_amd import _native
    return _native, _native.lib()


def _operand_buffer(x, kc, shadow, pad=0):
    """x [rows, K] logical -> (flat device buffer with a NaN tail, outer stride, k stride); pad: NaN elements behind every row of a k-contiguous operand"""
    rows, K = x.shape
    if pad:
        x = torch.nn.functional.pad(x, (0, pad), value=float('nan'))
        K += pad
    mem = x if kc else x.T
    flat = torch.full((mem.numel() + TAIL,), float('nan'), dtype=torch.bfloat16 if shadow else torch.float32)
    flat[:mem.numel()] = mem.contiguous().flatten().to(flat.dtype)
    return flat.to(DEV), (K if kc else 1), (1 if kc else rows)


class Fenced:
    """[guard | body | guard]: the body pre-filled with `init` (NaN unless the kernel accumulates into it)"""

    def __init__(self, shape, dtype=torch.float32, init=None, offset=0):
        n = 1
        for s in shape:
            n *= s
        self.shape, self.n, self.off = shape, n, GUARD + offset
        self.buf = torch.full((GUARD + offset + n + GUARD,), float('nan'), dtype=dtype, device=DEV)
        if init is not None:
            self.buf[self.off:self.off + n] = init.flatten().to(dtype).to(DEV)

    @property
    def ptr(self):
        return C.c_void_p(self.buf.data_ptr() + self.off * self.buf.element_size())

    def body(self):
        return self.buf[self.off:self.off + self.n].view(self.shape).cpu()

    def guards_intact(self):
        return bool(torch.isnan(self.buf[:self.off]).all()) and bool(torch.isnan(self.buf[self.off + self.n:]).all())


def _run_gemm(c, t, a16=None, b16=None, expect_rc=0, b_pad=0):
    """One call of parseq_op_train_gemm on fresh buffers -> (rc, route, outputs name -> Fenced, the scratch or None)"""
    _native, lib = _nat()
    a16 = c.a16 if a16 is None else a16
    b16 = c.b16 if b16 is None else b16
    A, sa_o, sa_k = _operand_buffer(t['A'], c.a_kc, a16)
    B, sb_o, sb_k = _operand_buffer(t['B'], c.b_kc, b16, b_pad)
    d = _native.TrainGemmDesc()
    d.A = _native.GemmOperand(A.data_ptr(), _native.PARSEQ_BF16 if a16 else _native.PARSEQ_F32, sa_o, sa_k)
    d.B = _native.GemmOperand(B.data_ptr(), _native.PARSEQ_BF16 if b16 else _native.PARSEQ_F32, sb_o, sb_k)
    d.M, d.N, d.K, d.alpha, d.accumulate, d.bf16_ops = c.M, c.N, c.K, c.alpha, int(c.accumulate), int(c.bf16_ops)
    keep, outs, scratch = [A, B], {}, None
    if c.c32:
        outs['C'] = Fenced((c.M, c.N), init=t['C_old'])
        d.C = outs['C'].ptr
    if c.c16:
        outs['c16'] = Fenced((c.M, c.N), torch.bfloat16)
        d.c16 = outs['c16'].ptr
    if c.gelu_out:
        outs['gelu_out'] = Fenced((c.M, c.N), torch.bfloat16 if c.gelu_out == 'b16' else torch.float32)
        setattr(d, 'gelu_out16' if c.gelu_out == 'b16' else 'gelu_out', outs['gelu_out'].ptr)
    if c.asum:
        outs['asum'] = Fenced((c.M,), init=t['asum_old'])
        d.asum = outs['asum'].ptr
    if c.bias:
        bias = Fenced((c.N,), init=t['bias'], offset=1 if c.bias == 2 else 0)      # offset 1: a pointer that is not 16-byte aligned
        keep.append(bias)
        d.bias = bias.ptr
    if c.rper:
        R = Fenced(tuple(t['R'].shape), init=t['R'])
        keep.append(R)
        d.R, d.ldr, d.rper = R.ptr, c.N, c.rper
    if c.gelu_pre:
        pre = Fenced((c.M, c.N), torch.bfloat16 if c.gelu_pre == 'b16' else torch.float32, init=t['pre'])
        keep.append(pre)
        setattr(d, 'gelu_pre16' if c.gelu_pre == 'b16' else 'gelu_pre', pre.ptr)
    if c.scratch:
        scratch = torch.full((c.scratch + TAIL,), float('nan'), device=DEV)
        keep.append(scratch)
        d.scratch, d.scratch_floats = scratch.data_ptr(), c.scratch
    route = _native.GemmRoute()
    rc = lib.parseq_op_train_gemm(C.byref(d), C.byref(route), _native.stream_ptr())
    torch.cuda.synchronize()
    if c.scratch:
        assert torch.isnan(scratch[c.scratch:]).all(), 'the scratch was written past its end'
    assert rc == expect_rc, (rc, lib.parseq_last_error())
    return rc, route, outs, scratch


def _bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_gemm_against_float64_within_the_derived_bound(case):
    _native, _ = _nat()
    t = G.make_inputs(case)
    want = G.expected(case, t)
    _, route, outs, _ = _run_gemm(case, t)
    kernel = _native.GEMM_KERNELS[route.kernel]
    splits, k_chunk = case.plan()
    print(f'{case.name}: kernel {kernel} whole {route.whole} splits {route.splits} k_chunk {route.k_chunk} folded {route.folded_asum}{route.folded_gelu_pre}{route.folded_gelu_out}')
    assert (kernel, bool(route.whole), route.splits, route.k_chunk) == (case.kernel, case.whole, splits, k_chunk), 'not the route this case was written for'
    assert bool(route.folded_asum) == bool(route.folded_gelu_pre) == bool(route.folded_gelu_out) == case.rounded
    got = {k: f.body() for k, f in outs.items()}
    assert set(got) == set(want)
    for name, (v, b) in want.items():
        err = (got[name].double() - v).abs()
        nan = int(torch.isnan(got[name].float()).sum())
        ratio = float((err / b.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max())
        idx = int((err / b.clamp_min(1e-300)).nan_to_num(nan=float('inf')).flatten().argmax())
        print(f'  {name}: worst error / bound {ratio:.4f} at flat index {idx} (max |err| {float(err.nan_to_num().max()):.3e}, NaN {nan})')
        RATIOS[kernel] = max(RATIOS.get(kernel, 0.0), ratio)
        assert nan == 0 and ratio <= 1.0, f'{name}: error / bound {ratio} at flat index {idx}, {nan} NaN'
        assert outs[name].guards_intact(), f'{name}: a guard was written'
    # a second run on fresh buffers: bit-identical
    _, _, outs2, _ = _run_gemm(case, t)
    for name in outs:
        assert torch.equal(_bits(outs[name].body()), _bits(outs2[name].body())), f'{name}: two runs differ'
    # the claim above gemm_plan(): a shadow is the same product as its fp32 copy in memory, bit for bit, where the split is the same
    if case.a16 or case.b16:
        _, r32, outs32, _ = _run_gemm(case, t, a16=False, b16=False)
        same_plan = (r32.splits, r32.k_chunk) == (route.splits, route.k_chunk)
        print(f'  fp32 copies in memory: kernel {_native.GEMM_KERNELS[r32.kernel]} splits {r32.splits} k_chunk {r32.k_chunk} -> {"compared" if same_plan else "different split, not compared"}')
        assert _native.GEMM_KERNELS[r32.kernel].startswith('bf16_')
        if same_plan:
            for name in outs:
                if name != 'asum' or not case.a16:      # row sums of a shadow A are sums of other values (rounded) than those of its fp32 copy
                    assert torch.equal(_bits(outs[name].body()), _bits(outs32[name].body())), f'{name}: shadow and fp32 copy differ'


def test_the_cases_reach_every_kernel_form():
    """The parametrization as a whole: every kernel of the route report, split and unsplit, whole and not where both forms exist
    (by construction here; each case's own test holds the device's report to it)."""
    _native, _ = _nat()
    assert tuple(_native.GEMM_KERNELS) == tuple(G.KERNELS)
    for k in G.KERNELS:
        mine = [c for c in CASES if c.kernel == k]
        assert mine, k
        assert {c.plan()[0] > 1 for c in mine} == ({False} if k == 'valu' else {False, True}), k
        if k in G.HAS_WHOLE:
            assert {c.whole for c in mine} == {False, True}, k
    for k, r in sorted(RATIOS.items()):
        print(f'worst error / bound  {k:10s} {r:.4f}')


REFUSALS = [
    ('shadow-outside-bf16-mode', dict(b16=True, bf16_ops=False), E_STATE),
    ('shadow-rows-not-16-bytes', dict(b16=True, bf16_ops=True, K=96, b_stride_pad=4), E_INVALID),
    ('shadow-A-k-contiguous-B-fp32', dict(a16=True, bf16_ops=True), E_INVALID),
    ('row-sums-of-k-contiguous-shadows', dict(a16=True, b16=True, bf16_ops=True, asum=True), E_INVALID),
    ('shadow-M-below-16', dict(b16=True, bf16_ops=True, M=8), E_STATE),
    ('shadow-N-below-16', dict(b16=True, bf16_ops=True, N=8), E_STATE),
    ('no-output', dict(bf16_ops=True, c32=False), E_INVALID),
]


@pytest.mark.parametrize('name,kw,code', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_gemm_refusals_leave_every_output_untouched(name, kw, code):
    _, lib = _nat()
    kw = dict(kw)
    pad = kw.pop('b_stride_pad', 0)      # rows of K + 4 bf16: not a multiple of 16 bytes
    case = G.GemmCase(name=name, kernel='valu', **{**dict(M=128, N=128, K=128, bias=1, gelu_out='f32' if kw.get('c32', True) else '',
                                                          c16=kw.get('b16', False) and not kw.get('asum', False)), **kw})
    t = G.make_inputs(case)
    if case.asum:
        t['asum_old'] = torch.full((case.M,), float('nan'))      # the row sums are accumulated into: NaN here so that "untouched" is "all NaN" for every output
    rc, route, outs, scratch = _run_gemm(case, t, expect_rc=code, b_pad=pad)
    print(f'{name}: rc {rc} ({lib.parseq_last_error().decode()})')
    assert rc == code and route.kernel == -1
    assert (not outs) == (name == 'no-output')      # that case has no output buffer to look at: for it the scratch is the witness
    for k, f in outs.items():
        assert torch.isnan(f.buf).all(), f'{k} was written by a refused call'
    assert torch.isnan(scratch).all(), 'the scratch was written by a refused call'


# ---- lin_fwd / lin_bwd -----------------------------------------------------------------------------------------------
# (M, N, K) of the four model families: PARSeq-Ti (E = 192), PARSeq-S (384), ViTSTR-S / PARSeq-patch16-224 (384, more tokens), the 95-class head;
# r_*: whether the route of that product rounds its operands to bf16 in the bf16-operand mode (what the test's float64 reference then does too)
LINEAR = [
    # name, M, N, K, bf16_ops, rper, gelu, dx, (rounded y, dW, dx)
    ('tiny-head-f32', 208, 95, 192, False, 0, False, True, (False, False, False)),
    ('tiny-head-bf16-padded', 416, 95, 192, True, 0, False, True, (True, True, True)),
    ('tiny-head-bf16-padded-M-not-32', 208, 95, 192, True, 0, False, True, (True, False, True)),   # dW contracts over M: 208 % 32 != 0 sends that product to the VALU kernel, unrounded
    ('head-bf16-unpadded-M', 130, 95, 384, True, 0, False, True, (True, False, False)),        # M % 4 != 0: no padded copies, dy rows not 16-byte -> VALU
    ('head-f32-two-stage-colsum', 2600, 95, 384, False, 0, False, True, (False, False, False)),
    ('head-bf16-padded-two-stage-colsum', 2912, 95, 384, True, 0, False, True, (True, True, True)),
    ('fc1-bf16-gelu', 1024, 1536, 384, True, 0, True, True, (True, True, True)),
    ('fc1-f32-gelu', 1024, 1536, 384, False, 0, True, False, (False, False, False)),           # dx NULL
    ('fc2-bf16-dx-gelu-pre', 1024, 384, 1536, True, 1024, True, True, (True, True, True)),
    ('fc2-f32-dx-gelu-pre', 640, 192, 768, False, 26, True, True, (False, False, False)),
    ('qkv-f32-colsum-two-stage', 2304, 1152, 384, False, 0, False, True, (False, False, False)),
    ('tiny-proj-bf16-resid', 3328, 192, 192, True, 26, False, True, (True, True, True)),
]


def _lin_call(x, W, bias, R, rper, dy, dW0, db0, pre, M, N, K, bf16_ops, want_gelu, want_dx):
    _native, lib = _nat()
    p = _native.ptr
    dev = lambda v: None if v is None else torch.cat([v.flatten(), torch.full((TAIL,), float('nan'))]).to(DEV)      # noqa: E731
    xd, Wd, bd, Rd, dyd, pred = dev(x), dev(W), dev(bias), dev(R), dev(dy), dev(pre)
    scratch = torch.full((G.STEP_SCRATCH + TAIL,), float('nan'), device=DEV)
    y, act = Fenced((M, N)), Fenced((M, N)) if want_gelu else None
    _native.check(lib.parseq_op_train_linear(p(xd), p(Wd), p(bd), p(Rd), rper, y.ptr, act.ptr if act else None, None, None, None, None, None,
                                             M, N, K, 0, int(bf16_ops), p(scratch), G.STEP_SCRATCH, _native.stream_ptr()))
    dW, db, dx = Fenced((N, K), init=dW0), Fenced((N,), init=db0), Fenced((M, K)) if want_dx else None
    _native.check(lib.parseq_op_train_linear(p(xd), p(Wd), None, None, 0, None, None, p(dyd), dW.ptr, db.ptr, dx.ptr if dx else None,
                                             p(pred) if (pre is not None and want_dx) else None, M, N, K, 1, int(bf16_ops), p(scratch), G.STEP_SCRATCH, _native.stream_ptr()))
    torch.cuda.synchronize()
    assert torch.isnan(scratch[G.STEP_SCRATCH:]).all()
    outs = {'y': y, 'dW': dW, 'db': db}
    if act:
        outs['gelu'] = act
    if dx:
        outs['dx'] = dx
    return outs


@pytest.mark.parametrize('name,M,N,K,bf16_ops,rper,gelu,want_dx,rounded', LINEAR, ids=[r[0] for r in LINEAR])
def test_linear_forward_backward_against_float64_autograd(name, M, N, K, bf16_ops, rper, gelu, want_dx, rounded):
    g = torch.Generator().manual_seed(len(name) * 1000 + M)
    x, W = G._operand(g, M, K, False), G._operand(g, N, K, False) / K ** 0.5
    bias, dy = torch.randn(N, generator=g), G._operand(g, M, N, False)
    R = torch.randn(rper, N, generator=g) if rper else None
    dW0, db0 = torch.randn(N, K, generator=g) * M ** 0.5, torch.randn(N, generator=g) * M ** 0.5
    pre = torch.randn(M, K, generator=g) * 1.5 if gelu else None          # the pre-activation of the layer below (dx's GELU backward)
    outs = _lin_call(x, W, bias, R, rper, dy, dW0, db0, pre, M, N, K, bf16_ops, gelu, want_dx)
    rd = lambda v, on: G.bf16_round(v.double()) if on else v.double()      # noqa: E731
    u, c = G.U, G.C_TREE
    # y = x W^T + b + R by float64 autograd on the operands as the route rounds them; the gradients by autograd of that
    x64, W64 = rd(x, rounded[0]).requires_grad_(True), rd(W, rounded[0]).requires_grad_(True)
    b64 = bias.double().requires_grad_(True)
    Rrows = R.double()[torch.arange(M) % rper] if rper else 0.0
    y64 = x64 @ W64.T + b64 + Rrows
    S = x64.detach().abs() @ W64.detach().abs().T + bias.double().abs() + (Rrows.abs() if rper else 0.0)
    by = c * (K + G.E_EPI) * u * S
    want = {'y': (y64.detach(), by)}
    if gelu:
        want['gelu'] = (G.gelu64(y64.detach()), G.GELU_LIP * by + c * G.E_GELU * u * y64.detach().abs())
    # backward: each product on its own route's operands (autograd of y = x W^T + b at those operands)
    xw, dyw = rd(x, rounded[1]), rd(dy, rounded[1])
    xg = xw.clone().requires_grad_(True)
    Wg = torch.zeros(N, K, dtype=torch.float64, requires_grad=True)
    bg = torch.zeros(N, dtype=torch.float64, requires_grad=True)
    (gW,) = torch.autograd.grad(xg @ Wg.T + bg, (Wg,), dyw)
    want['dW'] = (dW0.double() + gW, c * (M + G.E_EPI) * u * (dyw.abs().T @ xw.abs() + dW0.double().abs()))
    (gb,) = torch.autograd.grad((xg @ Wg.T + bg), (bg,), dy.double())      # the bias gradient sums the UNROUNDED dy on every route
    want['db'] = (db0.double() + gb, c * (M + 1) * u * (dy.double().abs().sum(0) + db0.double().abs()))
    if want_dx:
        Wx, dyx = rd(W, rounded[2]), rd(dy, rounded[2])
        xg2 = torch.zeros(M, K, dtype=torch.float64, requires_grad=True)
        (gx,) = torch.autograd.grad(xg2 @ Wx.T, (xg2,), dyx)
        Sx = dyx.abs() @ Wx.abs()
        bx = c * (N + 32 + G.E_EPI) * u * Sx                                  # N + 32: the padded head contracts over N rounded up to 32 (zeros)
        if gelu:
            gp = G.gelu_grad64(pre.double())
            gx, bx = gx * gp, c * u * ((N + 32 + G.E_EPI + 1) * Sx * gp.abs() + G.E_GELU * Sx)
        want['dx'] = (gx, bx)
    assert set(want) == set(outs)
    for k, (v, b) in want.items():
        got = outs[k].body().double()
        ratio = float(((got - v).abs() / b.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max())
        print(f'{name}: {k} worst error / bound {ratio:.4f}')
        assert ratio <= 1.0 and outs[k].guards_intact(), (k, ratio)
    outs2 = _lin_call(x, W, bias, R, rper, dy, dW0, db0, pre, M, N, K, bf16_ops, gelu, want_dx)
    for k in outs:
        assert torch.equal(_bits(outs[k].body()), _bits(outs2[k].body())), f'{k}: two runs differ'


# ---- train_ln_fwd / ln_bwd -------------------------------------------------------------------------------------------
def _ln_scratch_floats(rows, E, two_stage):
    """The least scratch ln_bwd takes: the chunk partials [chunks][2 E] at its END plus 64 E floats; the two-stage fold of the partials
    (2048 chunks and more) puts its 64 x 2 E intermediate sums at the START and runs only where those fit in front of the partials.
    Both are passed EXACTLY, so the partials end on the scratch's last float and the fold's sums end where the partials begin."""
    return -(-rows // G.LNB_ROWS) * 2 * E + (128 if two_stage else 64) * E


@pytest.mark.parametrize('E', [192, 384, 768])
@pytest.mark.parametrize('rows', [1, 3, 4, 5, 1000, 2048 * G.LNB_ROWS + 7])
@pytest.mark.parametrize('riders', [False, True], ids=['plain', 'add-dx16'])
def test_layernorm_forward_backward_against_float64_autograd(E, rows, riders):
    _native, lib = _nat()
    p = _native.ptr
    g = torch.Generator().manual_seed(E * 7 + rows)
    x = torch.randn(rows, E, generator=g) * 2 + (30.0 if riders else 0.0)      # with the riders: a row mean far from zero
    gamma, beta = torch.randn(E, generator=g), torch.randn(E, generator=g)
    dy = torch.randn(rows, E, generator=g)
    dy[-1] *= 64.0      # the last row (alone in its chunk of four, or nearly) outweighs the bound of the sums over all rows: losing it shows
    add = torch.randn(rows, E, generator=g) if riders else None
    dg0, db0 = torch.randn(E, generator=g) * rows ** 0.5, torch.randn(E, generator=g) * rows ** 0.5
    want = G.layernorm_reference(x, gamma, beta, 1e-5, dy, add, dg0, db0)
    dev = lambda v: None if v is None else torch.cat([v.flatten(), torch.full((TAIL,), float('nan'))]).to(DEV)      # noqa: E731
    xd, gd, bd, dyd, addd = dev(x), dev(gamma), dev(beta), dev(dy), dev(add)
    n_scr = _ln_scratch_floats(rows, E, two_stage=not riders)      # with the riders the one-stage fold runs at every row count
    scratch = torch.full((n_scr + TAIL,), float('nan'), device=DEV)

    def run():
        o = {'y': Fenced((rows, E)), 'y16': Fenced((rows, E), torch.bfloat16), 'dx': Fenced((rows, E)), 'dgamma': Fenced((E,), init=dg0), 'dbeta': Fenced((E,), init=db0)}
        if riders:
            o['dx16'] = Fenced((rows, E), torch.bfloat16)
        for key, code in (('y', _native.PARSEQ_F32), ('y16', _native.PARSEQ_BF16)):
            _native.check(lib.parseq_op_train_layernorm(p(xd), p(gd), p(bd), o[key].ptr, code, None, None, None, None, None, None, rows, E, 1e-5, 0, None, 0, _native.stream_ptr()))
        _native.check(lib.parseq_op_train_layernorm(p(xd), p(gd), None, None, 0, p(dyd), p(addd), o['dx'].ptr, o['dx16'].ptr if riders else None, o['dgamma'].ptr, o['dbeta'].ptr,
                                                    rows, E, 1e-5, 1, p(scratch), n_scr, _native.stream_ptr()))
        torch.cuda.synchronize()
        return o
    o = run()
    assert torch.isnan(scratch[n_scr:]).all(), 'the scratch was written past its end'
    want['y16'] = (want['y'][0], want['y'][1] + 2.0 ** -8 * want['y'][0].abs())
    if riders:
        want['dx16'] = (want['dx'][0], want['dx'][1] + 2.0 ** -8 * want['dx'][0].abs())
    assert set(want) == set(o)
    for k, (v, b) in want.items():
        ratio = float(((o[k].body().double() - v).abs() / b.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max())
        print(f'layernorm E={E} rows={rows}: {k} worst error / bound {ratio:.4f}')
        assert ratio <= 1.0 and o[k].guards_intact(), (k, ratio)
    # the bf16 outputs are the roundings of the fp32 ones
    assert torch.equal(o['y16'].body(), o['y'].body().to(torch.bfloat16))
    if riders:
        assert torch.equal(o['dx16'].body(), o['dx'].body().to(torch.bfloat16))
    o2 = run()
    for k in o:
        assert torch.equal(_bits(o[k].body()), _bits(o2[k].body())), f'{k}: two runs differ'


def test_layernorm_backward_refuses_a_scratch_that_is_too_small():
    _native, lib = _nat()
    p = _native.ptr
    rows, E = 1000, 384
    x, w, dy = torch.randn(rows, E, device=DEV), torch.randn(E, device=DEV), torch.randn(rows, E, device=DEV)
    n_scr = 250 * 2 * E + 64 * E - 1          # one float short of the chunk partials + the fold's 64 E
    scratch = torch.full((n_scr + TAIL,), float('nan'), device=DEV)
    dx, dg, db = Fenced((rows, E)), Fenced((E,)), Fenced((E,))
    for scr, n in ((scratch, n_scr), (None, 1 << 24)):
        rc = lib.parseq_op_train_layernorm(p(x), p(w), None, None, 0, p(dy), None, dx.ptr, None, dg.ptr, db.ptr, rows, E, 1e-5, 1, p(scr), n, _native.stream_ptr())
        torch.cuda.synchronize()
        assert rc == E_INVALID, rc
    for f in (dx, dg, db):
        assert torch.isnan(f.buf).all()
    assert torch.isnan(scratch).all()


# ---- exports that had one or two sizes: parseq_grad_norm, parseq_cross_entropy, parseq_adamw_step ---------------------
@pytest.mark.parametrize('n', [1, 255, 1024, 1025, 3 * (1 << 20) + 3])
@pytest.mark.parametrize('tail', ['gaussian', 'heavy-tail'])
def test_grad_norm_sizes(n, tail):
    """heavy-tail: the last three elements (the ones past the last whole block of 256, and past the last multiple of four) carry a
    third or more of the sum of squares, so a reduction that stops short of them is far outside the bound at every n."""
    _native, lib = _nat()
    g = torch.randn(n, generator=torch.Generator().manual_seed(n)) * 3
    if tail == 'heavy-tail':
        g[-3:] = torch.tensor([2000.0, -2500.0, 3000.0])[-min(n, 3):]
    gd = torch.cat([g, torch.full((TAIL,), float('nan'))]).to(DEV)
    out, ws = Fenced((1,)), Fenced((1024,))
    _native.check(lib.parseq_grad_norm(_native.ptr(gd), n, out.ptr, ws.ptr, _native.stream_ptr()))
    torch.cuda.synchronize()
    want = float(g.double().norm())
    err, bound = abs(float(out.body()) - want), G.grad_norm_bound(n, want)
    print(f'grad_norm n={n} {tail}: error / bound {err / bound:.4f} (relative error {err / want:.3e})')
    assert err <= bound and out.guards_intact() and ws.guards_intact()


@pytest.mark.parametrize('rows', [1, 40, 4099])
@pytest.mark.parametrize('ignored', ['none', 'all', 'all-but-last'])
def test_cross_entropy_rows_and_ignored_targets(rows, ignored):
    """all-but-last: the mean is the last row's loss alone, so a last row that is lost (4099 = 4 * 1024 + 3) shows in the value; in the
    mean of 4099 rows one row is 1e-3 of the loss and would not."""
    _native, lib = _nat()
    gen = torch.Generator().manual_seed(rows)
    lg = torch.randn(rows, 95, generator=gen) * 3
    tg = torch.randint(0, 95, (rows,), generator=gen)
    if ignored != 'none':
        tg[:rows if ignored == 'all' else rows - 1] = 96
    count = int((tg != 96).sum())
    lgd = torch.cat([lg.flatten(), torch.full((TAIL,), float('nan'))]).to(DEV)
    loss, ws = Fenced((1,)), Fenced((rows,))
    numel = torch.full((3,), -7, dtype=torch.int32, device=DEV)
    _native.check(lib.parseq_cross_entropy(_native.ptr(lgd), _native.ptr(tg.to(torch.int32).to(DEV)), rows, 95, 96, loss.ptr, C.c_void_p(numel.data_ptr() + 4),
                                           ws.ptr, _native.stream_ptr()))
    torch.cuda.synchronize()
    assert numel.tolist() == [-7, count, -7] and loss.guards_intact() and ws.guards_intact()
    if count == 0:
        assert torch.isnan(loss.body()).all()          # 0 / 0, as torch.nn.functional.cross_entropy gives
        return
    want = float(torch.nn.functional.cross_entropy(lg.double(), tg, ignore_index=96))
    # a row: 95 exponentials (2 u each) summed (95 u, all positive), the logarithm of that sum (absolute 97 u + its own rounding), the
    # maximum added and the target's logit subtracted (u of each intermediate, all below 2 max|logit| + log 95); then the mean of `count`
    # positive terms: relative (count + 1) u
    big = 2 * float(lg.abs().max()) + 4.6
    bound = G.C_TREE * G.U * ((95 + 4) + 4 * big + (count + 1) * want)
    err = abs(float(loss.body()) - want)
    print(f'cross_entropy rows={rows} {ignored}: error / bound {err / bound:.4f} (loss {want:.4f})')
    assert err <= bound


@pytest.mark.parametrize('clip', ['no-clip-scalar', 'clip-active', 'clip-inactive'])
def test_adamw_step_on_parseq_tiny_against_float64(clip):
    """One parseq_adamw_step on parseq-tiny's master weights against float64 AdamW (oracle.train_gemm_ref.adamw_reference, which the CPU
    test holds to torch.optim.AdamW): step 3 of a run with moments that are not zero, weight decay 0.1 on a mixed set of tensors whose
    flags change every one or two tensors (so the flat buffer goes out in many launches and every boundary between two of them is a
    boundary between a decayed and an undecayed tensor), without the clip scalar, with one that scales the gradient to a quarter and
    with one above which the norm stays (coefficient exactly 1)."""
    from gpu_util import make_model
    _native, lib = _nat()
    system = make_model('parseq-tiny', 'fp32')
    native = system.model._sync_native().model
    n, count = lib.parseq_model_grad_elems(native), lib.parseq_model_num_params(native)
    table = []
    for i in range(count):
        key, numel = C.c_char_p(), C.c_int64()
        _native.check(lib.parseq_model_param_info(native, i, C.byref(key), C.byref(numel)))
        table.append((key.value.decode(), numel.value, lib.parseq_model_param_offset(native, i)))
    assert all(off + k <= n for _, k, off in table)
    sd = system.model.state_dict()
    _, g, m0, v0, flags, decay = G.adamw_inputs([k for _, k, _ in table], seed=5)
    p0 = torch.cat([sd[key].detach().float().cpu().flatten() for key, _, _ in table])      # the weights the model was made with
    idx = torch.cat([torch.arange(off, off + k) for _, k, off in table])                   # where each tensor lies in the flat buffers

    def flat(x, fill=0.0):      # between two tensors (alignment padding, if any) the gradient and the moments are zero, as in a training step
        f = torch.full((n,), fill)
        f[idx] = x
        return f
    gd = torch.cat([flat(g), torch.full((TAIL,), float('nan'))]).to(DEV)
    md, vd = Fenced((n,), init=flat(m0)), Fenced((n,), init=flat(v0))
    norm = float(g.double().norm())
    max_norm = {'no-clip-scalar': 0.0, 'clip-active': norm / 4, 'clip-inactive': norm * 2}[clip]
    normd = Fenced((1,), init=torch.tensor([norm]))
    hp = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, step=3)
    _native.check(lib.parseq_adamw_step(native, _native.ptr(gd), md.ptr, vd.ptr, (C.c_int32 * count)(*flags), hp['lr'], hp['beta1'], hp['beta2'], hp['eps'],
                                        hp['weight_decay'], hp['step'], None if clip == 'no-clip-scalar' else normd.ptr, max_norm, _native.stream_ptr()))
    torch.cuda.synchronize()
    pd = torch.full((len(idx) + TAIL,), float('nan'), device=DEV)
    at = 0
    for key, k, _ in table:
        _native.check(lib.parseq_model_get_param(native, key.encode(), C.c_void_p(pd.data_ptr() + 4 * at), k, _native.stream_ptr()))
        at += k
    torch.cuda.synchronize()
    want = G.adamw_reference(p0, g, m0, v0, decay, norm=None if clip == 'no-clip-scalar' else float(normd.body()), max_norm=max_norm, **hp)
    got = {'p': pd[:len(idx)].cpu(), 'm': md.body()[idx], 'v': vd.body()[idx]}
    assert md.guards_intact() and vd.guards_intact() and normd.guards_intact() and torch.isnan(pd[len(idx):]).all()
    for name, (val, b) in want.items():
        err = (got[name].double() - val).abs()
        ratio = float((err / b.clamp_min(1e-300)).nan_to_num(nan=float('inf')).max())
        print(f'adamw {clip}: {name} worst error / bound {ratio:.4f} (max |err| {float(err.nan_to_num().max()):.3e})')
        assert ratio <= 1.0, (name, ratio)
