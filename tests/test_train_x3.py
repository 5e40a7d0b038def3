"""train_precision = 'bf16x3' on the device: the split-bf16 products of the training step (train_gemm.h mfma_x3gemm_kernel) one operator
at a time through parseq_op_train_gemm / parseq_op_train_linear, and whole steps against the goldens and the library's own fp32 mode.

Operator level: the harness of tests/test_train_gemm.py (NaN tails behind operands, NaN-filled outputs between NaN guards, the route
report) with the two references and derived bounds of tests/train_x3_reference.py — every stored element within bound (1) of the split
formula AND within bound (2) of the unsplit float64 product; tests/test_train_x3_bound.py proves on the CPU that both can fail.
Step level: the gates the fp32 mode is held to."""
import ctypes as C

import pytest
import torch

import train_x3_reference as X
from oracle import train_gemm_ref as G
from test_train_gemm import E_INVALID, E_STATE, LINEAR, _bits, _lin_call, _nat, _run_gemm

pytestmark = pytest.mark.gpu
DEV = 'cuda'
CASES = X.x3_cases()


def _check(tag, outs, want):
    """every output within both bounds, no NaN, guards intact -> the worst ratios"""
    assert set(outs) == set(want)
    worst = [0.0, 0.0]
    for name, refs in want.items():
        got = outs[name].body()
        nan = int(torch.isnan(got.float()).sum())
        for i, (which, (v, b)) in enumerate(zip(('split', 'full'), refs)):
            q = ((got.double() - v).abs() / b.clamp_min(1e-300)).nan_to_num(nan=float('inf'))
            ratio, idx = float(q.max()), int(q.flatten().argmax())
            print(f'  {tag} {name} against {which}: worst error / bound {ratio:.4f} at flat index {idx} (NaN {nan})')
            worst[i] = max(worst[i], ratio)
            assert nan == 0 and ratio <= 1.0, f'{tag} {name} against {which}: error / bound {ratio} at flat index {idx}, {nan} NaN'
        assert outs[name].guards_intact(), f'{tag} {name}: a guard was written'
    return worst


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_x3_gemm_within_both_derived_bounds(case):
    _native, _ = _nat()
    t = G.make_inputs(case)
    want = X.expected(case, t)
    _, route, outs, _ = _run_gemm(case, t)
    kernel = _native.GEMM_KERNELS_X3.get(route.kernel, route.kernel)
    splits, k_chunk = case.plan()
    print(f'{case.name}: kernel {kernel} splits {route.splits} k_chunk {route.k_chunk} folded {route.folded_asum}{route.folded_gelu_pre}{route.folded_gelu_out}')
    assert (kernel, route.whole, route.splits, route.k_chunk) == (case.kernel, 0, splits, k_chunk), 'not the route this case was written for'
    assert route.folded_asum and route.folded_gelu_pre and route.folded_gelu_out
    _check(case.name, outs, want)
    _, _, outs2, _ = _run_gemm(case, t)          # a second run on fresh buffers: bit-identical
    for name in outs:
        assert torch.equal(_bits(outs[name].body()), _bits(outs2[name].body())), f'{name}: two runs differ'


def test_x3_cases_split_as_the_bf16_mode_does():
    """same gemm_plan: a case's splits and k_chunk are those of the bf16-operand mode for the same product"""
    from dataclasses import replace
    for c in CASES:
        assert c.plan() == replace(c, kernel='bf16_kk', bf16_ops=True).plan()
    assert {c.plan()[0] for c in CASES if c.K == 1472} == {1, 10}


REFUSALS = [
    ('shadow-B', dict(b16=True, bf16_ops=X.X3), E_STATE),
    ('c16', dict(c16=True, bf16_ops=X.X3), E_STATE),
    ('gelu_out16', dict(gelu_out='b16', bf16_ops=X.X3), E_STATE),
    ('mode-2', dict(bf16_ops=2), E_INVALID),
]


@pytest.mark.parametrize('name,kw,code', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_x3_refusals_leave_every_output_untouched(name, kw, code):
    _, lib = _nat()
    case = G.GemmCase(name=name, kernel='valu', **{**dict(M=128, N=128, K=128, bias=1, gelu_out='f32'), **kw})
    t = G.make_inputs(case)
    rc, route, outs, scratch = _run_gemm(case, t, expect_rc=code)
    print(f'{name}: rc {rc} ({lib.parseq_last_error().decode()})')
    assert rc == code and route.kernel == -1 and outs
    for k, f in outs.items():
        assert torch.isnan(f.buf).all(), f'{k} was written by a refused call'
    assert torch.isnan(scratch).all(), 'the scratch was written by a refused call'


FALLBACKS = [
    ('K-40-not-a-stage', dict(M=144, N=80, K=40, bias=1), 0, 'valu'),
    ('K-48-whole-tiles', dict(M=128, N=128, K=48, bias=1), 0, 'mfma_f32'),
    ('unaligned-operand', dict(M=144, N=80, K=64, bias=1), 1, 'valu'),          # rows of B 65 floats apart
    ('no-scratch', dict(M=144, N=80, K=1472, scratch=0), 0, 'valu'),
]


@pytest.mark.parametrize('name,kw,b_pad,kernel', FALLBACKS, ids=[r[0] for r in FALLBACKS])
def test_x3_fallbacks_are_the_fp32_mode_bit_for_bit(name, kw, b_pad, kernel):
    _native, _ = _nat()
    runs = []
    for mode in (X.X3, 0):
        case = G.GemmCase(name=name, kernel=kernel, bf16_ops=mode, **kw)
        _, route, outs, _ = _run_gemm(case, G.make_inputs(case), b_pad=b_pad)
        assert _native.GEMM_KERNELS[route.kernel] == kernel and not route.folded_asum
        runs.append((route, outs))
    (r3, o3), (r0, o0) = runs
    assert (r3.kernel, r3.splits, r3.k_chunk) == (r0.kernel, r0.splits, r0.k_chunk)
    assert torch.equal(_bits(o3['C'].body()), _bits(o0['C'].body())) and not torch.isnan(o3['C'].body()).any() and o3['C'].guards_intact()


X3_LINEAR = [r for r in LINEAR if r[0] in ('tiny-head-bf16-padded', 'head-bf16-padded-two-stage-colsum', 'tiny-proj-bf16-resid', 'fc1-bf16-gelu', 'fc2-bf16-dx-gelu-pre')]


@pytest.mark.parametrize('name,M,N,K,_mode,rper,gelu,want_dx,_rounded', X3_LINEAR, ids=[r[0].replace('bf16', 'x3') for r in X3_LINEAR])
def test_x3_linear_forward_backward_within_both_bounds(name, M, N, K, _mode, rper, gelu, want_dx, _rounded):
    """lin_fwd / lin_bwd in the bf16x3 mode at the LINEAR shapes of tests/test_train_gemm.py whose products all qualify: PARSeq-Ti's
    projection, the 95-class head through its zero-padded copies (Ti and S), fc1 / fc2 with the GELU riders.  Same inputs as there."""
    assert len(X3_LINEAR) == 5
    g = torch.Generator().manual_seed(len(name) * 1000 + M)
    x, W = G._operand(g, M, K, False), G._operand(g, N, K, False) / K ** 0.5
    bias, dy = torch.randn(N, generator=g), G._operand(g, M, N, False)
    R = torch.randn(rper, N, generator=g) if rper else None
    dW0, db0 = torch.randn(N, K, generator=g) * M ** 0.5, torch.randn(N, generator=g) * M ** 0.5
    pre = torch.randn(M, K, generator=g) * 1.5 if gelu else None
    outs = _lin_call(x, W, bias, R, rper, dy, dW0, db0, pre, M, N, K, X.X3, gelu, want_dx)
    want = X.linear_expected(x, W, bias, R, rper, dy, dW0, db0, pre, gelu, want_dx)
    _check(name, outs, want)
    # float64 autograd of the unsplit Linear, for comparison: y and dW
    y64 = x.double() @ W.double().T + bias.double() + (R.double()[torch.arange(M) % rper] if rper else 0.0)
    print(f'  {name}: y against float64 autograd max |err| {float((outs["y"].body().double() - y64).abs().max()):.3e} of max |y| {float(y64.abs().max()):.3e}')
    outs2 = _lin_call(x, W, bias, R, rper, dy, dW0, db0, pre, M, N, K, X.X3, gelu, want_dx)
    for k in outs:
        assert torch.equal(_bits(outs[k].body()), _bits(outs2[k].body())), f'{k}: two runs differ'


@pytest.mark.parametrize('N,K', [(1152, 384), (384, 384), (1536, 384), (384, 1536)])
def test_a_batch_8_step_reaches_the_x3_kernels(N, K):
    """The Linear products of a batch-8 PARSeq-S step (M = 8 * 128 rows), forward orientation, at the step's own scratch: an x3 kernel"""
    _native, lib = _nat()
    M = 1024
    A, B = torch.randn(M * K, device=DEV), torch.randn(N * K, device=DEV)
    Cout, scratch = torch.empty(M * N, device=DEV), torch.empty(G.STEP_SCRATCH, device=DEV)
    d = _native.TrainGemmDesc()
    d.A = _native.GemmOperand(A.data_ptr(), _native.PARSEQ_F32, K, 1)
    d.B = _native.GemmOperand(B.data_ptr(), _native.PARSEQ_F32, K, 1)
    d.M, d.N, d.K, d.alpha, d.bf16_ops, d.C = M, N, K, 1.0, X.X3, Cout.data_ptr()
    d.scratch, d.scratch_floats = scratch.data_ptr(), G.STEP_SCRATCH
    route = _native.GemmRoute()
    _native.check(lib.parseq_op_train_gemm(C.byref(d), C.byref(route), _native.stream_ptr()))
    torch.cuda.synchronize()
    assert _native.GEMM_KERNELS_X3[route.kernel] == 'x3_kk'
    want = A.view(M, K).double() @ B.view(N, K).double().T
    assert float((Cout.view(M, N).double() - want).abs().max()) <= 1e-4 * float(want.abs().max())


# ---- step level ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def train_golden(golden):
    return golden('parseq_train')


@pytest.fixture(scope='module')
def cpu_step(train_golden):
    """the exact fp32 step of the parseq_train golden on the CPU oracle: memory and all 175 gradients"""
    from oracle import decoder_backward as DB, encoder_backward as EB, parseq_oracle as O
    from oracle.synth import CONFIGS, synth_state_dict
    from parseq_amd.tokenizer import Tokenizer
    torch.set_num_threads(8)
    g, meta = train_golden
    cfg = CONFIGS['parseq']
    sd = synth_state_dict(cfg, 0)
    with torch.no_grad():
        memory, saved = EB.forward(sd, cfg, g['images'])
        _, _, want, dmem = DB.loss_and_grads(sd, cfg, memory, Tokenizer(X.CHARSET_94).encode(meta['labels']), g['perms'].long(), O.attn_masks_from_perm)
        want.update(EB.backward(sd, cfg, saved, dmem))
    return memory, want


def _gate(got, want):
    """the fp32 mode's per-tensor gate: max-abs error <= 2e-4 max|want| + 1e-7 -> [(key, error / gate)] worst first"""
    r = []
    for key, w in want.items():
        w = w.cpu()
        r.append((float((got[key].cpu() - w).abs().max()) / (2e-4 * max(float(w.abs().max()), 1e-6) + 1e-7), key))
    return sorted(r, reverse=True)


def test_x3_full_step_meets_the_fp32_gates(train_golden, cpu_step):
    """The gates of test_full_step_gradients_match_reference, in the bf16x3 mode: loss within 1e-4, memory within 2e-4 (the fp32 test
    allows 1e-4 of its own exact products), all 175 gradients within 2e-4 max|want| + 1e-7 of the hand-derived CPU backward and their
    norms within 1e-3 of the reference's; the stored golden tensors whole.  A repeat reproduces every bit."""
    from gpu_util import make_model
    from parseq_amd.train import loss_and_grads
    g, meta = train_golden
    memory, want = cpu_step
    m = make_model('parseq', 'bf16')
    m.train_precision = 'bf16x3'
    perms = g['perms'].long()
    res = loss_and_grads(m, g['images'].to(DEV), meta['labels'], perms)
    torch.cuda.synchronize()
    mem_err = float((res.memory.cpu() - memory).abs().max())
    ratios = _gate(res.grads, want)
    print(f'bf16x3 step: loss {float(res.loss):.7f} against {meta["loss"]:.7f}; memory max-abs {mem_err:.2e}; worst error / gate ' +
          ', '.join(f'{k} {r:.3f}' for r, k in ratios[:5]))
    for r, k in ratios:
        print(f'  error / gate {r:.4f} {k}')
    assert mem_err <= 2e-4
    assert abs(float(res.loss) - meta['loss']) <= 1e-4 * meta['loss']
    assert set(res.grads) == set(meta['grads']) and len(res.grads) == 175
    assert ratios[0][0] <= 1.0, ratios[:5]
    for key, ref in meta['grads'].items():
        got = res.grads[key].cpu()
        assert abs(float(got.double().norm()) - ref['norm']) <= 1e-3 * max(ref['norm'], 1e-6), key
        if 'grad.' + key in g:
            assert (got - g['grad.' + key]).abs().max() <= 2e-4 * max(float(want[key].abs().max()), 1e-6) + 1e-7, key
    res2 = loss_and_grads(m, g['images'].to(DEV), meta['labels'], perms)
    torch.cuda.synchronize()
    assert torch.equal(res.flat, res2.flat) and float(res.loss) == float(res2.loss)


def test_x3_vitstr_step_meets_the_fp32_gates(golden):
    from parseq_amd.train import loss_and_grads
    from test_train_vitstr import _bad_grads, _cpu_step, _images, _system
    g, meta = golden('vitstr_train')
    m = _system()
    m.train_precision = 'bf16x3'
    images = _images(meta)
    res = loss_and_grads(m, images.cuda(), meta['labels'])
    torch.cuda.synchronize()
    want_loss, want, _ = _cpu_step(images, meta['labels'], m.tokenizer)
    assert abs(float(res.loss) - float(want_loss)) <= 1e-4 * float(want_loss) and abs(float(res.loss) - meta['loss']) <= 1e-4 * meta['loss']
    assert set(res.grads) == set(want) and len(res.grads) == 152
    print('bf16x3 ViTSTR step: worst error / gate ' + ', '.join(f'{k} {r:.3f}' for r, k in _gate(res.grads, want)[:3]))
    bad = _bad_grads(res.grads, want, meta, g)
    assert not bad, bad


def test_x3_patch16_step_meets_the_fp32_gates(golden):
    from oracle import parseq_oracle as O
    from oracle.synth import CONFIGS, synth_state_dict
    from test_train_wide import _p16_images, _p16_step
    g, meta = golden('parseq-patch16-224_train')
    cfg = CONFIGS['parseq-patch16-224']
    m, res = _p16_step('bf16x3', meta, g)
    assert abs(float(res.loss) - meta['loss']) <= 1e-4 * meta['loss']
    sd = {k: v.clone().requires_grad_(True) for k, v in synth_state_dict(cfg, 0).items()}
    O.training_loss(sd, cfg, _p16_images(meta), m.tokenizer.encode(meta['labels']), g['perms'].long())[0].backward()
    assert set(res.grads) == set(meta['grads']) and len(res.grads) == 175
    ratios = _gate(res.grads, {k: v.grad for k, v in sd.items()})
    print('bf16x3 patch16-224 step: worst error / gate ' + ', '.join(f'{k} {r:.3f}' for r, k in ratios[:3]))
    assert ratios[0][0] <= 1.0, ratios[:5]
    for key, ref in meta['grads'].items():
        got = res.grads[key].cpu()
        assert abs(float(got.double().norm()) - ref['norm']) <= 1e-3 * max(ref['norm'], 1e-6), key
        if 'grad.' + key in g:
            full = g['grad.' + key]
            assert float((got - full).abs().max()) <= 2e-4 * max(float(full.abs().max()), 1e-6) + 1e-7, key


def test_x3_with_dropout_against_the_fp32_mode_with_the_same_masks(train_golden):
    """dropout 0.1, one seed: the masks are counters of (seed, site, element), so both modes drop the same elements"""
    from gpu_util import make_model
    from parseq_amd.train import loss_and_grads
    g, meta = train_golden
    m = make_model('parseq', 'bf16')
    images, perms, seed = g['images'].to(DEV), g['perms'].long(), 0x0FEDCBA987654321
    ref = loss_and_grads(m, images, meta['labels'], perms, dropout=0.1, seed=seed)
    m.train_precision = 'bf16x3'
    res = loss_and_grads(m, images, meta['labels'], perms, dropout=0.1, seed=seed)
    torch.cuda.synchronize()
    ratios = _gate(res.grads, ref.grads)
    print(f'bf16x3 with dropout: loss {float(res.loss):.7f} against {float(ref.loss):.7f}; worst error / gate ' + ', '.join(f'{k} {r:.3f}' for r, k in ratios[:3]))
    assert abs(float(res.loss) - float(ref.loss)) <= 1e-4 * float(ref.loss)
    assert not torch.equal(res.flat, ref.flat) and ratios[0][0] <= 1.0, ratios[:5]


def test_three_x3_updates_follow_three_fp32_updates(train_golden):
    """TrainStep three times in each mode from the same start, under the gates of test_three_optimiser_steps_follow_torch_adamw: losses
    within 2e-4 relative; the weights' movement, where the first gradient is above the noise floor, within 0.1 of the summed learning
    rates at worst and 2e-3 of it in the mean."""
    from gpu_util import make_model
    from oracle.synth import CONFIGS, synth_state_dict
    from parseq_amd.train import TrainStep, loss_and_grads
    g, meta = train_golden
    perms, images = g['perms'].long(), g['images'].to(DEV)
    first = {k: v.cpu() for k, v in loss_and_grads(make_model('parseq', 'bf16'), images, meta['labels'], perms).grads.items()}
    clip = min(1.0, 5.0 / float(torch.cat([v.flatten() for v in first.values()]).double().norm()))
    runs = {}
    for mode in ('fp32', 'bf16x3'):
        m = make_model('parseq', 'bf16')
        m.train_precision = mode
        step = TrainStep(m, total_steps=40, clip_val=5.0, weight_decay=0.01)
        lrs, losses = [], []
        for _ in range(3):
            lrs.append(step.lr)
            losses.append(float(step(images, meta['labels'], perms)))
        torch.cuda.synchronize()
        runs[mode] = (losses, {k: v.cpu() for k, v in m.model.state_dict().items()}, sum(lrs))
    (l32, w32, lr_sum), (l3, w3, _) = runs['fp32'], runs['bf16x3']
    print(f'losses fp32 {l32} bf16x3 {l3}')
    assert all(abs(a - b) <= 2e-4 * b for a, b in zip(l3, l32)) and l3[2] < l3[0]
    start = synth_state_dict(CONFIGS['parseq'], 0)
    bad = []
    for key, t in w3.items():
        err = (t - w32[key]).abs()
        real = (first[key] * clip).abs() > 1e-6
        if real.any() and (float(err[real].max()) > 0.1 * lr_sum or float(err[real].mean()) > 2e-3 * lr_sum):
            bad.append((key, float(err[real].max()), float(err[real].mean())))
        if float((w32[key] - start[key]).abs().max()) > 0 and float((t - start[key]).abs().max()) == 0:
            bad.append((key, 'unchanged'))
    assert not bad, (bad, lr_sum)


def test_mode_switching_and_workspace_sizes(train_golden):
    """One model fp32 -> bf16x3 -> bf16 -> fp32: the first and the last result are the same bits; the workspaces of the bf16x3 mode are
    the fp32 mode's, byte for byte."""
    from gpu_util import make_model
    from parseq_amd.train import loss_and_grads
    _native, lib = _nat()
    g, meta = train_golden
    m = make_model('parseq', 'bf16')
    images, perms = g['images'].to(DEV), g['perms'].long()
    res = {}
    for i, mode in enumerate(('fp32', 'bf16x3', 'bf16', 'fp32')):
        m.train_precision = mode
        r = loss_and_grads(m, images, meta['labels'], perms)
        torch.cuda.synchronize()
        res[i] = (float(r.loss), r.flat.clone())
    assert res[0][0] == res[3][0] and torch.equal(res[0][1], res[3][1])
    assert not torch.equal(res[0][1], res[1][1]) and not torch.equal(res[1][1], res[2][1])
    native = m.model._sync_native().model
    sizes = {}
    for mode in (_native.PARSEQ_F32, _native.PARSEQ_BF16X3):
        _native.check(lib.parseq_model_set_train_precision(native, mode))
        sizes[mode] = [lib.parseq_train_encoder_workspace_bytes(native, B) for B in (2, 8, 384)] + \
                      [lib.parseq_train_decoder_workspace_bytes(native, B, 26, 6) for B in (2, 8, 384)]
    assert sizes[_native.PARSEQ_F32] == sizes[_native.PARSEQ_BF16X3] and all(s > 0 for s in sizes[_native.PARSEQ_F32])
    assert lib.parseq_model_set_train_precision(native, 2) == E_INVALID
    _native.check(lib.parseq_model_set_train_precision(native, _native.PARSEQ_F32))
