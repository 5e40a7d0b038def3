"""Training past 128 encoder tokens: the key-streaming encoder attention (parseq_amd/csrc/train_attn_wide.h) and the full training
step of PARSeq-patch16-224 (196 tokens) against golden vectors minted by executing the reference's own `training_step` +
`loss.backward()` (tools/make_golden_train_wide.py)."""
import ctypes as C
import math

import pytest
import torch

from oracle import parseq_oracle as O
from oracle.make_golden_train import checksum
from oracle.synth import CONFIGS, synth_images, synth_state_dict

WIDE_TOKENS = [129, 130, 144, 196, 256]


@pytest.fixture(scope='module')
def p16_golden(golden):
    return golden('parseq-patch16-224_train')


def _p16_images(meta):
    return synth_images(len(meta['labels']), CONFIGS['parseq-patch16-224'], seed=meta['image_seed'])


def test_patch16_golden_crops_regenerate(p16_golden):
    """The golden stores the crops' seed, not the crops: they must come back bit for bit."""
    _, meta = p16_golden
    assert abs(checksum(_p16_images(meta)) - meta['image_checksum']) <= 1e-9 * abs(meta['image_checksum'])


def test_patch16_golden_covers_every_parameter(p16_golden):
    g, meta = p16_golden
    sd = synth_state_dict(CONFIGS['parseq-patch16-224'], 0)
    assert list(meta['grads']) == list(sd) and len(sd) == 175
    assert sd['encoder.pos_embed'].shape[1] == 196
    for key in meta['grads']:
        if 'grad.' + key in g:
            assert abs(float(g['grad.' + key].double().norm()) - meta['grads'][key]['norm']) <= 1e-6 * max(meta['grads'][key]['norm'], 1e-6)


# ---- the kernels on their own ------------------------------------------------------------------------------------------------------
def _attention(qkv, o, lse, d_o, dqkv, dsum, B, N, H, backward):
    from gpu_util import native
    _native, lib = native()
    route = C.c_int(-1)
    p = lambda t: C.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    _native.check(lib.parseq_op_train_attention(p(qkv), p(o), p(lse), p(d_o), p(dqkv), p(dsum), B, N, H, 1 if backward else 0,
                                                C.byref(route), _native.stream_ptr()))
    return route.value


def _run_attention(qkv, d_o, B, N, H):
    E = 64 * H
    o = torch.full((B * N, E), float('nan'), device='cuda')
    lse = torch.full((B, H, N), float('nan'), device='cuda')
    dsum = torch.full((B, H, N), float('nan'), device='cuda')
    dqkv = torch.full((B * N, 3 * E), float('nan'), device='cuda')
    r_f = _attention(qkv, o, lse, None, None, None, B, N, H, False)
    r_b = _attention(qkv, o, lse, d_o, dqkv, dsum, B, N, H, True)
    torch.cuda.synchronize()
    assert r_f == r_b
    return r_f, o, lse, dqkv, dsum


def _want(qkv, d_o, B, N, H):
    """The encoder's attention (timm Attention, scale 1/8) in float64 autograd on the CPU."""
    x = qkv.detach().cpu().double().view(B, N, 3, H, 64).permute(2, 0, 3, 1, 4).clone().requires_grad_(True)
    q, k, v = x[0], x[1], x[2]
    s = (q @ k.transpose(-2, -1)) / 8.0
    o = (s.softmax(-1) @ v).transpose(1, 2).reshape(B * N, H * 64)
    o.backward(d_o.cpu().double())
    dqkv = x.grad.permute(1, 3, 0, 2, 4).reshape(B * N, 3 * H * 64)
    return o.detach(), torch.logsumexp(s.detach(), -1), dqkv


def _rel_err(got, want):
    return float((got.cpu().double() - want).abs().max() / want.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize('H', [3, 6])
@pytest.mark.parametrize('N', WIDE_TOKENS)
def test_wide_attention_forward_backward_against_autograd(N, H):
    """O, the log-sum-exp and dQ / dK / dV of the key-streaming kernels for N in (128, 256] — multiples of 32, of 16 and neither —
    within 1e-5 of each output's largest magnitude of a float64 autograd reference, and bit-identical over two runs."""
    B = 2
    gen = torch.Generator().manual_seed(1000 * N + H)
    qkv = (torch.randn(B * N, 3 * 64 * H, generator=gen) * 1.5).cuda()
    d_o = torch.randn(B * N, 64 * H, generator=gen).cuda()
    route, o, lse, dqkv, dsum = _run_attention(qkv, d_o, B, N, H)
    assert route == 1
    want_o, want_lse, want_dqkv = _want(qkv, d_o, B, N, H)
    E = 64 * H
    assert _rel_err(o, want_o) <= 1e-5
    assert _rel_err(lse, want_lse) <= 1e-5
    for name, sl in (('dq', slice(0, E)), ('dk', slice(E, 2 * E)), ('dv', slice(2 * E, 3 * E))):
        err = _rel_err(dqkv[:, sl], want_dqkv[:, sl])
        assert err <= 1e-5, (name, err)
    want_dsum = (d_o.cpu().double() * want_o).view(B, N, H, 64).sum(-1).permute(0, 2, 1)
    assert _rel_err(dsum, want_dsum) <= 1e-5
    _, o2, lse2, dqkv2, dsum2 = _run_attention(qkv, d_o, B, N, H)
    assert torch.equal(o, o2) and torch.equal(lse, lse2) and torch.equal(dqkv, dqkv2) and torch.equal(dsum, dsum2)


@pytest.mark.gpu
@pytest.mark.parametrize('N', [64, 96, 128])
def test_shapes_up_to_128_tokens_keep_their_kernels(N):
    """At 128 tokens or fewer the step's resident kernels run (route 0) and neither statistics slot is touched."""
    B, H = 2, 6
    gen = torch.Generator().manual_seed(N)
    qkv = torch.randn(B * N, 3 * 64 * H, generator=gen).cuda()
    d_o = torch.randn(B * N, 64 * H, generator=gen).cuda()
    route, o, lse, dqkv, dsum = _run_attention(qkv, d_o, B, N, H)
    assert route == 0
    assert torch.isnan(lse).all() and torch.isnan(dsum).all()
    want_o, _, want_dqkv = _want(qkv, d_o, B, N, H)
    assert _rel_err(o, want_o) <= 1e-5 and _rel_err(dqkv, want_dqkv) <= 1e-5


@pytest.mark.gpu
def test_shapes_past_256_tokens_are_refused():
    """The key-streaming kernels stop at 256 tokens; past that the dispatch still refuses with a message, and nothing is written."""
    from gpu_util import native
    _native, lib = native()
    B, N, H = 1, 260, 3
    qkv = torch.zeros(B * N, 3 * 64 * H, device='cuda')
    o = torch.full((B * N, 64 * H), 7.0, device='cuda')
    lse = torch.zeros(B, H, N, device='cuda')
    route = C.c_int(-1)
    rc = lib.parseq_op_train_attention(C.c_void_p(qkv.data_ptr()), C.c_void_p(o.data_ptr()), C.c_void_p(lse.data_ptr()), None, None, None,
                                       B, N, H, 0, C.byref(route), _native.stream_ptr())
    torch.cuda.synchronize()
    assert rc != 0 and route.value == 0
    assert b'do not fit' in lib.parseq_last_error()
    assert bool((o == 7.0).all())


# ---- PARSeq-patch16-224: the whole training step -------------------------------------------------------------------------------
def _p16_step(precision, meta, g):
    from gpu_util import DEV, make_model
    from parseq_amd.train import loss_and_grads
    m = make_model('parseq-patch16-224', 'bf16')            # the step computes in its training precision whatever the inference precision is
    m.train_precision = precision
    res = loss_and_grads(m, _p16_images(meta).to(DEV), meta['labels'], g['perms'].long())
    torch.cuda.synchronize()
    return m, res


@pytest.mark.gpu
def test_patch16_full_step_matches_reference(p16_golden):
    """Encoder forward (196 tokens) -> decoder forward / backward -> encoder backward in fp32: the loss and the gradient of all 175
    parameters against the reference's `training_step` + `loss.backward()` (norms of every tensor, the stored tensors whole) and
    every tensor against CPU autograd through the oracle."""
    g, meta = p16_golden
    cfg = CONFIGS['parseq-patch16-224']
    m, res = _p16_step('fp32', meta, g)
    assert abs(float(res.loss) - meta['loss']) <= 1e-4 * meta['loss']
    sd = {k: v.clone().requires_grad_(True) for k, v in synth_state_dict(cfg, 0).items()}
    loss = O.training_loss(sd, cfg, _p16_images(meta), m.tokenizer.encode(meta['labels']), g['perms'].long())[0]
    loss.backward()
    assert abs(float(loss.detach()) - meta['loss']) <= 1e-4 * meta['loss']
    assert set(res.grads) == set(meta['grads']) and len(res.grads) == 175
    bad = []
    for key, ref in meta['grads'].items():
        got, want = res.grads[key].cpu(), sd[key].grad
        tol = 2e-4 * max(float(want.abs().max()), 1e-6) + 1e-7
        err = float((got - want).abs().max())
        norm = float(got.double().norm())
        if err > tol or abs(norm - ref['norm']) > 1e-3 * max(ref['norm'], 1e-6):
            bad.append((key, err, tol, norm, ref['norm']))
        if 'grad.' + key in g:
            full = g['grad.' + key]
            if float((got - full).abs().max()) > 2e-4 * max(float(full.abs().max()), 1e-6) + 1e-7:
                bad.append((key, 'golden tensor'))
    assert not bad, bad
    # a repeat of the step reproduces every bit
    _, res2 = _p16_step('fp32', meta, g)
    assert torch.equal(res.flat, res2.flat) and float(res.loss) == float(res2.loss)


@pytest.mark.gpu
def test_patch16_bf16_step_against_fp32(p16_golden):
    """train_precision = 'bf16' (the encoder's products take bf16 operands around the fp32 key-streaming attention): every gradient
    against the fp32 step within the bounds of the PARSeq-S bf16 gates."""
    g, meta = p16_golden
    _, ref = _p16_step('fp32', meta, g)
    _, res = _p16_step('bf16', meta, g)
    assert abs(float(res.loss) - float(ref.loss)) <= 5e-4 * float(ref.loss)
    rel, cos = [], []
    for key, want in ref.grads.items():
        a, b = want.cpu().double().flatten(), res.grads[key].cpu().double().flatten()
        if float(a.norm()) < 1e-7:
            continue
        rel.append((float((a - b).norm() / a.norm()), key))
        cos.append(float(a @ b / (a.norm() * b.norm())))
    rel.sort()
    print(f'patch16-224 bf16 step: per-tensor L2 error median {rel[len(rel) // 2][0]:.2e}, worst {rel[-1][0]:.2e} ({rel[-1][1]}), '
          f'min cosine {min(cos):.5f}')
    assert rel[len(rel) // 2][0] < 2e-2 and rel[-1][0] < 6e-2 and min(cos) > 0.998
    assert rel[len(rel) // 2][0] > 1e-5        # visibly not the fp32 path
    assert all(math.isfinite(float(v)) for v in (res.loss,))
