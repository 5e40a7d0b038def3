"""ViTSTR's training step (strhub/models/vitstr/system.py:75-79 -> base.py:194-204): the training encoder over 129 tokens (class
token + 128 patches, the key-streaming attention of parseq_amd/csrc/train_attn_wide.h), `parseq_train_vitstr_head` and the encoder's
backward, against a golden minted by executing the reference's own `training_step` + `loss.backward()`
(tools/make_golden_train_wide.py -> tests/golden/vitstr_train.*) and against CPU autograd through oracle/vitstr_oracle.py."""
import ctypes as C

import pytest
import torch
import torch.nn.functional as F

from oracle import vitstr_oracle as V
from oracle.make_golden_train import checksum
from oracle.synth import synth_images

CFG = V.vitstr_config()


@pytest.fixture(scope='module')
def vgold(golden):
    return golden('vitstr_train')


def _images(meta, n=None):
    imgs = synth_images(len(meta['labels']), CFG, seed=meta['image_seed'])
    return imgs if n is None else imgs[:n]


def _system(device='cuda', precision='fp32'):
    from parseq_amd import create_model
    m = create_model('vitstr', precision=precision)
    m.model.load_state_dict(V.synth_state_dict(CFG, 0))
    return m.eval().to(device)


def _cpu_step(images, labels, tokenizer, sd=None):
    """forward_logits_loss on CPU autograd: oracle forward over max_len = T - 1, cross-entropy with ignore_index = <pad>."""
    sd = {k: v.clone().requires_grad_(True) for k, v in (sd or V.synth_state_dict(CFG, 0)).items()}
    targets = tokenizer.encode(labels)[:, 1:]
    logits = V.forward(sd, CFG, images, targets.shape[1] - 1)
    loss = F.cross_entropy(logits.flatten(end_dim=1), targets.flatten(), ignore_index=tokenizer.pad_id)
    loss.backward()
    return loss.detach(), {k: v.grad for k, v in sd.items()}, sd


def _bad_grads(got, want, meta=None, g=None):
    bad = []
    for key, w in want.items():
        x = got[key].cpu()
        tol = 2e-4 * max(float(w.abs().max()), 1e-6) + 1e-7
        err = float((x - w).abs().max())
        if err > tol:
            bad.append((key, 'cpu', err, tol))
        if meta is not None:
            ref = meta['grads'][key]['norm']
            if abs(float(x.double().norm()) - ref) > 1e-3 * max(ref, 1e-6):
                bad.append((key, 'norm', float(x.double().norm()), ref))
            if 'grad.' + key in g:
                full = g['grad.' + key]
                if float((x - full).abs().max()) > 2e-4 * max(float(full.abs().max()), 1e-6) + 1e-7:
                    bad.append((key, 'golden tensor'))
    return bad


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_vitstr_golden_crops_regenerate(vgold):
    _, meta = vgold
    assert abs(checksum(_images(meta)) - meta['image_checksum']) <= 1e-9 * abs(meta['image_checksum'])


def test_oracle_training_loss_matches_reference(vgold):
    """The CPU restatement the GPU tests compare with reproduces the reference's loss and every gradient norm."""
    from parseq_amd.tokenizer import Tokenizer
    from parseq_amd.configs import CHARSET_94_FULL
    g, meta = vgold
    loss, grads, _ = _cpu_step(_images(meta), meta['labels'], Tokenizer(CHARSET_94_FULL))
    assert abs(float(loss) - meta['loss']) <= 1e-5 * meta['loss']
    assert list(grads) == list(meta['grads']) and len(grads) == 152
    for key, ref in meta['grads'].items():
        assert abs(float(grads[key].double().norm()) - ref['norm']) <= 1e-4 * max(ref['norm'], 1e-6), key


def test_vitstr_refusals_before_device_work():
    """micro_batches > 1 and a label longer than max_label_length raise ValueError before anything touches a device (the system
    lives on the CPU here)."""
    from parseq_amd.train import TrainStep, loss_and_grads
    m = _system('cpu')
    with pytest.raises(ValueError, match='micro_batches'):
        TrainStep(m, total_steps=10, micro_batches=2)
    images = torch.zeros(2, 3, 32, 128)
    with pytest.raises(ValueError, match='max_label_length'):
        loss_and_grads(m, images, ['ok', 'x' * (m.max_label_length + 1)])
    with pytest.raises(ValueError, match='permutations'):
        loss_and_grads(m, images, ['ok', 'fine'], perms=torch.zeros(1, 4, dtype=torch.long))


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('batch', [8, 3, 1])
def test_vitstr_full_step_matches_reference(vgold, batch):
    """fp32 step: loss and all 152 gradients against CPU autograd (max error 2e-4 of each tensor's largest magnitude); at the
    golden's batch of 8 also against the reference's loss, gradient norms and stored tensors.  A repeat reproduces every bit."""
    from parseq_amd.train import loss_and_grads
    g, meta = vgold
    m = _system()
    labels = meta['labels'][:batch]
    images = _images(meta, batch)
    res = loss_and_grads(m, images.cuda(), labels)
    torch.cuda.synchronize()
    want_loss, want, _ = _cpu_step(images, labels, m.tokenizer)
    assert abs(float(res.loss) - float(want_loss)) <= 1e-4 * float(want_loss)
    assert set(res.grads) == set(want) and len(res.grads) == 152
    full = batch == len(meta['labels'])
    if full:
        assert abs(float(res.loss) - meta['loss']) <= 1e-4 * meta['loss']
    bad = _bad_grads(res.grads, want, meta if full else None, g)
    assert not bad, bad
    # d memory is zero on the class token's row and past row T
    T = max(len(s) for s in labels) + 1
    assert float(res.dmemory[:, 0].abs().max()) == 0.0 and float(res.dmemory[:, T + 1:].abs().max()) == 0.0
    res2 = loss_and_grads(m, images.cuda(), labels)
    torch.cuda.synchronize()
    assert torch.equal(res.flat, res2.flat) and float(res.loss) == float(res2.loss)


@pytest.mark.gpu
def test_vitstr_bf16_step_against_fp32(vgold):
    """train_precision = 'bf16': every gradient against the fp32 step within the bounds of the PARSeq-S bf16 gates."""
    from parseq_amd.train import loss_and_grads
    _, meta = vgold
    m = _system()
    images = _images(meta).cuda()
    ref = loss_and_grads(m, images, meta['labels'])
    m.train_precision = 'bf16'
    res = loss_and_grads(m, images, meta['labels'])
    torch.cuda.synchronize()
    assert abs(float(res.loss) - float(ref.loss)) <= 5e-4 * float(ref.loss)
    rel, cos = [], []
    for key, want in ref.grads.items():
        a, b = want.cpu().double().flatten(), res.grads[key].cpu().double().flatten()
        if float(a.norm()) < 1e-7:
            continue
        rel.append((float((a - b).norm() / a.norm()), key))
        cos.append(float(a @ b / (a.norm() * b.norm())))
    rel.sort()
    print(f'vitstr bf16 step: per-tensor L2 error median {rel[len(rel) // 2][0]:.2e}, worst {rel[-1][0]:.2e} ({rel[-1][1]}), min cosine {min(cos):.5f}')
    assert 1e-5 < rel[len(rel) // 2][0] < 2e-2 and rel[-1][0] < 6e-2 and min(cos) > 0.998


@pytest.mark.gpu
def test_vitstr_training_step_backward_fills_grad(vgold):
    """`ViTSTR.training_step(batch, 0).backward()` leaves in every parameter's .grad what loss_and_grads returns."""
    from parseq_amd.train import loss_and_grads
    _, meta = vgold
    m = _system()
    images = _images(meta).cuda()
    res = loss_and_grads(m, images, meta['labels'])
    loss = m.training_step((images, meta['labels']), 0)
    assert loss.requires_grad
    loss.backward()
    torch.cuda.synchronize()
    assert float(loss) == float(res.loss)
    for key, p in m.model.named_parameters():
        assert p.grad is not None and torch.equal(p.grad, res.grads[key]), key


@pytest.mark.gpu
def test_vitstr_three_optimiser_steps_follow_torch_adamw(vgold):
    """TrainStep on ViTSTR (clipping active, AdamW with weight decay on >= 2-D non-bias tensors, OneCycle) against the same three steps
    on the CPU: autograd through the oracle, clip_grad_norm_, torch.optim.AdamW + OneCycleLR."""
    from parseq_amd.train import TrainStep
    _, meta = vgold
    m = _system()
    images, labels = _images(meta), meta['labels']
    step = TrainStep(m, total_steps=40, clip_val=1.0, weight_decay=0.01)
    lrs, got = [], []
    for _ in range(3):
        lrs.append(step.lr)
        got.append(float(step(images.cuda(), labels)))
    torch.cuda.synchronize()
    start = V.synth_state_dict(CFG, 0)
    sd = {k: v.clone().requires_grad_(True) for k, v in start.items()}
    decay = [v for k, v in sd.items() if v.ndim > 1 and not k.endswith('.bias')]
    rest = [v for k, v in sd.items() if not (v.ndim > 1 and not k.endswith('.bias'))]
    opt = torch.optim.AdamW([{'params': decay, 'weight_decay': 0.01}, {'params': rest, 'weight_decay': 0.0}], lr=step.max_lr)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, step.max_lr, 40, pct_start=m.warmup_pct, cycle_momentum=False)
    targets = m.tokenizer.encode(labels)[:, 1:]
    want, first_norm = [], None
    for i in range(3):
        assert abs(opt.param_groups[0]['lr'] - lrs[i]) <= 1e-9 * step.max_lr
        opt.zero_grad()
        logits = V.forward(sd, CFG, images, targets.shape[1] - 1)
        loss = F.cross_entropy(logits.flatten(end_dim=1), targets.flatten(), ignore_index=m.pad_id)
        loss.backward()
        norm = torch.nn.utils.clip_grad_norm_(list(sd.values()), 1.0)
        if i == 0:
            first_norm = float(norm)
            first_grads = {k: v.grad.clone() for k, v in sd.items()}
        opt.step()
        sched.step()
        want.append(float(loss.detach()))
    assert first_norm > 1.0                       # clipping was active
    assert all(abs(a - b) <= 2e-4 * b for a, b in zip(got, want)), (got, want)
    lr_sum = sum(lrs)
    bad = []
    for key, t in m.model.state_dict().items():
        d_got, d_want = t.cpu() - start[key], sd[key].detach() - start[key]
        err = (d_got - d_want).abs()
        real = first_grads[key].abs() > 1e-6
        if real.any() and (float(err[real].max()) > 0.1 * lr_sum or float(err[real].mean()) > 2e-3 * lr_sum):
            bad.append((key, float(err[real].max()), float(err[real].mean())))
        if float(d_want.abs().max()) > 0 and float(d_got.abs().max()) == 0:
            bad.append((key, 'unchanged'))
    assert not bad, (bad, lr_sum)


@pytest.mark.gpu
def test_vitstr_head_entry_refuses_a_parseq_model():
    from gpu_util import make_model, native
    _native, lib = native()
    m = make_model('parseq', 'bf16')
    nm = m.model._sync_native().model
    buf = torch.zeros(1 << 16, device='cuda')
    p = C.c_void_p(buf.data_ptr())
    rc = lib.parseq_train_vitstr_head(nm, p, p, 1, 2, 1, p, p, p, p, buf.numel() * 4, _native.stream_ptr())
    assert rc != 0 and b'PARSeq model' in lib.parseq_last_error()
