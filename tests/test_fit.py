"""The training loop on the device (parseq_amd/fit.py, train.py) and the entries it adds to the library: uint8 crops into the training
encoder, the weight-averaging kernel, real gradient accumulation, and `fit` itself — against the hand-written loop, end to end with
SWA and checkpoints, resumed, and from the command line."""
import importlib.util
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from oracle.synth import CONFIGS, synth_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SEED = 11
# batch 8 scales the rate by 8 / 256 (base.py:98-101): this makes the scaled peak the reference's own 7e-4
LR = 7e-4 * 256 / 8


def _tool(name):
    spec = importlib.util.spec_from_file_location(f'parseq_tool_{name}', os.path.join(ROOT, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _tiny(**kw):
    from gpu_util import DEV
    from parseq_amd import create_model
    m = create_model('parseq-tiny', batch_size=8, lr=LR, **kw)
    m.model.load_state_dict(synth_state_dict(CONFIGS['parseq-tiny'], 0))
    return m.eval().to(DEV)                                     # evaluation mode (dropout 0) until `fit` or the test switches training on


@pytest.fixture(scope='module')
def folders(tmp_path_factory):
    """32 training and 16 validation words, rendered once."""
    root = tmp_path_factory.mktemp('words')
    make = _tool('make_text_dataset')
    make.write_dataset(str(root / 'data' / 'train'), 32, seed=0)
    make.write_dataset(str(root / 'data' / 'val'), 16, seed=1)
    return root


def _sets(folders, system):
    from parseq_amd.data import LabelledFolder
    hp = system.hparams
    return (LabelledFolder(str(folders / 'data' / 'train'), hp.charset_train, hp.max_label_length),
            LabelledFolder(str(folders / 'data' / 'val'), hp.charset_train, hp.max_label_length))


# ---- uint8 training input -----------------------------------------------------------------------------------------------------------
def _train_memory(system, images, table='torch'):
    """The training encoder's `memory` for fp32 images (the plain entry) or uint8 images (the _ex entry with the torch-built table, or
    with table=None the library's own IEEE expression)."""
    from parseq_amd import _native
    from parseq_amd.train import _set_train_precision, is_vitstr, u8_normalise_table
    lib = _native.lib()
    model = system.model
    native = model._sync_native().model
    _set_train_precision(system, native)
    B = images.shape[0]
    tokens = (model.pos_embed if is_vitstr(system) else model.encoder.pos_embed).shape[1]
    ws_bytes = lib.parseq_train_encoder_workspace_bytes(native, B)
    ws = torch.empty(ws_bytes // 4, dtype=torch.float32, device=images.device)
    memory = torch.full((B, tokens, model._cfg['embed_dim']), float('nan'), dtype=torch.float32, device=images.device)
    stream = _native.stream_ptr(images)
    if images.dtype == torch.uint8:
        tab = u8_normalise_table(images.device) if table == 'torch' else None
        _native.check(lib.parseq_train_encoder_forward_ex(native, _native.ptr(images), _native.PARSEQ_U8, _native.ptr(tab), B, _native.ptr(memory),
                                                          _native.ptr(ws), ws_bytes, stream))
    else:
        _native.check(lib.parseq_train_encoder_forward(native, _native.ptr(images), B, _native.ptr(memory), _native.ptr(ws), ws_bytes, stream))
    torch.cuda.synchronize()
    return memory


def _random_bytes(batch, system, seed):
    h, w = system.hparams.img_size
    g = torch.Generator().manual_seed(seed)
    u = torch.randint(0, 256, (batch, 3, h, w), generator=g, dtype=torch.int32).to(torch.uint8)
    u.view(-1)[:4] = torch.tensor([0, 255, 255, 0], dtype=torch.uint8)
    u.view(-1)[-2:] = torch.tensor([255, 0], dtype=torch.uint8)
    return u


@pytest.mark.parametrize('name,batch,precision', [('parseq', 3, 'fp32'), ('parseq', 3, 'bf16'), ('parseq', 3, 'bf16x3'), ('parseq-tiny', 3, 'fp32'),
                                                  ('vitstr', 2, 'fp32'), ('parseq-patch16-224', 2, 'fp32')])
def test_uint8_crops_give_the_float_entrys_memory(name, batch, precision):
    """parseq_train_encoder_forward_ex(PARSEQ_U8) against parseq_train_encoder_forward on the converted image, bit for bit: 8-byte
    segments (4 x 8 patches), 16-byte segments and 768 patch columns (patch16-224), S - 1 patch rows per image (ViTSTR)."""
    from gpu_util import DEV
    if name == 'vitstr':
        from oracle import vitstr_oracle as V
        from parseq_amd import create_model
        system = create_model('vitstr')
        system.model.load_state_dict(V.synth_state_dict(V.vitstr_config(), 0))
        system = system.to(DEV)
    else:
        from gpu_util import make_model
        system = make_model(name, 'bf16')
    system.train_precision = precision
    u = _random_bytes(batch, system, seed=3).to(DEV)
    assert int(u.min()) == 0 and int(u.max()) == 255
    converted = ((u.float() / 255.0) - 0.5) / 0.5               # the expression of the float path, on the device
    want = _train_memory(system, converted)
    got = _train_memory(system, u)
    assert not torch.isnan(want).any() and torch.equal(got, want)
    if name == 'parseq-tiny':
        # no table: the library's own IEEE ((v / 255) - 0.5) / 0.5, what the same expression gives on the host
        host = (((u.cpu().float() / 255.0) - 0.5) / 0.5).to(DEV)
        assert torch.equal(_train_memory(system, u, table=None), _train_memory(system, host))
        # an image pointer that is not patch_w-aligned takes the byte-wise loads: the same rows
        shifted = torch.empty(u.numel() + 3, dtype=torch.uint8, device=DEV)
        shifted[3:] = u.view(-1)
        assert torch.equal(_train_memory(system, shifted[3:].view(u.shape)), want)
    if name == 'parseq':
        from parseq_amd import _native
        bad = _native.lib().parseq_train_encoder_forward_ex(system.model._sync_native().model, _native.ptr(u), _native.PARSEQ_BF16, None, batch,
                                                            _native.ptr(want), _native.ptr(want), 0, _native.stream_ptr(u))
        assert bad != 0                                         # only fp32 and uint8 images


def test_loss_and_grads_takes_uint8_crops_unchanged():
    from gpu_util import DEV
    from parseq_amd.train import loss_and_grads
    system = _tiny()                                            # evaluation mode: dropout 0
    u = _random_bytes(4, system, seed=5).to(DEV)
    labels = ['ab', 'hello', 'x', 'word']
    perms = system.gen_tgt_perms(system.tokenizer.encode(labels, None))
    a = loss_and_grads(system, u, labels, perms)
    b = loss_and_grads(system, ((u.float() / 255.0) - 0.5) / 0.5, labels, perms)
    torch.cuda.synchronize()
    assert torch.equal(a.loss, b.loss) and torch.equal(a.flat, b.flat) and float(a.flat.abs().max()) > 0


# ---- parseq_weights_average ---------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """Distance in units in the last place between two fp32 tensors of the same sign pattern (or equal)."""
    d = (a.view(torch.int32).long() - b.view(torch.int32).long()).abs()
    return int(torch.where(a == b, torch.zeros_like(d), d).max())


@pytest.mark.parametrize('n_averaged', [0, 1, 2, 7])
def test_weights_average_on_the_flat_buffer_of_parseq_tiny(n_averaged):
    """avg <- w (n = 0), avg <- avg + (w - avg) / (n + 1) otherwise, against the torch expression in fp32 on the host, whose subtraction,
    division and addition are IEEE-exact like the kernel's (the bound asked for is 1 ulp; bit-identical for n = 0).  The flat buffer's
    length is a multiple of 32 (every tensor starts on a 32-element boundary), so ranges that are no multiple of the vector width, and a
    pair of pointers that is not 16-byte aligned, run too; elements past the range stay as they were."""
    from gpu_util import DEV
    from parseq_amd import _native
    from parseq_amd.train import param_views
    lib = _native.lib()
    system = _tiny()
    native = system.model._sync_native().model
    n = lib.parseq_model_grad_elems(native)
    assert n % 4 == 0
    sd = system.model.state_dict()
    shapes = {k: tuple(v.shape) for k, v in sd.items()}
    w = torch.zeros(n + 64, dtype=torch.float32, device=DEV)
    for k, view in param_views(native, w, shapes).items():
        view.copy_(sd[k])
    g = torch.Generator().manual_seed(n_averaged)
    start = (w.cpu() + 0.05 * torch.randn(n + 64, generator=g)).to(DEV)
    start[n:] = -7.0                                            # the guard past the end
    for lo, length in ((0, n), (0, n - 3), (1, n - 2), (5, 1001)):
        avg = start.clone()
        with _native.guard(avg):
            _native.check(lib.parseq_op_weights_average(_native.ptr(w[lo:]), _native.ptr(avg[lo:]), length, n_averaged, _native.stream_ptr(avg)))
        torch.cuda.synchronize()
        a, x = start.cpu()[lo:lo + length], w.cpu()[lo:lo + length]
        want = x.clone() if n_averaged == 0 else a + (x - a) / (n_averaged + 1)
        got = avg.cpu()
        assert torch.equal(got[:lo], start.cpu()[:lo]) and torch.equal(got[lo + length:], start.cpu()[lo + length:]), (lo, length)
        if n_averaged == 0:
            assert torch.equal(got[lo:lo + length], want)
        else:
            assert _ulps(got[lo:lo + length], want) <= 1, (lo, length)
    # the model's entry: over the master weights
    avg = start[:n].clone()
    _native.check(lib.parseq_weights_average(native, _native.ptr(avg), n_averaged, _native.stream_ptr(avg)))
    torch.cuda.synchronize()
    got, before = param_views(native, avg.cpu(), shapes), param_views(native, start[:n].cpu(), shapes)
    for k, v in sd.items():
        want = v.cpu() if n_averaged == 0 else before[k] + (v.cpu() - before[k]) / (n_averaged + 1)
        assert _ulps(got[k].contiguous(), want.contiguous()) <= (0 if n_averaged == 0 else 1), k
    assert lib.parseq_weights_average(native, None, 0, None) != 0 and lib.parseq_op_weights_average(_native.ptr(w), _native.ptr(avg), 0, 0, None) != 0


# ---- accumulation -------------------------------------------------------------------------------------------------------------------
def test_two_accumulated_batches_are_one_adamw_step_on_the_summed_halves():
    """TrainStep(accumulate_grad_batches=2) over batches A and B against the recomputation: the two gradients halved and summed,
    torch.nn.utils.clip_grad_norm_, one torch.optim.AdamW step on a host copy — to the tolerance of
    tests/test_training.py::test_three_optimiser_steps_follow_torch_adamw (errors against lr: max 0.1 lr and mean 2e-3 lr where the
    gradient is above 1e-6, Adam's own step bound elsewhere)."""
    from gpu_util import DEV
    from parseq_amd.train import TrainStep, loss_and_grads, param_views
    system = _tiny()                                            # fp32, evaluation mode: dropout 0
    assert getattr(system, 'train_precision', 'fp32') == 'fp32' and not system.training
    A, B = _random_bytes(4, system, seed=7).to(DEV), _random_bytes(4, system, seed=8).to(DEV)
    labels_a, labels_b = ['ab', 'hello', 'x', 'word'], ['tests', 'go', 'here', 'ok']
    perms = system.gen_tgt_perms(system.tokenizer.encode(labels_a, None))
    start = {k: v.detach().cpu().clone() for k, v in system.model.state_dict().items()}
    shapes = {k: tuple(v.shape) for k, v in start.items()}
    native = system.model._sync_native().model
    grads = [loss_and_grads(system, x, y, perms).flat.cpu() for x, y in ((A, labels_a), (B, labels_b))]
    step = TrainStep(system, total_steps=10, clip_val=5.0, accumulate_grad_batches=2)
    lr = step.lr
    assert step.max_lr == 2 * 8 / 256.0 * LR                    # base.py:98-101: the rate scales with the accumulation
    step(A, labels_a, perms)
    torch.cuda.synchronize()
    assert step.step_count == 0
    assert all(torch.equal(v.cpu(), start[k]) for k, v in system.model.state_dict().items())      # nothing moves after the first call
    step(B, labels_b, perms)
    torch.cuda.synchronize()
    assert step.step_count == 1 and step.flush() is False
    # the recomputation
    summed = grads[0] / 2 + grads[1] / 2
    params = {k: v.clone().requires_grad_(True) for k, v in start.items()}
    for k, gview in param_views(native, summed, shapes).items():
        params[k].grad = gview.clone()
    norm = torch.nn.utils.clip_grad_norm_(list(params.values()), 5.0)
    assert float(norm) > 5.0                                    # clipping is active
    first = {k: v.grad.clone() for k, v in params.items()}
    torch.optim.AdamW(list(params.values()), lr=lr, weight_decay=0.0).step()
    bad = []
    for key, t in system.model.state_dict().items():
        d_got, d_want = t.cpu() - start[key], params[key].detach() - start[key]
        err = (d_got - d_want).abs()
        real = first[key].abs() > 1e-6
        if real.any() and (float(err[real].max()) > 0.1 * lr or float(err[real].mean()) > 2e-3 * lr):
            bad.append((key, 'real', float(err[real].max()), float(err[real].mean())))
        if float(d_got.abs().max()) > 1.05 * lr + 0.02 * float(start[key].abs().max()) * lr:
            bad.append((key, 'bound', float(d_got.abs().max())))
        if float(d_want.abs().max()) > 0 and float(d_got.abs().max()) == 0:
            bad.append((key, 'unchanged'))
    assert not bad, (bad, lr)
    state = step.state_dict()
    assert state['step_count'] == 1 and state['accum_count'] == 0 and state['accum'] is None and float(state['exp_avg'].abs().max()) > 0


# ---- the loop is the step -----------------------------------------------------------------------------------------------------------
def test_fit_leaves_the_weights_of_the_hand_written_loop(folders):
    from gpu_util import DEV
    from parseq_amd.data import batch_slices, epoch_order
    from parseq_amd.fit import fit
    from parseq_amd.preprocess import resize_batch
    from parseq_amd.train import TrainStep
    looped = _tiny()
    train_set, val_set = _sets(folders, looped)
    assert len(train_set) == 32 and len(val_set) == 16
    result = fit(looped, train_set, val_set, max_epochs=2, val_check_interval=4, out_dir=str(folders / 'outputs' / 'parseq-tiny' / 'plain'),
                 accumulate_grad_batches=1, swa_epoch_start=1.0, augment=False, seed=SEED, workers=2)
    assert result.swa_n == 0 and result.train_step.step_count == 8
    by_hand = _tiny().train()
    by_hand.rng = np.random.default_rng(SEED)
    torch.manual_seed(SEED)
    step = TrainStep(by_hand, total_steps=8)
    for epoch in range(2):
        order = epoch_order(32, SEED, epoch)
        for b, e in batch_slices(32, 8):
            idx = order[b:e].tolist()
            crops = [torch.from_numpy(train_set.load(i).copy()).to(DEV) for i in idx]
            step(resize_batch(crops, (32, 128)), [train_set.labels[i] for i in idx])
    torch.cuda.synchronize()
    want, got = by_hand.model.state_dict(), looped.model.state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert torch.equal(result.train_step.exp_avg, step.exp_avg) and torch.equal(result.train_step.exp_avg_sq, step.exp_avg_sq)
    assert not torch.equal(want['head.weight'].cpu(), synth_state_dict(CONFIGS['parseq-tiny'], 0)['head.weight'])


# ---- end to end -----------------------------------------------------------------------------------------------------------------
E2E = dict(max_epochs=4, val_check_interval=4, accumulate_grad_batches=1, swa_epoch_start=0.5, augment=True, seed=SEED, workers=2)


@pytest.fixture(scope='module')
def end_to_end(folders):
    """The one uninterrupted run: PARSeq-Ti, fp32, dropout and augmentation on, 4 epochs of 4 batches, SWA from epoch 2."""
    from parseq_amd.fit import fit
    system = _tiny()
    system.train_precision = 'fp32'
    train_set, val_set = _sets(folders, system)
    out = str(folders / 'outputs' / 'parseq-tiny' / 'e2e')
    result = fit(system, train_set, val_set, out_dir=out, keep_epoch_snapshots=True, **E2E)
    torch.cuda.synchronize()
    return system, result, out


def _evaluate(system, val_set):
    from parseq_amd.data import Loader
    from parseq_amd.evaluate import Evaluator
    ev = Evaluator(system, validation=True)
    for batch in Loader(val_set, 8, (32, 128), system.device, shuffle=False, workers=2).epoch(0):
        ev.update(batch.images, batch.labels)
    r = ev.result()
    return 100.0 * r.correct / r.num_samples, 100.0 * (1.0 - r.ned / r.num_samples), float(r.loss)


def test_end_to_end_run(end_to_end, folders):
    from gpu_util import DEV
    from parseq_amd import load_from_checkpoint
    system, result, out = end_to_end
    _, val_set = _sets(folders, system)
    records = [json.loads(line) for line in open(os.path.join(out, 'log.jsonl'), encoding='utf-8')]
    assert records == result.log
    vals = [r for r in records if r['event'] == 'validation']
    assert [(r['epoch'], r['batch'], r['global_step']) for r in vals] == [(0, 3, 4), (1, 3, 8), (2, 3, 12), (3, 3, 16)]
    epochs = [r for r in records if r['event'] == 'epoch']
    assert [r['epoch'] for r in epochs] == [0, 1, 2, 3] and [r['swa_n'] for r in epochs] == [0, 0, 1, 2]
    print('training loss per epoch:', [round(r['train_loss'], 4) for r in epochs], 'validation:', [(r['val_accuracy'], r['val_NED'], r['val_loss']) for r in vals])
    # checkpoints: at most three ranked ones and last.ckpt (plus the snapshots this run was asked to keep)
    files = sorted(os.listdir(os.path.join(out, 'checkpoints')))
    ranked = [f for f in files if f.startswith('epoch=')]
    assert 1 <= len(ranked) <= 3 and 'last.ckpt' in files
    assert sorted(set(files) - set(ranked)) == [f'epoch_start={e}.ckpt' for e in range(4)] + ['last.ckpt']
    assert all(re.fullmatch(r'epoch=\d+-step=\d+-val_accuracy=\d+\.\d{4}-val_NED=-?\d+\.\d{4}(-v\d+)?\.ckpt', f) for f in ranked)
    assert sorted(os.path.basename(e['path']) for e in result.best) == ranked
    by_file = {r['checkpoint']: r for r in vals if r['checkpoint']}
    assert set(ranked) <= set(by_file)
    # what a validation logged is what a FRESH system loaded from the file of that validation measures (stale plans after an optimiser
    # step would show here)
    for name in ranked:
        r = by_file[name]
        assert name.startswith(f"epoch={r['epoch']}-step={r['global_step']}-val_accuracy={r['val_accuracy']:.4f}-val_NED={r['val_NED']:.4f}")
        fresh = load_from_checkpoint(os.path.join(out, 'checkpoints', name)).eval().to(DEV)
        acc, ned, loss = _evaluate(fresh, val_set)
        assert acc == r['val_accuracy'] and ned == pytest.approx(r['val_NED'], rel=1e-12, abs=1e-12) and loss == pytest.approx(r['val_loss'], rel=1e-6)
    # the model ends as the average of the weights at the starts of epochs 2 and 3
    assert result.swa_n == 2
    snaps = [torch.load(os.path.join(out, 'checkpoints', f'epoch_start={e}.ckpt'), map_location='cpu', weights_only=False)['state_dict'] for e in (2, 3)]
    final = system.model.state_dict()
    last = torch.load(os.path.join(out, 'checkpoints', 'last.ckpt'), map_location='cpu', weights_only=False)
    assert last['fit']['finished'] and last['fit']['swa_n'] == 2 and last['global_step'] == 16
    for k, v in final.items():
        a, b = snaps[0]['model.' + k], snaps[1]['model.' + k]
        want = a + (b - a) / 2
        assert torch.equal(v.cpu(), want), k
        assert torch.equal(last['state_dict']['model.' + k], want), k
    assert not torch.equal(snaps[0]['model.head.weight'], snaps[1]['model.head.weight'])
    # and the inference path runs on them
    assert _evaluate(system.eval(), val_set) == _evaluate(load_from_checkpoint(os.path.join(out, 'checkpoints', 'last.ckpt')).eval().to(DEV), val_set)
    assert epochs[-1]['train_loss'] < epochs[0]['train_loss'], [r['train_loss'] for r in epochs]


def test_resumed_run_ends_where_the_uninterrupted_one_does(end_to_end, folders):
    from parseq_amd.fit import fit
    system, result, _ = end_to_end
    out = str(folders / 'outputs' / 'parseq-tiny' / 'resumed')
    first = _tiny()
    assert float(first.hparams.dropout) > 0                      # dropout is on in both runs
    train_set, val_set = _sets(folders, first)
    half = fit(first, train_set, val_set, out_dir=out, stop_after_epoch=2, **E2E)
    assert not half.finished and half.train_step.step_count == 8 and half.swa_n == 0
    second = _tiny()
    whole = fit(second, train_set, val_set, out_dir=out, resume=os.path.join(out, 'checkpoints', 'last.ckpt'), **E2E)
    torch.cuda.synchronize()
    assert whole.finished and whole.train_step.step_count == 16 and whole.swa_n == 2
    want, got = system.model.state_dict(), second.model.state_dict()
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert torch.equal(whole.train_step.exp_avg, result.train_step.exp_avg) and torch.equal(whole.train_step.exp_avg_sq, result.train_step.exp_avg_sq)
    assert torch.equal(whole.swa_avg, result.swa_avg)
    with pytest.raises(ValueError):                              # a finished run has nothing to resume
        fit(_tiny(), train_set, val_set, out_dir=out, resume=os.path.join(out, 'checkpoints', 'last.ckpt'), **E2E)


# ---- command line -------------------------------------------------------------------------------------------------------------------
def test_train_py_writes_a_checkpoint_that_test_py_reads(folders):
    out = folders / 'outputs' / 'parseq-tiny' / 'cli'
    env = dict(os.environ, PYTHONPATH=ROOT + os.pathsep + os.environ.get('PYTHONPATH', ''))
    train = subprocess.run([sys.executable, os.path.join(ROOT, 'train.py'), 'parseq-tiny', '--train_dir', str(folders / 'data' / 'train'),
                            '--val_dir', str(folders / 'data' / 'val'), '--max_epochs', '1', '--batch_size', '8', '--val_check_interval', '4',
                            '--train_precision', 'bf16x3', '--workers', '2', '--out_dir', str(out), 'lr:float=0.0224'],
                           capture_output=True, text=True, timeout=300, env=env)
    assert train.returncode == 0, train.stdout[-2000:] + train.stderr[-2000:]
    last = out / 'checkpoints' / 'last.ckpt'
    assert last.is_file() and (out / 'log.jsonl').is_file()
    test = subprocess.run([sys.executable, os.path.join(ROOT, 'test.py'), str(last), '--data_root', str(folders / 'data'), '--batch_size', '16'],
                          capture_output=True, text=True, timeout=300, env=env)
    assert test.returncode == 0, test.stdout[-2000:] + test.stderr[-2000:]
    assert '| train' in test.stdout and '| val' in test.stdout and 'Combined' in test.stdout
    assert os.path.isfile(str(last) + '.log.txt')
