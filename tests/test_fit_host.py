"""Host half of the training loop (parseq_amd/fit.py, parseq_amd/data.py, the accumulation bookkeeping of parseq_amd/train.py): the
schedule against torch's own schedulers, the averaging rule against AveragedModel, the dataset filter and the shuffle, the optimiser-step
bookkeeping, and the checkpoint round trip — none of it needs a device."""
import importlib.util
import math
import os

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool(name):
    spec = importlib.util.spec_from_file_location(f'parseq_tool_{name}', os.path.join(ROOT, 'tools', f'{name}.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---- schedule ---------------------------------------------------------------------------------------------------------------------
def _one_cycle_factor(warmup_pct, swa_epoch_start, div_factor=25, final_div_factor=1e4):
    """The OneCycle formula on a 1000-step cycle, from torch's scheduler itself: the rate at step int(1000 * swa_epoch_start) - 1
    over the peak — with the phase boundary the reference's rule uses (int(total * pct) - 1; the scheduler's own is float(pct * total) - 1,
    the same number for every warm-up share whose product with 1000 is whole)."""
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.AdamW([p], lr=1.0)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, 1.0, 1000, pct_start=warmup_pct, cycle_momentum=False, div_factor=div_factor,
                                                final_div_factor=final_div_factor)
    for _ in range(int(1000 * swa_epoch_start) - 1):
        opt.step()
        sched.step()
    return opt.param_groups[0]['lr']


@pytest.mark.parametrize('swa_epoch_start', [0.5, 0.75])
def test_swa_lr_factor_is_the_one_cycle_value(swa_epoch_start):
    from parseq_amd.fit import swa_lr_factor
    got = swa_lr_factor(0.075, swa_epoch_start)
    assert abs(got - _one_cycle_factor(0.075, swa_epoch_start)) <= 1e-12 * got
    # and the closed form: cosine from 1 to 1 / (25 * 1e4) over steps 74 .. 999
    pct = ((int(1000 * swa_epoch_start) - 1) - 74) / (999 - 74)
    floor = 1 / 25e4
    assert abs(got - (floor + (1 - floor) / 2 * (math.cos(math.pi * pct) + 1))) <= 1e-15


@pytest.mark.parametrize('accumulate', [1, 2])
@pytest.mark.parametrize('swa_epoch_start', [0.5, 0.75])
@pytest.mark.parametrize('batches_per_epoch', [3, 7])
@pytest.mark.parametrize('max_epochs', [4, 20])
def test_learning_rate_follows_one_cycle_then_swalr(max_epochs, batches_per_epoch, swa_epoch_start, accumulate):
    """Every optimiser step's rate against a real AdamW driven by OneCycleLR per step and, from epoch swa_start on, by SWALR per epoch."""
    from parseq_amd.fit import learning_rate, optimiser_steps_per_epoch, swa_lr_factor, swa_start_epoch
    base_lr, warmup, batch_size = 7e-4, 0.075, 384
    spe = optimiser_steps_per_epoch(batches_per_epoch, accumulate)
    assert spe == -(-batches_per_epoch // accumulate)
    max_lr = accumulate * math.sqrt(1) * batch_size / 256.0 * base_lr          # base.py:98-101
    swa_lr = base_lr * swa_lr_factor(warmup, swa_epoch_start)
    assert abs(swa_lr - base_lr * _one_cycle_factor(warmup, swa_epoch_start)) <= 1e-12 * swa_lr
    first = swa_start_epoch(max_epochs, swa_epoch_start)
    assert first == int(max_epochs * swa_epoch_start)
    p = torch.zeros(1, requires_grad=True)
    opt = torch.optim.AdamW([p], lr=max_lr)
    sched = torch.optim.lr_scheduler.OneCycleLR(opt, max_lr, spe * max_epochs, pct_start=warmup, cycle_momentum=False)
    swa_sched = None
    step = 0
    for epoch in range(max_epochs):
        if epoch == first:
            swa_sched = torch.optim.swa_utils.SWALR(opt, swa_lr, anneal_epochs=10, anneal_strategy='cos')
        for _ in range(spe):
            want = opt.param_groups[0]['lr']
            got = learning_rate(step, spe, max_epochs, max_lr, warmup, swa_lr, swa_epoch_start)
            assert abs(got - want) <= 1e-12 * want, (epoch, step, got, want)
            p.grad = torch.ones(1)
            opt.step()
            if swa_sched is None:
                sched.step()
            step += 1
        if swa_sched is not None:
            swa_sched.step()
    assert step == spe * max_epochs
    with pytest.raises(ValueError):
        learning_rate(step, spe, max_epochs, max_lr, warmup, swa_lr, swa_epoch_start)


def test_swa_off_is_the_plain_one_cycle():
    from parseq_amd.fit import learning_rate
    from parseq_amd.train import one_cycle_lr
    for step in range(12):
        assert learning_rate(step, 3, 4, 1e-3, 0.075, 1e-4, swa_epoch_start=1.0) == one_cycle_lr(step, 12, 1e-3, 0.075)


# ---- averaging and transfer rule ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('max_epochs,swa_epoch_start', [(4, 0.5), (4, 0.75), (20, 0.75), (5, 1.0)])
def test_swa_averages_the_epoch_start_snapshots_like_averaged_model(max_epochs, swa_epoch_start):
    from parseq_amd.fit import Swa, average_tensors_
    g = torch.Generator().manual_seed(3)
    module = torch.nn.Sequential(torch.nn.Linear(7, 5), torch.nn.Linear(5, 3))
    weights = [p.detach() for p in module.parameters()]
    avg = [torch.zeros_like(w) for w in weights]
    transferred = []

    def transfer():
        transferred.append(True)
        for w, a in zip(weights, avg):
            w.copy_(a)
    swa = Swa(max_epochs, swa_epoch_start, lambda n: average_tensors_(avg, weights, n), transfer)
    reference = torch.optim.swa_utils.AveragedModel(module)
    first = int(max_epochs * swa_epoch_start)
    snapshots = []
    for epoch in range(max_epochs):
        entered = swa.on_epoch_start(epoch)
        assert entered == (first <= epoch <= max_epochs - 1)
        if entered:
            snapshots.append([w.clone() for w in weights])
            reference.update_parameters(module)
        for w in weights:                                  # the fake step
            w.add_(torch.randn(w.shape, generator=g) * 0.1)
    assert swa.n_averaged == len(snapshots) == max(0, max_epochs - first)
    # exactly those snapshots: the running mean, folded in the rule's own order
    want = None
    for n, snap in enumerate(snapshots):
        want = [s.clone() for s in snap] if n == 0 else [a + (s - a) / (n + 1) for a, s in zip(want, snap)]
    before = [w.clone() for w in weights]
    assert swa.on_train_end() == bool(snapshots) == bool(transferred)
    if not snapshots:
        assert all(torch.equal(w, b) for w, b in zip(weights, before))      # SWA off: the weights stay
        return
    for w, a, ref, plain in zip(weights, want, reference.module.parameters(), zip(*snapshots)):
        assert torch.equal(w, a)
        # AveragedModel folds with lerp(avg, w, 1 / (n + 1)): the same number up to the rounding of a handful of fp32 operations on
        # values of the snapshots' size, per update
        bound = 4 * 2.0 ** -23 * float(torch.stack(plain).abs().max()) * len(snapshots)
        assert float((w - ref.detach()).abs().max()) <= bound
        assert float((w - torch.stack(plain).mean(0)).abs().max()) <= bound


# ---- dataset ----------------------------------------------------------------------------------------------------------------------
def test_labelled_folder_applies_the_reference_filter(tmp_path):
    from parseq_amd.configs import CHARSET_94_FULL
    from parseq_amd.data import LabelledFolder, read_gt
    lines = ['a.png Hello World\n', 'b.png  Café \n', 'c.png ' + 'x' * 26 + '\n', 'd.png 丘丸\n', 'lonely.png\n', '\n', 'e.png\ttab\tbed\n',
             'f.png ' + 'y' * 25 + '\n']
    (tmp_path / 'gt.txt').write_text(''.join(lines), encoding='utf-8')
    ds = LabelledFolder(str(tmp_path), CHARSET_94_FULL, 25)
    assert ds.labels == ['HelloWorld', 'Cafe', 'tabbed', 'y' * 25]
    assert [os.path.basename(f) for f, _ in ds.samples] == ['a.png', 'b.png', 'e.png', 'f.png']
    # the 36-character training charset lower-cases, as the reference's CharsetAdapter does
    assert [label for _, label in read_gt(str(tmp_path), '0123456789abcdefghijklmnopqrstuvwxyz', 25)][:2] == ['helloworld', 'cafe']
    # test.py's names are the same functions
    spec = importlib.util.spec_from_file_location('parseq_test_cli_fit', os.path.join(ROOT, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    from parseq_amd import data
    assert cli.preprocess_label is data.preprocess_label and cli.parse_gt_line is data.parse_gt_line


def test_shuffle_is_seeded_per_epoch_and_keeps_the_short_batch():
    from parseq_amd.data import batch_slices, epoch_order
    a, b = epoch_order(37, 5, 0), epoch_order(37, 5, 0)
    assert np.array_equal(a, b) and sorted(a.tolist()) == list(range(37))
    assert not np.array_equal(a, epoch_order(37, 5, 1)) and not np.array_equal(a, epoch_order(37, 6, 0))
    assert np.array_equal(epoch_order(37, 5, 0, shuffle=False), np.arange(37))
    assert batch_slices(37, 8) == [(0, 8), (8, 16), (16, 24), (24, 32), (32, 37)]
    assert batch_slices(32, 8)[-1] == (24, 32) and batch_slices(3, 8) == [(0, 3)]


def test_loader_host_half_visits_every_sample_once(tmp_path):
    """The host half of the loader (decode pool, per-epoch order, policy draws) on a rendered folder; the device half needs a GPU."""
    from concurrent.futures import ThreadPoolExecutor

    from parseq_amd.data import LabelledFolder, Loader
    labels = _tool('make_text_dataset').write_dataset(str(tmp_path / 'words'), 11, seed=4)
    ds = LabelledFolder(str(tmp_path / 'words'), 'abcdefghijklmnopqrstuvwxyz', 25)
    assert ds.labels == labels and all(1 <= len(s) <= 6 and s.islower() for s in labels)
    loader = Loader(ds, 4, (32, 128), 'cpu', augment=True, seed=9, workers=2)
    assert len(loader) == 3
    with ThreadPoolExecutor(2) as pool:
        host = list(loader._host_batches(1, 0, pool))
        again = list(Loader(ds, 4, (32, 128), 'cpu', augment=True, seed=9, workers=2)._host_batches(1, 0, pool))
        tail = list(Loader(ds, 4, (32, 128), 'cpu', augment=True, seed=9, workers=2)._host_batches(1, 2, pool))
    assert [len(h.crops) for h in host] == [4, 4, 3]
    assert sorted(i for h in host for i in h.indices.tolist()) == list(range(11))
    assert np.array_equal(np.concatenate([h.indices for h in host]), loader.order(1))
    for h in host:
        assert h.labels == [labels[i] for i in h.indices.tolist()] and len(h.chains) == len(h.crops)
        assert all(c.dtype == np.uint8 and c.ndim == 3 and c.shape[2] == 3 for c in h.crops)
    assert [h.chains for h in host] == [h.chains for h in again] and host[-1].policy_state == again[-1].policy_state
    assert [h.index for h in tail] == [2] and np.array_equal(tail[0].indices, host[2].indices)
    sizes = {h.crops[0].shape[:2] for h in host} | {c.shape[:2] for c in host[0].crops}
    assert len(sizes) > 1                                                   # crops of varied size


# ---- accumulation bookkeeping -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('every', [1, 2, 3])
def test_accumulator_steps_every_n_calls_and_at_flush(every):
    from parseq_amd.train import GradAccumulator
    seen = []
    acc = GradAccumulator(every, lambda flat: seen.append(flat.clone()))
    grads = [torch.full((5,), float(i + 1)) for i in range(7)]
    stepped = [acc.add(g) for g in grads]
    assert stepped == [(i + 1) % every == 0 for i in range(7)]
    assert acc.flush() == (7 % every != 0) and acc.flush() is False
    groups = [grads[at:at + every] for at in range(0, 7, every)]
    assert len(seen) == len(groups)
    for got, group in zip(seen, groups):                                     # an incomplete group is still divided by the full count
        want = sum(g / every for g in group)
        assert torch.allclose(got, want, rtol=1e-6, atol=0)
    with pytest.raises(ValueError):
        GradAccumulator(0, lambda flat: None)


def test_validation_points_and_top_k():
    from parseq_amd.fit import TopK, checkpoint_name, validation_batches
    assert validation_batches(10, 4) == [3, 7] and validation_batches(4, 4) == [3] and validation_batches(4, 1000) == [3]
    assert checkpoint_name(3, 120, 87.5, 93.21987) == 'epoch=3-step=120-val_accuracy=87.5000-val_NED=93.2199.ckpt'
    top = TopK(3)
    dropped = []
    for name, score in [('a', 10.0), ('b', 30.0), ('c', 20.0), ('d', 5.0), ('e', 20.0), ('f', 25.0)]:
        if top.accepts(score):
            dropped.append(top.add(name, score))
    # d (5) and nothing else is refused; e (20) pushes a (10) out; f (25) pushes out the earlier of the two 20s
    assert sorted(e['path'] for e in top.entries) == ['b', 'e', 'f'] and dropped == [None, None, None, 'a', 'c']


# ---- checkpoint -----------------------------------------------------------------------------------------------------------------
def test_checkpoint_loads_through_load_from_checkpoint(tmp_path):
    from parseq_amd import create_model, load_from_checkpoint
    from parseq_amd.fit import write_checkpoint
    system = create_model('parseq-tiny', batch_size=8, max_label_length=10, charset_train='abcdefghijklmnopqrstuvwxyz')
    with torch.no_grad():
        for i, p in enumerate(system.parameters()):
            p.add_(0.01 * (i % 7))
    path = tmp_path / 'outputs' / 'parseq-tiny' / 'run' / 'checkpoints' / 'last.ckpt'
    path.parent.mkdir(parents=True)
    write_checkpoint(str(path), system, 3, 17, {'next_epoch': 4})
    raw = torch.load(str(path), map_location='cpu', weights_only=False)
    assert raw['epoch'] == 3 and raw['global_step'] == 17 and raw['fit'] == {'next_epoch': 4}
    assert all(k.startswith('model.') for k in raw['state_dict'])
    loaded = load_from_checkpoint(str(path))
    assert dict(loaded.hparams) == dict(system.hparams)
    want, got = system.state_dict(), loaded.state_dict()
    assert list(want) == list(got) and all(torch.equal(want[k], got[k]) for k in want)
