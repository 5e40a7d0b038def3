"""`Trainer.fit` on the reference's configuration (train.py:53-108, configs/main.yaml:33-41), on one device: from a folder of labelled
crops to trained checkpoints.

    fit(system, train_set, val_set, max_epochs=20, val_check_interval=1000, out_dir='outputs/parseq/run0')

The loop.  `system.train()` (dropout on); per batch of the `parseq_amd.data.Loader` — a shuffle per epoch from (seed, epoch), the last
short batch kept, RandAugment + bicubic resize on the device, uint8 crops straight into the training encoder — ONE `TrainStep` call
(forward, backward, accumulation, clipping, AdamW).  `total_steps`, the length of the OneCycle schedule, is the number of OPTIMISER steps
of the whole run: ceil(batches per epoch / accumulate_grad_batches) * max_epochs — the last batches of an epoch step as an incomplete
group (`TrainStep.flush`), as under Lightning.

Validation: after every `val_check_interval`-th batch of an epoch (Lightning's rule for an integer interval), at the end of every epoch if
the interval is longer than an epoch; `Evaluator(system, validation=True)` over the whole validation set; `val_accuracy` and `val_NED`
in percent and `val_loss` as base.py:146-177 defines them.  The weights it sees are those of the last optimiser step: the step re-packs
the inference plans.

Checkpoints, under `out_dir/checkpoints/`: the best three by `val_accuracy` as
`epoch=<e>-step=<optimiser steps>-val_accuracy=<.4f>-val_NED=<.4f>.ckpt` (train.py:86-92) and `last.ckpt`, rewritten at every validation,
at the end of every epoch and at the end of training.  A file is a `torch.save` of
    {'state_dict': {'model.<key>': tensor}, 'hyper_parameters': {...}, 'epoch', 'global_step',          # what load_from_checkpoint reads
     'fit': {'next_epoch', 'next_batch', 'train_step': TrainStep.state_dict(), 'swa_avg', 'swa_n',        # what an exact resume needs
             'rng': {'system', 'policy', 'torch', 'shuffle'}, 'best', 'epoch_losses', 'config', 'finished'}}
`rng`: the numpy generator states of the system (permutations, dropout seeds) and of the augmentation policy, torch's CPU generator
(`torch.randperm` draws the permutations of labels of five and more characters) and the (seed, epoch) pair the epoch's shuffle is drawn
from.  The default `out_dir` is `outputs/<model name>/<timestamp>`: `load_from_checkpoint` picks the class from the path.
`fit(..., resume=path)` continues from such a file — same configuration — and ends with the weights, moments and average of the
uninterrupted run, bit for bit.

Stochastic weight averaging.  The reference always switches on Lightning's `StochasticWeightAveraging(swa_lr, swa_epoch_start=0.75)`
(train.py:93-95).  Lightning is not installed here, so its callback cannot be executed; what this loop implements is, by definition:
  * `swa_start = int(max_epochs * swa_epoch_start)`;
  * from epoch `swa_start` on the OneCycle schedule is replaced by `torch.optim.swa_utils.SWALR(swa_lr, anneal_epochs=10,
    anneal_strategy='cos')`, stepped once per epoch, starting from the OneCycle value of that epoch's first step;
  * at the START of every epoch in [swa_start, max_epochs - 1] the current weights enter the average (the default rule of
    `torch.optim.swa_utils.AveragedModel`: avg <- w the first time, then avg <- avg + (w - avg) / (n + 1); `parseq_weights_average`);
  * at the end of training the average becomes the model's weights (`parseq_model_set_params`; there are no batch-norm statistics);
  * `swa_lr = lr * swa_lr_factor(warmup_pct, swa_epoch_start)`, the factor being what OneCycle's cosine annealing has left of the peak
    at `swa_epoch_start` of a 1000-step cycle (the rule of train.py:43-50, restated), `lr` the model's UNSCALED rate as in train.py:94.
`swa_epoch_start=1.0` switches it off.  `learning_rate` is the whole run's schedule as one pure function.

Log: one JSON line per validation and per epoch in `out_dir/log.jsonl`.  Out of scope: several ranks (`process_group` is handed to
`TrainStep` as it is), Hydra, LMDB, TensorBoard.
"""
from __future__ import annotations

import json
import math
import os
import shutil
import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import numpy as np
import torch
from torch import Tensor

from .train import one_cycle_lr

SWA_ANNEAL_EPOCHS = 10
AUGMENT_POLICIES = ('fourteen', 'reference')           # augment.RandAugment, augment.ReferenceRandAugment


# ---- the schedule: pure functions ---------------------------------------------------------------------------------------------------
def swa_lr_factor(warmup_pct: float, swa_epoch_start: float, div_factor: float = 25.0, final_div_factor: float = 1e4) -> float:
    """What fraction of its peak a OneCycle learning rate (cosine annealing, warm-up share `warmup_pct`) still has `swa_epoch_start` of the
    way through a 1000-step cycle: the second phase's cosine from 1 to 1 / (div_factor * final_div_factor)."""
    total = 1000
    begin, end = int(total * warmup_pct) - 1, total - 1
    pct = ((int(total * swa_epoch_start) - 1) - begin) / (end - begin)
    floor = 1 / (div_factor * final_div_factor)
    return floor + (1 - floor) / 2.0 * (math.cos(math.pi * pct) + 1)


def optimiser_steps_per_epoch(batches_per_epoch: int, accumulate_grad_batches: int) -> int:
    return -(-batches_per_epoch // accumulate_grad_batches)


def swa_start_epoch(max_epochs: int, swa_epoch_start: float) -> int:
    return int(max_epochs * swa_epoch_start)


def learning_rate(step: int, steps_per_epoch: int, max_epochs: int, max_lr: float, pct_start: float, swa_lr: float,
                  swa_epoch_start: float = 0.75, anneal_epochs: int = SWA_ANNEAL_EPOCHS) -> float:
    """The learning rate of optimiser step `step` (counted from 0) of a run of `max_epochs` epochs of `steps_per_epoch` optimiser steps:
    OneCycleLR(max_lr, steps_per_epoch * max_epochs, pct_start, cycle_momentum=False) stepped per optimiser step up to epoch `swa_start`,
    then SWALR(swa_lr, anneal_epochs, 'cos') stepped per epoch, which starts from the OneCycle value of its first epoch's first step.
    SWALR's recurrence is followed literally (it recovers the starting rate from the current one at every step), so the value is the one
    the scheduler object arrives at, rounding included."""
    total = steps_per_epoch * max_epochs
    if not 0 <= step < total:
        raise ValueError(f'step {step} outside the {total} optimiser steps of the run')
    epoch, first = step // steps_per_epoch, swa_start_epoch(max_epochs, swa_epoch_start)
    if epoch < first:
        return one_cycle_lr(step, total, max_lr, pct_start)
    anneal = lambda t: (1 - math.cos(math.pi * t)) / 2          # noqa: E731
    clamp = lambda v: max(0, min(1, v))                         # noqa: E731
    lr = one_cycle_lr(first * steps_per_epoch, total, max_lr, pct_start)
    for k in range(0, epoch - first + 1):                        # SWALR.get_lr at its step k (k = 0: the constructor's initial step)
        k_eff = max(1, k) if anneal_epochs == 0 else k
        prev_alpha = anneal(clamp((k_eff - 1) / max(1, anneal_epochs)))
        start = swa_lr if prev_alpha == 1 else (lr - prev_alpha * swa_lr) / (1 - prev_alpha)
        alpha = anneal(clamp(k_eff / max(1, anneal_epochs)))
        lr = swa_lr * alpha + start * (1 - alpha)
    return lr


# ---- stochastic weight averaging: the rule, apart from where the weights live ---------------------------------------------------------
def average_tensors_(avg: List[Tensor], weights: List[Tensor], n_averaged: int) -> None:
    """The averaging rule on lists of tensors (host stand-in of parseq_weights_average): avg <- w, or avg <- avg + (w - avg) / (n + 1)."""
    for a, w in zip(avg, weights):
        if n_averaged == 0:
            a.copy_(w)
        else:
            a.copy_(a + (w - a) / (n_averaged + 1))


class Swa:
    """When the weights enter the average and when the average becomes the weights.  `update(n_averaged)` and `transfer()` do the work
    wherever the weights live (the device buffers in `fit`, lists of tensors in the host tests)."""

    def __init__(self, max_epochs: int, swa_epoch_start: float, update: Callable[[int], None], transfer: Callable[[], None]):
        self.max_epochs, self.start = max_epochs, swa_start_epoch(max_epochs, swa_epoch_start)
        self.update, self.transfer = update, transfer
        self.n_averaged = 0

    def on_epoch_start(self, epoch: int) -> bool:
        if not self.start <= epoch <= self.max_epochs - 1:
            return False
        self.update(self.n_averaged)
        self.n_averaged += 1
        return True

    def on_train_end(self) -> bool:
        if not self.n_averaged:
            return False
        self.transfer()
        return True


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------------
def checkpoint_name(epoch: int, step: int, val_accuracy: float, val_ned: float) -> str:
    """ModelCheckpoint(filename='{epoch}-{step}-{val_accuracy:.4f}-{val_NED:.4f}') of train.py:86-92."""
    return f'epoch={epoch}-step={step}-val_accuracy={val_accuracy:.4f}-val_NED={val_ned:.4f}.ckpt'


def write_checkpoint(path: str, system, epoch: int, global_step: int, fit_state: Optional[dict] = None) -> None:
    """A file `parseq_amd.utils.load_from_checkpoint` reads like a Lightning checkpoint, plus the loop's own state under 'fit'.  Written
    to a temporary name and moved into place."""
    ckpt = {'state_dict': {'model.' + k: v.detach().cpu() for k, v in system.model.state_dict().items()},
            'hyper_parameters': dict(system.hparams), 'epoch': epoch, 'global_step': global_step, 'fit': fit_state}
    tmp = f'{path}.tmp{os.getpid()}'
    torch.save(ckpt, tmp)
    os.replace(tmp, path)


class TopK:
    """ModelCheckpoint(monitor='val_accuracy', mode='max', save_top_k=3): `offer` tells whether a file of this score is kept and
    returns the path that drops out (or None)."""

    def __init__(self, k: int = 3, entries=None):
        self.k = k
        self.entries = list(entries or [])          # [{'path', 'val_accuracy'}], any order

    def accepts(self, score: float) -> bool:
        return len(self.entries) < self.k or score > min(e['val_accuracy'] for e in self.entries)

    def add(self, path: str, score: float) -> Optional[str]:
        self.entries.append({'path': path, 'val_accuracy': score})
        if len(self.entries) <= self.k:
            return None
        worst = min(self.entries, key=lambda e: e['val_accuracy'])      # the earliest of equals
        self.entries.remove(worst)
        return worst['path']


def validation_batches(batches_per_epoch: int, val_check_interval: int) -> List[int]:
    """The batch numbers of an epoch (0-based) after which validation runs."""
    every = min(int(val_check_interval), batches_per_epoch)
    if every < 1:
        raise ValueError(f'val_check_interval={val_check_interval}')
    return [b for b in range(batches_per_epoch) if (b + 1) % every == 0]


@dataclass
class FitResult:
    out_dir: str
    train_step: object
    swa_avg: Optional[Tensor]
    swa_n: int
    best: List[dict]
    log: List[dict] = field(default_factory=list)
    finished: bool = True


def _validate(system, loader) -> dict:
    from .evaluate import Evaluator
    was_training = system.training
    system.eval()
    try:
        ev = Evaluator(system, validation=True)
        for batch in loader.epoch(0):
            ev.update(batch.images, batch.labels)
        r = ev.result()
    finally:
        system.train(was_training)
    n = max(r.num_samples, 1)
    return {'val_accuracy': 100.0 * r.correct / n, 'val_NED': 100.0 * (1.0 - r.ned / n), 'val_loss': float(r.loss)}


def fit(system, train_set, val_set, max_epochs: int, val_check_interval: int, out_dir: Optional[str] = None,
        accumulate_grad_batches: int = 1, swa_epoch_start: float = 0.75, augment: bool = True, seed: int = 0, resume: Optional[str] = None,
        workers: int = 8, clip_val: float = 20.0, process_group=None, stop_after_epoch: Optional[int] = None,
        keep_epoch_snapshots: bool = False, on_batch: Optional[Callable] = None, augment_policy: str = 'fourteen') -> FitResult:
    """Train `system` (on the GPU) on `train_set`, validating on `val_set` (datasets of parseq_amd.data); see the module docstring.

    The batch size is `system.batch_size`, the hyper-parameter the learning rate is scaled with (base.py:98-101), the arithmetic of the
    step `system.train_precision`.  `seed` seeds the shuffle, the augmentation policy, the system's permutation / dropout generator and
    torch's CPU generator.  `augment_policy`: 'fourteen' (`augment.RandAugment`, the draws of every run so far) or 'reference'
    (`augment.ReferenceRandAugment`: the reference's sixteen operators, GaussianBlur and PoissonNoise included).  `resume`: a checkpoint
    of this loop written under the same arguments (one without `augment_policy` reads as 'fourteen').  For tests and experiments:
    `stop_after_epoch=e` returns after epoch e - 1 (schedule and SWA as for `max_epochs`, nothing transferred; `last.ckpt` resumes it),
    `keep_epoch_snapshots` writes `checkpoints/epoch_start=<e>.ckpt` at the start of every epoch, `on_batch(epoch, batch, loss)` is
    called after every batch's step has been enqueued."""
    from . import _native
    from .data import Loader
    from .train import TrainStep
    dev = system.device
    if dev.type != 'cuda':
        raise RuntimeError('fit runs on the GPU (no CPU fallback); move the system to the device first')
    if augment_policy not in AUGMENT_POLICIES:
        raise ValueError(f'augment_policy {augment_policy!r} must be one of {AUGMENT_POLICIES}')
    name = system.hparams.get('name', 'parseq')
    if out_dir is None:
        out_dir = os.path.join('outputs', name, time.strftime('%Y-%m-%d_%H-%M-%S'))
    ckpt_dir = os.path.join(out_dir, 'checkpoints')
    os.makedirs(ckpt_dir, exist_ok=True)
    img_size, batch_size = tuple(system.hparams.img_size), int(system.batch_size)
    config = {'max_epochs': max_epochs, 'val_check_interval': val_check_interval, 'accumulate_grad_batches': accumulate_grad_batches,
              'swa_epoch_start': swa_epoch_start, 'augment': augment, 'seed': seed, 'batch_size': batch_size,
              'train_precision': getattr(system, 'train_precision', 'fp32'), 'train_samples': len(train_set), 'augment_policy': augment_policy}

    state = None
    if resume is not None:
        ckpt = torch.load(resume, map_location='cpu', weights_only=False)
        state = ckpt.get('fit')
        if not state:
            raise ValueError(f'{resume!r} holds no training state (not written by parseq_amd.fit)')
        saved = dict(state['config'])
        saved.setdefault('augment_policy', 'fourteen')     # checkpoints from before the key existed were drawn by the fourteen
        if saved != config:
            raise ValueError(f"resume under a different configuration: the checkpoint's {saved}, this run's {config}")
        system.load_state_dict(ckpt['state_dict'])

    system.train()
    policy = None
    if augment and augment_policy == 'reference':
        from .augment import ReferenceRandAugment
        policy = ReferenceRandAugment(seed=seed)
    train_loader = Loader(train_set, batch_size, img_size, dev, shuffle=True, augment=augment, seed=seed, workers=workers, policy=policy)
    val_loader = Loader(val_set, batch_size, img_size, dev, shuffle=False, augment=False, workers=workers)
    batches = len(train_loader)
    spe = optimiser_steps_per_epoch(batches, accumulate_grad_batches)
    step = TrainStep(system, total_steps=spe * max_epochs, clip_val=clip_val, accumulate_grad_batches=accumulate_grad_batches,
                     process_group=process_group)
    swa_lr = system.lr * swa_lr_factor(system.warmup_pct, swa_epoch_start)
    step.lr_fn = lambda k: learning_rate(k, spe, max_epochs, step.max_lr, step.pct_start, swa_lr, swa_epoch_start)
    val_at = set(validation_batches(batches, val_check_interval))

    lib = _native.lib()
    model = system.model
    swa_avg = torch.zeros_like(step.exp_avg)

    def swa_update(n_averaged: int) -> None:
        _native.check(lib.parseq_weights_average(model._sync_native().model, _native.ptr(swa_avg), n_averaged, _native.stream_ptr(swa_avg)))

    def swa_transfer() -> None:
        _native.check(lib.parseq_model_set_params(model._sync_native().model, _native.ptr(swa_avg), _native.stream_ptr(swa_avg)))
        model._adopt_native_weights()          # the module's tensors and the inference plans follow the master weights

    swa = Swa(max_epochs, swa_epoch_start, swa_update, swa_transfer)
    top = TopK(3)
    first_epoch = first_batch = 0
    epoch_losses: List[float] = []
    if hasattr(system, 'rng'):
        system.rng = np.random.default_rng(seed)
    torch.manual_seed(seed)
    if state is not None:
        if state.get('finished'):
            raise ValueError(f'{resume!r} is the end of a finished run')
        step.load_state_dict(state['train_step'])
        if state['swa_avg'] is not None:
            swa_avg.copy_(state['swa_avg'])
        swa.n_averaged = int(state['swa_n'])
        top = TopK(3, state['best'])
        first_epoch, first_batch = int(state['next_epoch']), int(state['next_batch'])
        epoch_losses = list(state['epoch_losses'])
        rng = state['rng']
        if hasattr(system, 'rng') and rng['system'] is not None:
            system.rng.bit_generator.state = rng['system']
        if train_loader.policy is not None and rng['policy'] is not None:
            train_loader.policy.rng.bit_generator.state = rng['policy']
        torch.set_rng_state(rng['torch'])

    records: List[dict] = []
    log_path = os.path.join(out_dir, 'log.jsonl')

    def log(record: dict) -> None:
        records.append(record)
        with open(log_path, 'a', encoding='utf-8') as fh:
            fh.write(json.dumps(record) + '\n')

    policy_state = [train_loader.policy.rng.bit_generator.state if train_loader.policy is not None else None]

    def fit_state(next_epoch: int, next_batch: int, losses: List[float], finished: bool = False) -> dict:
        return {'next_epoch': next_epoch, 'next_batch': next_batch, 'train_step': step.state_dict(),
                'swa_avg': swa_avg.cpu() if swa.n_averaged else None, 'swa_n': swa.n_averaged,
                'rng': {'system': system.rng.bit_generator.state if hasattr(system, 'rng') else None, 'policy': policy_state[0],
                        'torch': torch.get_rng_state(), 'shuffle': {'seed': seed, 'epoch': next_epoch}},
                'best': list(top.entries), 'epoch_losses': list(losses), 'config': config, 'finished': finished}

    last_path = os.path.join(ckpt_dir, 'last.ckpt')
    for epoch in range(first_epoch, max_epochs):
        if stop_after_epoch is not None and epoch >= stop_after_epoch:
            return FitResult(out_dir, step, swa_avg if swa.n_averaged else None, swa.n_averaged, list(top.entries), records, finished=False)
        started = time.time()
        start_batch = first_batch if epoch == first_epoch else 0
        losses: List = list(epoch_losses) if epoch == first_epoch else []
        if start_batch == 0:
            if keep_epoch_snapshots:
                write_checkpoint(os.path.join(ckpt_dir, f'epoch_start={epoch}.ckpt'), system, epoch, step.step_count)
            swa.on_epoch_start(epoch)
        for batch in train_loader.epoch(epoch, start=start_batch):
            loss = step(batch.images, batch.labels)
            policy_state[0] = batch.policy_state
            last_of_epoch = batch.index == batches - 1
            if last_of_epoch:
                step.flush()                     # an incomplete accumulation group steps at the end of the epoch
            losses.append(loss)
            if on_batch is not None:
                on_batch(epoch, batch.index, loss)
            if batch.index in val_at:
                metrics = _validate(system, val_loader)
                losses = [float(v) for v in losses]
                nxt = (epoch + 1, 0) if last_of_epoch else (epoch, batch.index + 1)
                kept = None
                if top.accepts(metrics['val_accuracy']):
                    base = checkpoint_name(epoch, step.step_count, metrics['val_accuracy'], metrics['val_NED'])
                    path, version = os.path.join(ckpt_dir, base), 0
                    while os.path.exists(path):          # the same epoch, step and scores twice (accumulation): Lightning's -v<n>
                        version += 1
                        path = os.path.join(ckpt_dir, base[:-len('.ckpt')] + f'-v{version}.ckpt')
                    dropped = top.add(path, metrics['val_accuracy'])
                    write_checkpoint(path, system, epoch, step.step_count, fit_state(nxt[0], nxt[1], [] if last_of_epoch else losses))
                    shutil.copyfile(path, last_path + '.tmp')
                    os.replace(last_path + '.tmp', last_path)
                    if dropped is not None and os.path.exists(dropped):
                        os.remove(dropped)
                    kept = os.path.basename(path)
                else:
                    write_checkpoint(last_path, system, epoch, step.step_count, fit_state(nxt[0], nxt[1], [] if last_of_epoch else losses))
                log({'event': 'validation', 'epoch': epoch, 'batch': batch.index, 'global_step': step.step_count, **metrics,
                     'checkpoint': kept})
        losses = [float(v) for v in losses]
        if (batches - 1) not in val_at:
            write_checkpoint(last_path, system, epoch, step.step_count, fit_state(epoch + 1, 0, []))
        log({'event': 'epoch', 'epoch': epoch, 'global_step': step.step_count, 'train_loss': sum(losses) / max(len(losses), 1),
             'lr': step.lr_fn(step.step_count - 1), 'swa_n': swa.n_averaged, 'seconds': time.time() - started})
    if swa.on_train_end():
        log({'event': 'swa_transfer', 'swa_n': swa.n_averaged, 'global_step': step.step_count})
    write_checkpoint(last_path, system, max_epochs - 1, step.step_count, fit_state(max_epochs, 0, [], finished=True))
    torch.cuda.current_stream(dev).synchronize()
    return FitResult(out_dir, step, swa_avg if swa.n_averaged else None, swa.n_averaged, list(top.entries), records)
