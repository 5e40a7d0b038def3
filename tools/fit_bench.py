#!/usr/bin/env python3
"""What the training loop costs on top of the bare training step (profiles/fit_loop.md): PARSeq-S, batch 384, rendered words held in
memory (tools/make_text_dataset.py render_words: no file decode), one process, every figure a median over repeated windows with its
spread (min .. max), each window closed by a device synchronise.

  bare_u8       TrainStep on one resident uint8 batch (the loop's input type)
  bare_f32      the same on the resident batch converted to normalised fp32 beforehand (the step as it was)
  bare_convert  the uint8 batch converted by torch inside the window — ((u.float() / 255) - 0.5) / 0.5 — what a caller of the float
                entry paid per step; bare_convert - bare_u8 is the uint8 path's saving
  loop_plain    the loop of parseq_amd.fit per batch — Loader (shuffle, one upload, resize on the device) + TrainStep — over whole epochs
  loop_augment  the same with RandAugment on the device

    python tools/fit_bench.py [--words 3072] [--batch 384] [--train-precision bf16x3] [--epochs 4] [--out FILE]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def summary(ms):
    return {'median_ms': statistics.median(ms), 'min_ms': min(ms), 'max_ms': max(ms), 'windows': len(ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--words', type=int, default=3072)
    ap.add_argument('--batch', type=int, default=384)
    ap.add_argument('--train-precision', default='bf16x3', choices=['fp32', 'bf16', 'bf16x3'])
    ap.add_argument('--epochs', type=int, default=4, help='timed epochs per loop variant (after one warm-up epoch)')
    ap.add_argument('--steps', type=int, default=8, help='steps per bare window')
    ap.add_argument('--windows', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fit_bench needs the GPU')
    from make_text_dataset import render_words
    from parseq_amd import create_model
    from parseq_amd.data import InMemoryDataset, Loader
    from parseq_amd.train import TrainStep
    dev = torch.device('cuda')
    torch.manual_seed(0)
    system = create_model('parseq', batch_size=args.batch).to(dev).train()
    system.train_precision = args.train_precision
    crops, labels = render_words(args.words, seed=0)
    data = InMemoryDataset(crops, labels)
    step = TrainStep(system, total_steps=10 ** 6)
    size = tuple(system.hparams.img_size)

    first = next(iter(Loader(data, args.batch, size, dev, shuffle=False).epoch(0)))
    u8, batch_labels = first.images, first.labels
    f32 = ((u8.float() / 255.0) - 0.5) / 0.5
    bare = {'bare_u8': lambda: step(u8, batch_labels), 'bare_f32': lambda: step(f32, batch_labels),
            'bare_convert': lambda: step(((u8.float() / 255.0) - 0.5) / 0.5, batch_labels)}
    result = {'config': vars(args), 'device': torch.cuda.get_device_name(0)}
    times = {k: [] for k in bare}
    for fn in bare.values():                                   # warm up every variant
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    for _ in range(args.windows):                              # alternate the variants window by window
        for name, fn in bare.items():
            t = time.perf_counter()
            for _ in range(args.steps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t) * 1e3 / args.steps)
    for name in bare:
        result[name] = summary(times[name])

    loops = {'loop_plain': Loader(data, args.batch, size, dev, augment=False, seed=0), 'loop_augment': Loader(data, args.batch, size, dev, augment=True, seed=0)}
    times = {k: [] for k in loops}
    for epoch in range(args.epochs + 1):                       # epoch 0 warms up; the variants alternate epoch by epoch
        for name, loader in loops.items():
            torch.cuda.synchronize()
            t = time.perf_counter()
            n = 0
            for batch in loader.epoch(epoch):
                step(batch.images, batch.labels)
                n += 1
            torch.cuda.synchronize()
            if epoch:
                times[name].append((time.perf_counter() - t) * 1e3 / n)
    for name in loops:
        result[name] = summary(times[name])
    line = json.dumps(result)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
