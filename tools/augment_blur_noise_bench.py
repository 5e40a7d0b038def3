#!/usr/bin/env python3
"""Cost of GaussianBlur and PoissonNoise on the device: `augment_resize_batch` on the 384 seeded ragged crops of tools/augment_bench.py
(heights 16-96, widths 32-400) under
  * the sixteen-operator policy (`ReferenceRandAugment(magnitude=5, num_layers=3)`),
  * one GaussianBlur per crop, radius 2 and radius 4,
  * one PoissonNoise per crop, lam 21 and lam 41,
  * empty chains (the resize alone: what every figure above contains).
Timing as in tools/augment_bench.py: W warm-up calls, K calls bracketed by device events, median and minimum; host wall time beside it.
Host: the same blurs through Pillow plus `Image.resize(BICUBIC)`, one thread, compared byte for byte first.  The noise has no host
counterpart to time: imgaug is not installed.

    python tools/augment_blur_noise_bench.py [--batch 384] [--steps 20] [--warmup 5] [--out FILE]   ->  one JSON line
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn, warmup, steps):
    for _ in range(warmup):
        out = fn()
    torch.cuda.synchronize()
    dev_ms, wall_ms = [], []
    for _ in range(steps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        out = fn()
        stop.record()
        stop.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(start.elapsed_time(stop))
    return out, {'device_ms_median': statistics.median(dev_ms), 'device_ms_min': min(dev_ms), 'call_wall_ms_median': statistics.median(wall_ms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=384)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from parseq_amd.augment import ReferenceRandAugment, augment_resize_batch
    rng = np.random.default_rng(2024)
    sizes = [(int(rng.integers(16, 97)), int(rng.integers(32, 401))) for _ in range(args.batch)]
    hosts = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    dev = torch.device('cuda', 0)
    imgs = [torch.from_numpy(a).to(dev) for a in hosts]
    policy = ReferenceRandAugment(magnitude=5, num_layers=3, seed=7).sample(sizes)
    cases = {'resize_only': [[]] * args.batch, 'sixteen_operator_policy': policy,
             'blur_radius_2': [[('GaussianBlur', 2)]] * args.batch, 'blur_radius_4': [[('GaussianBlur', 4)]] * args.batch,
             'noise_lam_21': [[('PoissonNoise', 21, i)] for i in range(args.batch)], 'noise_lam_41': [[('PoissonNoise', 41, i)] for i in range(args.batch)]}
    result = {'batch': args.batch, 'steps': args.steps, 'warmup': args.warmup, 'gpu': torch.cuda.get_device_name(dev),
              'policy_operators': sum(len(c) for c in policy),
              'policy_new_operators': sum(op[0] in ('GaussianBlur', 'PoissonNoise') for c in policy for op in c)}
    outs = {}
    for name, chains in cases.items():
        outs[name], result[name] = timed(lambda: augment_resize_batch(imgs, chains), args.warmup, args.steps)
    try:
        from PIL import Image, ImageFilter
    except ImportError:
        result['host_pillow'] = None
    else:
        for radius in (2, 4):
            def host_pass():
                return [np.asarray(Image.fromarray(a, 'RGB').filter(ImageFilter.GaussianBlur(radius)).resize((128, 32), Image.BICUBIC)) for a in hosts]
            host_pass()
            t0 = time.perf_counter()
            want = host_pass()
            ms = (time.perf_counter() - t0) * 1e3
            got = outs[f'blur_radius_{radius}'].cpu().numpy()
            result[f'blur_radius_{radius}'].update(host_pillow_ms=ms, equal_to_pillow=bool(all(np.array_equal(got[i], w.transpose(2, 0, 1)) for i, w in enumerate(want))),
                                                   host_over_device=ms / result[f'blur_radius_{radius}']['device_ms_median'])
    print(json.dumps(result))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            json.dump(result, fh, indent=1)
            fh.write('\n')


if __name__ == '__main__':
    main()
