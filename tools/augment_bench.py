#!/usr/bin/env python3
"""Cost of the training augmentation: `augment_resize_batch` on 384 seeded ragged crops (heights 16-96, widths 32-400) with chains
drawn by the policy (`RandAugment(magnitude=5, num_layers=3)`), against the same chains through Pillow plus `Image.resize(BICUBIC)`
on the host in the same process.

Device: W warm-up calls, then K calls each bracketed by device events on the current stream (the call uploads its descriptors and
synchronises once at its end, so the event pair covers descriptor copy + plan + stages + resize); host wall time of the same calls
beside it (descriptor building in Python included).  Median and minimum are reported.  Host: one pass of Pillow over the batch, one
thread, crops already decoded — the work a data loader would do per step.  The two results are compared byte for byte first.

    python tools/augment_bench.py [--batch 384] [--steps 20] [--warmup 5]   ->  one JSON line, profiles/augment_bench.json
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
sys.path.insert(0, os.path.join(ROOT, 'tools'))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=384)
    ap.add_argument('--steps', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'augment_bench.json'))
    args = ap.parse_args()
    from parseq_amd.augment import RandAugment, augment_resize_batch
    rng = np.random.default_rng(2024)
    sizes = [(int(rng.integers(16, 97)), int(rng.integers(32, 401))) for _ in range(args.batch)]
    hosts = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in sizes]
    chains = RandAugment(magnitude=5, num_layers=3, seed=7).sample(sizes)
    dev = torch.device('cuda', 0)
    imgs = [torch.from_numpy(a).to(dev) for a in hosts]

    for _ in range(args.warmup):
        out = augment_resize_batch(imgs, chains)
    torch.cuda.synchronize(dev)
    dev_ms, wall_ms = [], []
    for _ in range(args.steps):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        start.record()
        out = augment_resize_batch(imgs, chains)
        stop.record()
        stop.synchronize()
        wall_ms.append((time.perf_counter() - t0) * 1e3)
        dev_ms.append(start.elapsed_time(stop))

    result = {'batch': args.batch, 'steps': args.steps, 'warmup': args.warmup, 'operators': sum(len(c) for c in chains),
              'device_ms_median': statistics.median(dev_ms), 'device_ms_min': min(dev_ms),
              'call_wall_ms_median': statistics.median(wall_ms), 'call_wall_ms_min': min(wall_ms), 'gpu': torch.cuda.get_device_name(dev)}
    try:
        from PIL import Image
        from make_augment_golden import pillow_op
    except ImportError:
        result['host_pillow_ms'] = None
    else:
        def host_pass():
            res = []
            for a, chain in zip(hosts, chains):
                img = Image.fromarray(a, 'RGB')
                for op in chain:
                    img = pillow_op(img, op[0], *op[1:])
                res.append(np.asarray(img.resize((128, 32), Image.BICUBIC)))
            return res
        host_pass()
        t0 = time.perf_counter()
        want = host_pass()
        result['host_pillow_ms'] = (time.perf_counter() - t0) * 1e3
        got = out.cpu().numpy()
        result['equal_to_pillow'] = bool(all(np.array_equal(got[i], w.transpose(2, 0, 1)) for i, w in enumerate(want)))
        result['host_over_device'] = result['host_pillow_ms'] / result['device_ms_median']
        result['host_over_call_wall'] = result['host_pillow_ms'] / result['call_wall_ms_median']
    print(json.dumps(result))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as fh:
        json.dump(result, fh, indent=1)
        fh.write('\n')


if __name__ == '__main__':
    main()
