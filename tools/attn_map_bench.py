#!/usr/bin/env python3
"""Time what character localisation adds to a forward: PARSeq-S, bf16x3, synthetic weights, batch 512, AR decoding
with one refinement, max_length given so all 26 steps run.  Two calls alternate in one process — `forward` alone and `localize` (the same
forward, then the map pass, the map kernel and the geometry kernel, in one library call) — one call per timed run (a synchronisation after
each), over `--rounds` rounds; the median and the spread are reported, and the added time per batch with its share of `forward`.

    python tools/attn_map_bench.py [--batch 512] [--rounds 5] [--iters 10] [--out attn_map_bench.json]
    python tools/attn_map_bench.py --profile     # one warm-up + two localize calls, for a kernel trace
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

from oracle.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402


def build():
    from parseq_amd import create_model
    m = create_model('parseq', decode_ar=True, refine_iters=1, precision='bf16x3')
    m.model.load_state_dict(synth_state_dict(CONFIGS['parseq'], 0), strict=True)
    return m.eval().to('cuda')


def timed(fn, iters: int) -> float:
    """Seconds per call, one call at a time."""
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', action='store_true')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('attn_map_bench.py measures on the GPU; none is visible')
    cfg = CONFIGS['parseq']
    x = synth_images(args.batch, cfg, seed=1).to('cuda')
    m = build()

    def forward():
        with torch.inference_mode():
            m(x, cfg.max_label_length)

    def localize():
        with torch.inference_mode():
            m.localize(x)

    if args.profile:
        for _ in range(3):
            localize()
            torch.cuda.synchronize()
        return

    cases = {'forward': forward, 'localize': localize}
    for fn in cases.values():                 # every shape warm
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.rounds):              # alternate: other people's work shares the host
        for k, fn in cases.items():
            samples[k].append(timed(fn, args.iters) * 1e3)
    med = {k: statistics.median(v) for k, v in samples.items()}
    added = med['localize'] - med['forward']
    out = {'batch': args.batch, 'rounds': args.rounds, 'iters': args.iters, 'precision': 'bf16x3',
           'ms_median': {k: round(v, 3) for k, v in med.items()},
           'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in samples.items()},
           'added_ms': round(added, 3), 'added_over_forward': round(added / med['forward'], 4)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
