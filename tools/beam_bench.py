#!/usr/bin/env python3
"""Time of one beam search: PARSeq-S, bf16x3, synthetic weights, W in {1, 2, 4, 8} at B * W = 512 decoder rows,
max_length given so all 26 steps run.  One forward per timed run (a synchronisation after each), the configurations alternated over
`--rounds` rounds, the median and the spread reported.

Baselines, timed in the same process and the same rounds:
  greedy    `forward` (AR, 0 refinements) at batch B = 512 / W — the fused AR step, what a caller runs today for one string per crop
  per-op    the per-operation AR loop at batch 512 (PARSEQ_NO_FUSED_STEP=1, read when the plan is created): the decoder pass the search is built
            from, without the selection kernel, the replication and the second K / V projection

    python tools/beam_bench.py [--rows 512] [--rounds 5] [--iters 10] [--out beam_bench.json]
    python tools/beam_bench.py --profile 4      # one warm-up + one search of that width, for a kernel trace
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

WIDTHS = (1, 2, 4, 8)


def build(per_op: bool):
    from parseq_amd import create_model
    if per_op:
        os.environ['PARSEQ_NO_FUSED_STEP'] = '1'      # read when the plan is created (first forward)
    else:
        os.environ.pop('PARSEQ_NO_FUSED_STEP', None)
    m = create_model('parseq', decode_ar=True, refine_iters=0, precision='bf16x3')
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
    ap.add_argument('--rows', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('beam_bench.py measures on the GPU; none is visible')
    cfg = CONFIGS['parseq']
    steps, ml = cfg.max_label_length + 1, cfg.max_label_length
    x = synth_images(args.rows, cfg, seed=1).to('cuda')
    fused = build(False)

    def beam(W):
        def run():
            with torch.inference_mode():
                fused.beam_search(x[:args.rows // W], W, ml)
        return run

    if args.profile:
        for _ in range(2):
            beam(args.profile)()
            torch.cuda.synchronize()
        return

    def greedy(m, B):
        def run():
            with torch.inference_mode():
                m(x[:B], ml)
        return run

    def encode(B):
        def run():
            with torch.inference_mode():
                fused.model.encode(x[:B])
        return run

    with torch.inference_mode():
        fused(x, ml)                          # the fused model's plan at 512 rows, before the switch below is set
    per_op = build(True)
    with torch.inference_mode():
        per_op(x, ml)                         # plan creation reads PARSEQ_NO_FUSED_STEP
    os.environ.pop('PARSEQ_NO_FUSED_STEP', None)
    cases = {'per_op_ar_512': greedy(per_op, args.rows)}
    for W in WIDTHS:
        B = args.rows // W
        cases[f'beam_w{W}'] = beam(W)
        cases[f'greedy_b{B}'] = greedy(fused, B)
        cases[f'encode_b{B}'] = encode(B)
    for fn in cases.values():                 # every shape warm
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.rounds):              # alternate the configurations: other people's work shares the host
        for k, fn in cases.items():
            samples[k].append(timed(fn, args.iters) * 1e3)
    med = {k: statistics.median(v) for k, v in samples.items()}
    out = {'rows': args.rows, 'steps': steps, 'rounds': args.rounds, 'iters': args.iters, 'precision': 'bf16x3',
           'ms_median': {k: round(v, 3) for k, v in med.items()},
           'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in samples.items()}, 'widths': {}}
    for W in WIDTHS:
        B = args.rows // W
        b, g, e = med[f'beam_w{W}'], med[f'greedy_b{B}'], med[f'encode_b{B}']
        out['widths'][W] = {'batch': B, 'beam_ms': round(b, 3), 'greedy_ms': round(g, 3), 'encode_ms': round(e, 3),
                            'beam_over_greedy': round(b / g, 2), 'beam_over_per_op_512': round(b / med['per_op_ar_512'], 2),
                            'decode_us_per_step': round((b - e) * 1e3 / steps, 1), 'images_per_s': round(B / b * 1e3, 1)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
