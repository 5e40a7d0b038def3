#!/usr/bin/env python3
"""Time the cloze refinement of the N-best adds to a beam search: PARSeq-S, bf16x3, synthetic weights, W in {4, 8, 16}
at B * W = 512 decoder rows, max_length given so all 26 steps run.  Three calls alternate in one process — the search alone, the search with
refine='score', the search with refine='edit' and one iteration — one call per timed run (a synchronisation after each), over `--rounds`
rounds; the median and the spread are reported.

The yardstick, timed in the same rounds: `forward`'s own refinement pass at 512 rows (AR decode with one refinement minus AR decode with
none).  The decoder pass is the same code, so what a refined search adds beyond it is the preparation, the two selection kernels and the copies.

    python tools/beam_refine_bench.py [--rows 512] [--rounds 5] [--iters 10] [--out beam_refine_bench.json]
    python tools/beam_refine_bench.py --profile 4 [--mode edit]     # one warm-up + one refined search of that width, for a kernel trace
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

WIDTHS = (4, 8, 16)


def build(refine_iters: int):
    from parseq_amd import create_model
    m = create_model('parseq', decode_ar=True, refine_iters=refine_iters, precision='bf16x3')
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
    ap.add_argument('--mode', default='edit', choices=['edit', 'score'], help='refinement of --profile')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('beam_refine_bench.py measures on the GPU; none is visible')
    cfg = CONFIGS['parseq']
    steps, ml = cfg.max_label_length + 1, cfg.max_label_length
    x = synth_images(args.rows, cfg, seed=1).to('cuda')
    m = build(0)

    def search(W, refine=None):
        def run():
            with torch.inference_mode():
                m.beam_search(x[:args.rows // W], W, ml, refine=refine)
        return run

    if args.profile:
        for _ in range(2):
            search(args.profile, args.mode)()
            torch.cuda.synchronize()
        return

    refined = build(1)

    def forward(model):
        def run():
            with torch.inference_mode():
                model(x, ml)
        return run

    cases = {'forward_ar_512': forward(m), 'forward_ar_refine1_512': forward(refined)}
    for W in WIDTHS:
        cases[f'search_w{W}'] = search(W)
        cases[f'score_w{W}'] = search(W, 'score')
        cases[f'edit_w{W}'] = search(W, 'edit')
    for fn in cases.values():                 # every shape warm
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.rounds):              # alternate the configurations: other people's work shares the host
        for k, fn in cases.items():
            samples[k].append(timed(fn, args.iters) * 1e3)
    med = {k: statistics.median(v) for k, v in samples.items()}
    yardstick = med['forward_ar_refine1_512'] - med['forward_ar_512']
    out = {'rows': args.rows, 'steps': steps, 'rounds': args.rounds, 'iters': args.iters, 'precision': 'bf16x3',
           'ms_median': {k: round(v, 3) for k, v in med.items()},
           'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in samples.items()},
           'forward_refinement_pass_ms': round(yardstick, 3), 'widths': {}}
    for W in WIDTHS:
        base = med[f'search_w{W}']
        out['widths'][W] = {'batch': args.rows // W, 'search_ms': round(base, 3),
                            'score_added_ms': round(med[f'score_w{W}'] - base, 3), 'edit_added_ms': round(med[f'edit_w{W}'] - base, 3),
                            'score_over_search': round(med[f'score_w{W}'] / base, 3), 'edit_over_search': round(med[f'edit_w{W}'] / base, 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
