#!/usr/bin/env python3
"""Times of orientation-robust reading on the GPU, written as a record to profiles/orient.md: `orient` at
(B, K) = (256, 2) and (128, 4) beside what a caller had before — `forward` on the same 512 rows followed by `parseq_postprocess` — PARSeq-S,
bf16x3, synthetic weights, uint8 views.  The calls run in one process, one call per timed sample with a synchronisation after it,
alternated over `--rounds` rounds; the median and the spread are reported.  The bytes the select kernel moves are computed from the shapes
here; its own time comes from a kernel trace taken in a separate run (`--trace-only` runs just the calls to be traced, a few times) and is
passed back in with `--select-us` / `--postprocess-us` / `--d2h-copies` when the record is written.  What was not measured is written as
"not measured".  Recognition accuracy is not measured: the weights are synthetic.

    python tools/orient_bench.py [--rounds 5] [--iters 20] [--out profiles/orient.md]
    rocprofv3 --kernel-trace --memory-copy-trace --stats -d DIR -- python tools/orient_bench.py --trace-only
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.synth import CONFIGS, synth_state_dict  # noqa: E402

SHAPES = [(256, 2), (128, 4)]
HBM_BYTES_PER_S = 8e12


def timed(fn, iters: int) -> float:
    """Seconds per call, one call at a time."""
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def select_bytes(B: int, K: int, L: int, C: int, image_bytes: int) -> dict:
    """What the two kernels of the choice read and write, from the shapes."""
    rows = B * K
    post = rows * L * C * 4 + rows * (2 * L + 2) * 4                          # every logit once (cache-resident for the second pass), ids / probs / len / conf out
    select = rows * (L + 1) * 4 + B * (2 * (L * C * 4 + image_bytes) + (L + 2) * 4 + K * 8 + 4)      # probs and lengths in; the winner's row and crop in and out
    return dict(postprocess=post, select=select)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--trace-only', action='store_true', help='run every call three times and exit (under a profiler)')
    ap.add_argument('--select-us', type=float, default=None, help='mean time of orient_select_kernel in the trace at (256, 2), microseconds')
    ap.add_argument('--postprocess-us', type=float, default=None, help='mean time of postprocess_kernel on 512 rows in the trace, microseconds')
    ap.add_argument('--d2h-copies', type=int, default=None, help='device-to-host copies the trace shows inside the orient calls')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'orient.md'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('orient_bench.py measures on the GPU; none is visible')
    from parseq_amd import _native, create_model
    cfg = CONFIGS['parseq']
    m = create_model('parseq', decode_ar=True, refine_iters=1, precision='bf16x3')
    m.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    m = m.eval().to('cuda')
    L, C = cfg.max_label_length + 1, len(m.tokenizer) - 2
    lib = _native.lib()
    g = torch.Generator().manual_seed(0)
    calls = {}
    for B, K in SHAPES:
        views = torch.randint(0, 256, (B, K, 3, *m.hparams.img_size), dtype=torch.uint8, generator=g).cuda()
        flat = views.flatten(0, 1)
        rows = B * K
        ids = torch.empty(rows, L, dtype=torch.int32, device='cuda')
        lengths = torch.empty(rows, dtype=torch.int32, device='cuda')
        probs = torch.empty(rows, L, dtype=torch.float32, device='cuda')
        conf = torch.empty(rows, dtype=torch.float32, device='cuda')

        def before(flat=flat, rows=rows, ids=ids, lengths=lengths, probs=probs, conf=conf):
            logits = m(flat)
            _native.check(lib.parseq_postprocess(_native.ptr(logits), rows, L, C, m.eos_id, _native.ptr(ids), _native.ptr(lengths), _native.ptr(probs),
                                                 _native.ptr(conf), _native.stream_ptr(logits)))

        calls[(B, K)] = (before, lambda views=views: m.orient(views))
    with torch.inference_mode():
        for before, orient in calls.values():      # warm-up: plans, code objects, allocator blocks
            for _ in range(3):
                before(); orient()
        torch.cuda.synchronize()
        if args.trace_only:
            return
        samples = {key: ([], []) for key in calls}
        for _ in range(args.rounds):
            for key, (before, orient) in calls.items():
                samples[key][0].append(timed(before, args.iters))
                samples[key][1].append(timed(orient, args.iters))

    def cell(values):
        return f'{1e3 * statistics.median(values):.3f} ms ({1e3 * min(values):.3f} .. {1e3 * max(values):.3f})'

    image_bytes = 3 * m.hparams.img_size[0] * m.hparams.img_size[1]
    nm = 'not measured'
    lines = ['# Orientation-robust reading: what the choice costs', '',
             f'`tools/orient_bench.py`, PARSeq-S, bf16x3, synthetic weights, uint8 views, AR + 1 refinement; {args.rounds} rounds of {args.iters} calls each, one call at a',
             'time with a synchronisation after it, the two calls alternated; median (least .. greatest round).  "before" is `forward` on the',
             'B K rows followed by `parseq_postprocess`: what a caller ran before the choice existed, without the copy to the host and the gather',
             'that would follow it.', '',
             '| (B, K) | rows | before: forward + postprocess | `orient` | difference of the medians |', '|---|---|---|---|---|']
    for (B, K), (tb, to) in samples.items():
        lines.append(f'| ({B}, {K}) | {B * K} | {cell(tb)} | {cell(to)} | {1e6 * (statistics.median(to) - statistics.median(tb)):+.1f} us |')
    by = select_bytes(256, 2, L, C, image_bytes)
    lines += ['', '## The two kernels of the choice, (B, K) = (256, 2)', '',
              '| kernel | time in the kernel trace (separate run) | bytes it moves (from the shapes) | those bytes at 8 TB/s |', '|---|---|---|---|',
              f'| `postprocess_kernel`, 512 rows | {f"{args.postprocess_us:.1f} us" if args.postprocess_us is not None else nm} | {by["postprocess"]} | {1e6 * by["postprocess"] / HBM_BYTES_PER_S:.2f} us |',
              f'| `orient_select_kernel`, 256 workgroups | {f"{args.select_us:.1f} us" if args.select_us is not None else nm} | {by["select"]} | {1e6 * by["select"] / HBM_BYTES_PER_S:.2f} us |',
              '', f'Device-to-host copies inside the `orient` calls in the trace: {args.d2h_copies if args.d2h_copies is not None else nm}.', '',
              'Recognition accuracy: not measured (no trained weights).', '']
    with open(args.out, 'w', encoding='utf-8') as fh:
        fh.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
