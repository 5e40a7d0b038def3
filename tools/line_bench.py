#!/usr/bin/env python3
"""Times of line reading on the GPU, written as a record to profiles/read_lines.md: `read_lines` on 64 lines of
32 x 1000 pixels (11 windows each, 704 rows, one library call) beside the host alternative it replaces — the same plan and resize, then
`localize` and `forward` + `parseq_postprocess` on the window batch, five copies to the host and the numpy stitch of tests/line_reference.py.
PARSeq-S, bf16x3, synthetic weights.  The two run in one process, one call per timed sample with a synchronisation after it, alternated over
`--rounds` rounds; the median and the range are reported.  The stitch kernel's own time comes from a kernel trace taken in a separate run
(`--trace-only` runs just the calls to be traced, a few times) and is passed back in with `--stitch-us` when the record is written.  What was
not measured is written as "not measured".  Recognition accuracy is not measured: the weights are synthetic.

    python tools/line_bench.py [--rounds 5] [--iters 5] [--out profiles/read_lines.md]
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/line_bench.py --trace-only
"""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

from oracle.synth import CONFIGS, synth_state_dict  # noqa: E402

LINES, HEIGHT, WIDTH, MAX_BATCH = 64, 32, 1000, 1024


def timed(fn, iters: int) -> float:
    """Seconds per call, one call at a time."""
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--trace-only', action='store_true', help='run every call three times and exit (under a profiler)')
    ap.add_argument('--stitch-us', default=None, help='time of line_stitch_kernel in the trace, as text for the record')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'read_lines.md'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('line_bench.py measures on the GPU; none is visible')
    import line_reference as R
    from parseq_amd import _native, create_model
    from parseq_amd.preprocess import line_plan, line_views, resize_batch
    cfg = CONFIGS['parseq']
    m = create_model('parseq', decode_ar=True, refine_iters=1, precision='bf16x3')
    m.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    m = m.eval().to('cuda')
    L, C = cfg.max_label_length + 1, len(m.tokenizer) - 2
    img_size = tuple(m.hparams.img_size)
    lib = _native.lib()
    g = torch.Generator().manual_seed(0)
    images = [torch.randint(0, 256, (HEIGHT, WIDTH, 3), dtype=torch.uint8, generator=g).cuda() for _ in range(LINES)]
    stitch_seconds = []

    def device():
        return m.read_lines(images, max_batch=MAX_BATCH)

    def host():
        win, first = line_plan([(HEIGHT, WIDTH)] * LINES, img_size)
        batch = resize_batch(line_views(images, win, first), img_size)
        rows = batch.shape[0]
        loc = m.localize(batch)
        logits = m(batch)
        ids = torch.empty(rows, L, dtype=torch.int32, device='cuda')
        lengths = torch.empty(rows, dtype=torch.int32, device='cuda')
        probs = torch.empty(rows, L, dtype=torch.float32, device='cuda')
        _native.check(lib.parseq_postprocess(_native.ptr(logits), rows, L, C, m.eos_id, _native.ptr(ids), _native.ptr(lengths), _native.ptr(probs), None,
                                             _native.stream_ptr(logits)))
        parts = [t.cpu().numpy() for t in (loc.tokens, loc.lengths, probs, loc.centres, loc.boxes)]
        t0 = time.perf_counter()
        out = R.stitch_lines(*parts, np.array(win, np.int32), first, C, img_size, np.full(LINES, 0.25 * HEIGHT), 11 * (L - 1))
        stitch_seconds.append(time.perf_counter() - t0)
        return out

    with torch.inference_mode():
        for _ in range(2):                      # warm-up: plans, code objects, allocator blocks
            res = device(); ref = host()
        torch.cuda.synchronize()
        same = all(np.array_equal(getattr(res, k).cpu().numpy(), ref[r]) for k, r in (('lengths', 'len'), ('tokens', 'tokens'), ('src', 'src')))
        if args.trace_only:
            device()
            torch.cuda.synchronize()
            return
        stitch_seconds.clear()
        td, th = [], []
        for _ in range(args.rounds):
            td.append(timed(device, args.iters))
            th.append(timed(host, args.iters))

    def cell(values):
        return f'{1e3 * statistics.median(values):.2f} ms ({1e3 * min(values):.2f} .. {1e3 * max(values):.2f})'

    rows = int(res.windows.tokens.shape[0])
    lines = ['# Reading whole lines: the stitch on the device against the host loop it replaces', '',
             f'`tools/line_bench.py`, PARSeq-S, bf16x3, synthetic weights, AR + 1 refinement; {LINES} lines of {HEIGHT} x {WIDTH} pixels, {rows // LINES} windows each,',
             f'{rows} rows in one library call; {args.rounds} rounds of {args.iters} calls each, one call at a time with a synchronisation after it, the two',
             'alternated; median (least .. greatest round).  Both sides make the plan and the one `resize_batch` launch.  The host side then calls',
             '`localize` and `forward` + `parseq_postprocess` on the window batch, copies five tensors to the host and runs the plain numpy stitch of',
             '`tests/line_reference.py`, a Python loop per line; its own share is the last column.', '',
             '| `read_lines` | host alternative | of which the numpy stitch | ratio of the medians |', '|---|---|---|---|',
             f'| {cell(td)} | {cell(th)} | {1e3 * statistics.median(stitch_seconds):.2f} ms | {statistics.median(td) / statistics.median(th):.3f} |', '',
             f'Lengths, tokens and sources of the two agree on this workload: {same}.  Survivors per line: {int(res.lengths.min())} .. {int(res.lengths.max())}.', '',
             f'`line_stitch_kernel`, {LINES} workgroups, in the kernel trace (separate run): {args.stitch_us if args.stitch_us is not None else "not measured"}.', '',
             'Recognition accuracy: not measured (no trained weights).', '']
    with open(args.out, 'w', encoding='utf-8') as fh:
        fh.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
