#!/usr/bin/env python3
"""Throughput of PARSeq-S with decoders of depth 1, 2 and 3: batch 512, AR + 1 refinement (max_length given,
so every step runs and no host read ends the call), bf16x3, synthetic weights.

For every configuration: images/s with forwards enqueued back to back and one synchronisation at the end ("in flight"), and with a
synchronisation after each forward ("one at a time"); the AR loop's time per step, from the same batch's AR + 0 forward minus its
encoder alone, divided by the step count.  The depth-1 rows are measured twice: the fused AR step (the default) and the per-op step
(PARSEQ_NO_FUSED_STEP=1), the per-layer building block a deeper decoder composes.

    python tools/dec_depth_bench.py [--batch 512] [--iters 20] [--out dec_depth_bench.json]
    python tools/dec_depth_bench.py --profile-depth 2     # one warm-up + one forward of that depth, for a kernel trace
"""
from __future__ import annotations

import argparse
import dataclasses
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402


def build(depth: int, per_op: bool):
    from parseq_amd import create_model
    if per_op:
        os.environ['PARSEQ_NO_FUSED_STEP'] = '1'      # read when the plan is created (first forward)
    else:
        os.environ.pop('PARSEQ_NO_FUSED_STEP', None)
    cfg = dataclasses.replace(CONFIGS['parseq'], dec_depth=depth)
    m = create_model('parseq', dec_depth=depth, precision='bf16x3')
    m.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    return m.eval().to('cuda'), cfg


def timed(fn, iters: int, sync_each: bool) -> float:
    """Seconds per call."""
    fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        if sync_each:
            torch.cuda.synchronize()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def measure(depth: int, per_op: bool, batch: int, iters: int) -> dict:
    m, cfg = build(depth, per_op)
    x = synth_images(batch, cfg, seed=1).to('cuda')
    steps = cfg.max_label_length + 1

    def fwd(refine):
        def run():
            m.model.decode_ar, m.model.refine_iters = True, refine
            with torch.inference_mode():
                m(x, cfg.max_label_length)
        return run
    with torch.inference_mode():
        m(x, cfg.max_label_length)                  # plan creation + the per-op flag read
    ar1_flight = timed(fwd(1), iters, False)
    ar1_seq = timed(fwd(1), iters, True)
    ar0 = timed(fwd(0), iters, True)

    def enc():
        with torch.inference_mode():
            m.model.encode(x)
    enc_t = timed(enc, iters, True)
    row = {'dec_depth': depth, 'ar_step': 'per-op' if (per_op or depth > 1) else 'fused', 'batch': batch, 'steps': steps,
           'ar1_images_per_s_in_flight': round(batch / ar1_flight, 1), 'ar1_images_per_s_one_at_a_time': round(batch / ar1_seq, 1),
           'ar1_ms_one_at_a_time': round(ar1_seq * 1e3, 3), 'ar0_ms': round(ar0 * 1e3, 3), 'encode_ms': round(enc_t * 1e3, 3),
           'ar_loop_us_per_step': round((ar0 - enc_t) * 1e6 / steps, 1)}
    del m
    torch.cuda.empty_cache()
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--out', default=None, help='also write the rows as JSON to this file')
    ap.add_argument('--profile-depth', type=int, default=0)
    args = ap.parse_args()
    os.environ.setdefault('PARSEQ_SMALL_BATCH', '64')
    if args.profile_depth:
        m, cfg = build(args.profile_depth, False)
        x = synth_images(args.batch, cfg, seed=1).to('cuda')
        m.model.decode_ar, m.model.refine_iters = True, 1
        with torch.inference_mode():
            for _ in range(2):                        # warm-up (plan creation) + the traced forward
                m(x, cfg.max_label_length)
        torch.cuda.synchronize()
        print('profiled', args.profile_depth)
        return
    rows = [measure(1, False, args.batch, args.iters), measure(1, True, args.batch, args.iters),
            measure(2, False, args.batch, args.iters), measure(3, False, args.batch, args.iters)]
    for r in rows:
        print(json.dumps(r))
    if not args.out:
        return
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        json.dump({'device': torch.cuda.get_device_name(0), 'precision': 'bf16x3', 'mode': 'AR + 1 refinement, max_length 25', 'rows': rows}, f, indent=1)


if __name__ == '__main__':
    main()
