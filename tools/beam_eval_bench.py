#!/usr/bin/env python3
"""What evaluating an N-best costs per batch: PARSeq-S, bf16x3, batch 512, W = 5, synthetic weights.  Over the same
batches, the three loops alternated over `--rounds` rounds after a warm-up pass of each; median (min .. max) of the rounds:

  search       `model.beam_search(images, W)` back to back, one synchronisation at the end
  host         per batch `beam_search`, `tokenizer.decode_beams` (the copy to the host), then the per-hypothesis Python loop: adapter, edit
               distance, ranks — `parseq_amd.evaluate.host_beam_metrics`, what `BeamEvaluator` itself runs on its host path
  evaluator    `BeamEvaluator.update(images, labels)` per batch, then `result()`: the search and the metrics on the device, one copy at the end

    python tools/beam_eval_bench.py [--batch 512] [--batches 20] [--width 5] [--rounds 5] [--out profiles/beam_eval.json]
    python tools/beam_eval_bench.py --only evaluator        # one loop alone, for a kernel / memory-copy trace

The labels are the model's own N-best strings, image i taking rank i mod (W + 1) (W: a string of its own), so hits at every rank and misses
occur; recognition accuracy is not measured: the weights are synthetic.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--width', type=int, default=5)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', choices=['search', 'host', 'evaluator'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from parseq_amd import create_model
    from parseq_amd.evaluate import BeamEvaluator, host_beam_metrics
    cfg = CONFIGS['parseq']
    model = create_model('parseq', precision='bf16x3')
    model.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    model = model.eval().to('cuda')
    width, adapter, tokenizer = args.width, model.charset_adapter, model.tokenizer
    data = []
    for i in range(args.batches):
        images = synth_images(args.batch, cfg, seed=100 + i).to('cuda')
        with torch.inference_mode():
            beams = tokenizer.decode_beams(model.beam_search(images, width))
        labels = []
        for k, alts in enumerate(beams):
            strings = [adapter(s) for s, _ in alts]
            rank = k % (width + 1)
            labels.append(strings[rank] if rank < len(strings) and strings[rank] else 'q' * (1 + k % 7))
        data.append((images, labels))
    evaluator = BeamEvaluator(model, beam_width=width)

    def search_loop():
        with torch.inference_mode():
            for images, _ in data:
                model.beam_search(images, width)
        torch.cuda.synchronize()

    def host_loop():
        correct = 0
        with torch.inference_mode():
            for images, labels in data:
                beams = tokenizer.decode_beams(model.beam_search(images, width))
                slots = [[(adapter(s), score) for s, score in alts] + [None] * (width - len(alts)) for alts in beams]
                correct += host_beam_metrics(slots, labels)[2].correct
        torch.cuda.synchronize()
        return correct

    def evaluator_loop():
        evaluator.reset()
        for images, labels in data:
            evaluator.update(images, labels)
        return evaluator.result().correct

    loops = {'search': search_loop, 'host': host_loop, 'evaluator': evaluator_loop}
    if args.only:
        loops = {args.only: loops[args.only]}
    out = {'device': torch.cuda.get_device_name(0), 'model': 'parseq (PARSeq-S), synthetic weights', 'precision': 'bf16x3', 'width': width,
           'batch': args.batch, 'batches': args.batches, 'rounds': args.rounds}
    answers, times = {}, {name: [] for name in loops}
    for name, fn in loops.items():               # warm-up: plan creation, allocator, pinned staging
        fn()
        torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in loops.items():
            t0 = time.perf_counter()
            answers[name] = fn()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.batches)
    for name, ms in times.items():
        out[f'{name}_ms_per_batch'] = {'median': round(statistics.median(ms), 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3)}
        out[f'{name}_images_per_s'] = round(args.batch * 1e3 / statistics.median(ms), 1)
    if not args.only:
        assert answers['host'] == answers['evaluator'], answers          # the two paths count the same matches
        r = evaluator.result()
        out['correct'], out['first_hit'], out['miss'] = r.correct, list(r.first_hit[:width]), r.miss
        out['evaluator_over_search'] = round(out['search_ms_per_batch']['median'] / out['evaluator_ms_per_batch']['median'], 4)
        out['evaluator_over_host'] = round(out['host_ms_per_batch']['median'] / out['evaluator_ms_per_batch']['median'], 4)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
