#!/usr/bin/env python3
"""What the evaluation metrics cost per batch: PARSeq-S, bf16x3, batch 512, AR + 1 refinement, synthetic
weights.  Over the same batches, after a warm-up pass of each loop:

  forward      `model(images)` back to back, one synchronisation at the end
  test_step    `model.test_step((images, labels), i)` per batch — forward, ids and lengths to the host, the per-sample Python loop
  evaluator    `Evaluator.update(images, labels)` per batch, then `result()` — forward and metrics on the device, one copy at the end

    python tools/eval_bench.py [--batch 512] [--batches 20] [--out profiles/eval_step.json]
    python tools/eval_bench.py --only evaluator        # one loop alone, for a kernel / memory-copy trace
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--only', choices=['forward', 'test_step', 'evaluator'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from parseq_amd import create_model
    from parseq_amd.evaluate import Evaluator
    cfg = CONFIGS['parseq']
    model = create_model('parseq', precision='bf16x3')
    model.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    model = model.eval().to('cuda')
    rng = np.random.default_rng(0)
    charset = model.hparams.charset_test
    data = []
    for i in range(args.batches):
        images = synth_images(args.batch, cfg, seed=100 + i).to('cuda')
        with torch.inference_mode():
            preds, _ = model.tokenizer.read(model(images))
        labels = []
        for p in preds:                      # the model's own reading, every other one edited: matches and misses, realistic lengths
            s = list(model.charset_adapter(p)) or ['a']
            if rng.random() < 0.5:
                s[int(rng.integers(len(s)))] = charset[int(rng.integers(len(charset)))]
            labels.append(''.join(s))
        data.append((images, labels))
    evaluator = Evaluator(model)

    def forward_loop():
        with torch.inference_mode():
            for images, _ in data:
                model(images)
        torch.cuda.synchronize()

    def test_step_loop():
        total = 0
        for i, (images, labels) in enumerate(data):
            total += model.test_step((images, labels), i)['output'].correct
        torch.cuda.synchronize()
        return total

    def evaluator_loop():
        evaluator.reset()
        for images, labels in data:
            evaluator.update(images, labels)
        return evaluator.result().correct

    loops = {'forward': forward_loop, 'test_step': test_step_loop, 'evaluator': evaluator_loop}
    out = {'device': torch.cuda.get_device_name(0), 'model': 'parseq (PARSeq-S), synthetic weights', 'precision': 'bf16x3',
           'mode': 'AR + 1 refinement, max_length None', 'batch': args.batch, 'batches': args.batches}
    answers = {}
    for name, fn in loops.items():
        if args.only and name != args.only:
            continue
        fn()                                 # warm-up: plan creation, allocator, pinned staging
        torch.cuda.synchronize()
        best = float('inf')
        for _ in range(3):
            t0 = time.perf_counter()
            answers[name] = fn()
            best = min(best, time.perf_counter() - t0)
        out[f'{name}_images_per_s'] = round(args.batch * args.batches / best, 1)
        out[f'{name}_ms_per_batch'] = round(best * 1e3 / args.batches, 3)
    if not args.only:
        assert answers['test_step'] == answers['evaluator'], answers          # the two paths count the same matches
        out['correct'] = answers['evaluator']
        out['evaluator_over_forward'] = round(out['evaluator_images_per_s'] / out['forward_images_per_s'], 4)
        out['evaluator_over_test_step'] = round(out['evaluator_images_per_s'] / out['test_step_images_per_s'], 4)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
