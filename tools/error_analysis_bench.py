#!/usr/bin/env python3
"""What the error analysis costs per batch: PARSeq-S, bf16x3, batch 512, AR + 1 refinement, synthetic weights — the
`Evaluator` loop of tools/eval_bench.py three ways over the same batches, alternated over `--rounds` rounds after a warm-up pass of each;
median (min .. max) of the rounds:

  plain     `Evaluator(model).update(images, labels)` per batch, then `result()`: forward and metrics on the device, no analysis
  errors    `Evaluator(model, errors=ErrorAnalysis(model))`: the same, plus `parseq_eval_errors` on the ids the metrics kernel wrote; the
            tables are copied once, at the end
  host      the same `Evaluator`, the analysis done the way it had to be done before: per batch the ids and lengths are copied to the host
            and every sample goes through the adapter and `host_edit_script` (what `ErrorAnalysis` itself runs on its host path)

    python tools/error_analysis_bench.py [--batch 512] [--batches 20] [--rounds 5] [--out profiles/error_analysis.json]
    python tools/error_analysis_bench.py --only errors        # one loop alone, for a kernel trace

The labels are the model's own readings, every other one edited (a substitution, a deletion or an insertion), so that every operation
occurs; recognition accuracy is not measured: the weights are synthetic.
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

from oracle.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402


class HostAnalysis:
    """What `ErrorAnalysis` replaces, behind the same two methods `Evaluator` calls: a copy of ids and lengths per batch, then Python."""

    def __init__(self, model, symbols):
        from parseq_amd.evaluate import _CONFUSION
        self.model, self.index = model, {ch: i for i, ch in enumerate(symbols)}
        self.size, self.labels = _CONFUSION + (len(symbols) + 2) ** 2, None
        self.reset()

    def reset(self):
        self.words = np.zeros(self.size, dtype=np.int64)

    def update_ids(self, ids, lengths, _encoded):
        from parseq_amd.evaluate import _accumulate_script, host_edit_script
        tokenizer, adapter = self.model.tokenizer, self.model.charset_adapter
        for row, k, gt in zip(ids.cpu().numpy(), lengths.cpu().tolist(), self.labels):
            pred = adapter(tokenizer._ids2tok(row[:k].tolist()))
            _accumulate_script(self.words, self.index, host_edit_script(pred, gt), pred, gt)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--batch', type=int, default=512)
    ap.add_argument('--batches', type=int, default=20)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--only', choices=['plain', 'errors', 'host'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    from parseq_amd import create_model
    from parseq_amd.evaluate import ErrorAnalysis, Evaluator
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
        for p in preds:
            s = list(model.charset_adapter(p)) or ['a']
            if rng.random() < 0.5:
                what, at = int(rng.integers(3)), int(rng.integers(len(s)))
                if what == 0:
                    s[at] = charset[int(rng.integers(len(charset)))]
                elif what == 1 and len(s) > 1:
                    del s[at]
                else:
                    s.insert(at, charset[int(rng.integers(len(charset)))])
            labels.append(''.join(s))
        data.append((images, labels))
    errors = ErrorAnalysis(model)
    host = HostAnalysis(model, errors.symbols)
    evaluators = {'plain': Evaluator(model), 'errors': Evaluator(model, errors=errors), 'host': Evaluator(model, errors=host)}

    def loop(name):
        ev = evaluators[name]

        def run():
            ev.reset()
            for images, labels in data:
                host.labels = labels
                ev.update(images, labels)
            totals = ev.result()
            if name == 'errors':
                return totals.correct, errors.result()._words()
            return totals.correct, host.words.copy() if name == 'host' else None
        return run

    loops = {name: loop(name) for name in evaluators if args.only in (None, name)}
    out = {'device': torch.cuda.get_device_name(0), 'model': 'parseq (PARSeq-S), synthetic weights', 'precision': 'bf16x3',
           'mode': 'AR + 1 refinement, max_length None', 'batch': args.batch, 'batches': args.batches, 'rounds': args.rounds}
    answers, times = {}, {name: [] for name in loops}
    for fn in loops.values():                    # warm-up: plan creation, allocator, pinned staging, code objects
        fn()
        torch.cuda.synchronize()
    for _ in range(args.rounds):
        for name, fn in loops.items():
            t0 = time.perf_counter()
            answers[name] = fn()                 # ends in result(): a copy from the device, so the batches are done
            times[name].append((time.perf_counter() - t0) * 1e3 / args.batches)
    for name, ms in times.items():
        out[f'{name}_ms_per_batch'] = {'median': round(statistics.median(ms), 3), 'min': round(min(ms), 3), 'max': round(max(ms), 3)}
        out[f'{name}_images_per_s'] = round(args.batch * 1e3 / statistics.median(ms), 1)
    if not args.only:
        assert answers['plain'][0] == answers['errors'][0] == answers['host'][0], [a[0] for a in answers.values()]
        assert np.array_equal(answers['errors'][1], answers['host'][1])          # the device's tables are the host loop's
        r = errors.result()
        out.update(correct=answers['errors'][0], matches=r.matches, substitutions=r.substitutions, insertions=r.insertions, deletions=r.deletions)
        out['errors_over_plain'] = round(out['errors_ms_per_batch']['median'] / out['plain_ms_per_batch']['median'], 4)
        out['errors_over_host'] = round(out['errors_ms_per_batch']['median'] / out['host_ms_per_batch']['median'], 4)
    print(json.dumps(out))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            json.dump(out, f, indent=1)


if __name__ == '__main__':
    main()
