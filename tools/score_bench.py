#!/usr/bin/env python3
"""Times of scoring given readings on the GPU, written as a record to profiles/score.md: `parseq_score` at 512 crops x
N candidates x K orders for N in {1, 2, 16} and K in {1, 2, 6}, beside `forward` on the same 512 crops, and the bare `Evaluator` loop on
512 crops with and without `audit=` — PARSeq-S, bf16x3, synthetic weights, uint8 crops, candidates of 1 to 25 random characters.  The calls
run in one process, one call per timed sample with a synchronisation after it, alternated over `--rounds` rounds; the median and the spread
are reported.  The worst errors the GPU tests print (tests/test_score.py, per summed term) are passed back in with `--parity` when the record
is written; what was not passed is written as "not measured".  The accuracy of an audit is not measured: the weights are synthetic.

    python tools/score_bench.py [--rounds 3] [--iters 5] [--parity 'fp32 1.2e-5, bf16x3 3.4e-5, bf16 2.1e-3'] [--out profiles/score.md]
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

from oracle.synth import CONFIGS, synth_state_dict  # noqa: E402

CROPS = 512
CANDIDATES = (1, 2, 16)
ORDERS = (1, 2, 6)


def timed(fn, iters: int) -> float:
    """Seconds per call, one call at a time."""
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=5)
    ap.add_argument('--parity', default=None, help='the worst |d order score| per term the GPU tests printed, as text for the record')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'score.md'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('score_bench.py measures on the GPU; none is visible')
    from parseq_amd import create_model
    from parseq_amd import score as S
    from parseq_amd.evaluate import Evaluator, LabelAudit
    cfg = CONFIGS['parseq']
    m = create_model('parseq', decode_ar=True, refine_iters=1, precision='bf16x3')
    m.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    m = m.eval().to('cuda')
    T = cfg.max_label_length
    g = torch.Generator().manual_seed(0)
    rng = np.random.default_rng(0)
    images = torch.randint(0, 256, (CROPS, 3, *m.hparams.img_size), dtype=torch.uint8, generator=g).cuda()
    perms = S.parse_orders(max(ORDERS), T, m, seed=0)
    calls = {'forward': lambda: m(images)}
    for N in CANDIDATES:
        rows = np.full((CROPS, N, T + 1), m.pad_id, dtype=np.int32)
        for b in range(CROPS):
            for j in range(N):
                n = int(rng.integers(1, T + 1))
                rows[b, j, :n] = rng.integers(1, len(m.tokenizer) - 2, size=n)
                rows[b, j, n] = m.eos_id
        cand = torch.from_numpy(rows).cuda()
        for K in ORDERS:
            masks = S.query_masks(perms[:K]).cuda()
            calls[(N, K)] = lambda cand=cand, masks=masks: m.model.score(m.tokenizer, images, cand, masks, 0)
    letters = np.array(list('0123456789abcdefghijklmnopqrstuvwxyz'))
    labels = [''.join(rng.choice(letters, size=int(rng.integers(1, 11)))) for _ in range(CROPS)]
    plain, audited = Evaluator(m), Evaluator(m, audit=LabelAudit(m))

    def evaluate(ev):
        ev.reset()
        ev.update(images, labels)
    calls['evaluator'] = lambda: evaluate(plain)
    calls['evaluator+audit'] = lambda: evaluate(audited)
    with torch.inference_mode():
        for fn in calls.values():      # warm-up: plans, code objects, allocator blocks
            for _ in range(2):
                fn()
        torch.cuda.synchronize()
        samples = {key: [] for key in calls}
        for _ in range(args.rounds):
            for key, fn in calls.items():
                samples[key].append(timed(fn, args.iters))

    def cell(values):
        return f'{1e3 * statistics.median(values):.3f} ms ({1e3 * min(values):.3f} .. {1e3 * max(values):.3f})'

    lines = ['# Scoring given readings: what a call costs', '',
             f'`tools/score_bench.py`, PARSeq-S, bf16x3, synthetic weights, {CROPS} uint8 crops, candidates of 1 to {T} random characters (L = {T + 1});',
             f'{args.rounds} rounds of {args.iters} calls each, one call at a time with a synchronisation after it, all calls alternated; median (least ..',
             'greatest round).  A `parseq_score` call is: encode the crops once, replicate the memory N-fold and project it, then per order one',
             'decoder pass over all 512 N rows and the row kernel, then the rank kernel.', '',
             f'`forward` (AR + 1 refinement) on the same {CROPS} crops: {cell(samples["forward"])}', '',
             '| N candidates | rows | K = 1 | K = 2 | K = 6 |', '|---|---|---|---|---|']
    for N in CANDIDATES:
        lines.append(f'| {N} | {CROPS * N} | ' + ' | '.join(cell(samples[(N, K)]) for K in ORDERS) + ' |')
    ev, au = samples['evaluator'], samples['evaluator+audit']
    lines += ['', f'## The `Evaluator` loop, one `update` of {CROPS} crops', '',
              '| | time |', '|---|---|', f'| `Evaluator(model)` | {cell(ev)} |', f"| `Evaluator(model, audit=LabelAudit(model))` (N = 2, 'forward', L = {T + 1}) | {cell(au)} |",
              f'| difference of the medians | {1e3 * (statistics.median(au) - statistics.median(ev)):+.3f} ms |', '',
              '## Parity', '',
              f'Worst |d order score| per summed term against the float64 restatement on the CPU oracle (tests/test_score.py): {args.parity or "not measured"}.',
              'The bound per term is 2 x the logits gate of the precision (1e-3 for fp32 and bf16x3, 6e-2 for bf16) + 4e-5.', '',
              'Accuracy of the audit (does a high suspicion find wrong labels): not measured (no trained weights).', '']
    with open(args.out, 'w', encoding='utf-8') as fh:
        fh.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
