#!/usr/bin/env python3
"""Time of a lexicon-constrained beam search against the unconstrained one: PARSeq-S, bf16x3, synthetic weights,
W in {4, 8, 16} at B * W = 512 decoder rows, max_length given so all 26 steps run, under a 1 k-word and a 90 k-word synthetic lexicon (one
shared trie, root 0).  Both searches run in the same process: one search per timed call (a synchronisation after each), the
configurations alternated over `--rounds` rounds, the median and the spread reported.

    python tools/lexicon_bench.py [--rows 512] [--rounds 5] [--iters 10] [--out lexicon_bench.json]
    python tools/lexicon_bench.py --profile 4 [--words 90000]     # one warm-up + one constrained search of that width, for a kernel trace
"""
from __future__ import annotations

import argparse
import json
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402

WIDTHS = (4, 8, 16)
SIZES = (1000, 90000)


def synthetic_words(n: int, seed: int = 0):
    """n distinct lower-case words of 3 to 12 letters, letter frequencies skewed so that prefixes are shared as in a real word list."""
    rng = random.Random(seed)
    letters = 'etaoinshrdlucmfwypvbgkqjxz'
    weights = [1.0 / (k + 2) for k in range(len(letters))]
    words = set()
    while len(words) < n:
        words.add(''.join(rng.choices(letters, weights, k=rng.randint(3, 12))))
    return sorted(words)


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
    ap.add_argument('--words', type=int, default=SIZES[-1], help='lexicon size of --profile')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lexicon_bench.py measures on the GPU; none is visible')
    from parseq_amd import create_model
    from parseq_amd.lexicon import Lexicon
    cfg = CONFIGS['parseq']
    steps, ml = cfg.max_label_length + 1, cfg.max_label_length
    x = synth_images(args.rows, cfg, seed=1).to('cuda')
    m = create_model('parseq', decode_ar=True, refine_iters=0, precision='bf16x3')
    m.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    m = m.eval().to('cuda')

    def lexicon(n):
        t0 = time.perf_counter()
        lex = Lexicon(synthetic_words(n), m.tokenizer).to('cuda')
        torch.cuda.synchronize()
        return lex, time.perf_counter() - t0

    def search(W, lex=None):
        def run():
            with torch.inference_mode():
                m.beam_search(x[:args.rows // W], W, ml, lexicon=lex)
        return run

    if args.profile:
        lex, _ = lexicon(args.words)
        for _ in range(2):
            search(args.profile, lex)()
            torch.cuda.synchronize()
        return

    lexicons = {n: lexicon(n) for n in SIZES}
    cases = {}
    for W in WIDTHS:
        cases[f'free_w{W}'] = search(W)
        for n, (lex, _) in lexicons.items():
            cases[f'lex{n}_w{W}'] = search(W, lex)
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
           'lexicons': {n: {'nodes': lex.num_nodes, 'table_mb': round(lex.nbytes / 1e6, 1), 'build_and_upload_s': round(t, 2)}
                        for n, (lex, t) in lexicons.items()},
           'ms_median': {k: round(v, 3) for k, v in med.items()},
           'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in samples.items()}, 'widths': {}}
    for W in WIDTHS:
        free = med[f'free_w{W}']
        out['widths'][W] = {'batch': args.rows // W, 'free_ms': round(free, 3),
                            **{f'lex{n}_over_free': round(med[f'lex{n}_w{W}'] / free, 3) for n in SIZES}}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
