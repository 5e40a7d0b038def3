#!/usr/bin/env python3
"""Time of a beam search over a weighted automaton against the unconstrained and the lexicon-constrained search, at
tools/lexicon_bench.py's shapes: PARSeq-S, bf16x3, synthetic weights, W in {4, 8, 16} at B * W = 512 decoder rows, max_length given so all
26 steps run.  Four searches in one process: `parseq_forward_beam`, `parseq_forward_beam_lexicon` under the 90 k-word synthetic lexicon,
`parseq_forward_beam_automaton` under the weighted trie of the same words (synthetic counts) and under a trigram table counted from them.
One search per timed call (a synchronisation after each), the configurations alternated over `--rounds` rounds, the median and the
spread reported.

    python tools/automaton_bench.py [--rows 512] [--rounds 5] [--iters 10] [--words 90000] [--out automaton_bench.json]
    python tools/automaton_bench.py --profile 4 [--words 90000]     # one warm-up + one search over the weighted trie, for a kernel trace
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from lexicon_bench import WIDTHS, synthetic_words, timed  # noqa: E402
from oracle.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=512)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--words', type=int, default=90000)
    ap.add_argument('--out', default=None)
    ap.add_argument('--profile', type=int, default=0)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('automaton_bench.py measures on the GPU; none is visible')
    from parseq_amd import create_model
    from parseq_amd.automaton import Automaton
    from parseq_amd.lexicon import Lexicon
    cfg = CONFIGS['parseq']
    steps, ml = cfg.max_label_length + 1, cfg.max_label_length
    x = synth_images(args.rows, cfg, seed=1).to('cuda')
    m = create_model('parseq', decode_ar=True, refine_iters=0, precision='bf16x3')
    m.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    m = m.eval().to('cuda')

    words = synthetic_words(args.words)
    rng = random.Random(1)
    counts = [int(1000 / (1 + rng.random() * k)) for k in range(len(words))]      # a long tail: a few frequent words, most rare

    def built(make):
        t0 = time.perf_counter()
        table = make().to('cuda')
        torch.cuda.synchronize()
        return table, time.perf_counter() - t0

    def search(W, **kw):
        def run():
            with torch.inference_mode():
                m.beam_search(x[:args.rows // W], W, ml, **kw)
        return run

    trie, trie_s = built(lambda: Automaton.from_lexicon(words, counts, m.tokenizer))
    if args.profile:
        for _ in range(2):
            search(args.profile, automaton=trie, alpha=0.5, beta=0.1)()
            torch.cuda.synchronize()
        return
    lex, lex_s = built(lambda: Lexicon(words, m.tokenizer))
    lm, lm_s = built(lambda: Automaton.ngram(words, 3, m.tokenizer))

    cases = {}
    for W in WIDTHS:
        cases[f'free_w{W}'] = search(W)
        cases[f'lex_w{W}'] = search(W, lexicon=lex)
        cases[f'trie_w{W}'] = search(W, automaton=trie, alpha=0.5, beta=0.1)
        cases[f'lm_w{W}'] = search(W, automaton=lm, alpha=0.5, beta=0.1)
    for fn in cases.values():                 # every shape warm
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.rounds):              # alternate the configurations: other people's work shares the host
        for k, fn in cases.items():
            samples[k].append(timed(fn, args.iters) * 1e3)
    med = {k: statistics.median(v) for k, v in samples.items()}
    out = {'rows': args.rows, 'steps': steps, 'rounds': args.rounds, 'iters': args.iters, 'precision': 'bf16x3', 'words': len(words),
           'tables': {'lexicon': {'states': lex.num_nodes, 'table_mb': round(lex.nbytes / 1e6, 1), 'build_and_upload_s': round(lex_s, 2)},
                      'weighted_trie': {'states': trie.num_states, 'table_mb': round(trie.nbytes / 1e6, 1), 'build_and_upload_s': round(trie_s, 2)},
                      'trigram': {'states': lm.num_states, 'table_mb': round(lm.nbytes / 1e6, 3), 'build_and_upload_s': round(lm_s, 2)}},
           'ms_median': {k: round(v, 3) for k, v in med.items()},
           'ms_min_max': {k: [round(min(v), 3), round(max(v), 3)] for k, v in samples.items()}, 'widths': {}}
    for W in WIDTHS:
        base = med[f'lex_w{W}']
        spread = (max(samples[f'lex_w{W}']) - min(samples[f'lex_w{W}'])) / base
        out['widths'][W] = {'batch': args.rows // W, 'lexicon_ms': round(base, 3), 'lexicon_spread': round(spread, 3),
                            'free_over_lexicon': round(med[f'free_w{W}'] / base, 3), 'trie_over_lexicon': round(med[f'trie_w{W}'] / base, 3),
                            'lm_over_lexicon': round(med[f'lm_w{W}'] / base, 3)}
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as fh:
            fh.write(line + '\n')


if __name__ == '__main__':
    main()
