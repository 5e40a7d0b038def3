#!/usr/bin/env python3
"""Times of lexicon matching on the GPU, written as a record to profiles/lexicon_match.md: the matching operator alone
(512 readings against the 90 k-word synthetic list of tools/lexicon_bench.py, N = 8), what bounds it, and the whole call with rescoring beside
`forward` and the trie-constrained search with `refine='score'` at the same batch (B * N = 512 decoder rows).  PARSeq-S, bf16x3, synthetic
weights.  The three model calls run in the same process, one call per timed sample with a synchronisation after it, alternated over
`--rounds` rounds; the median and the spread are reported.  Recognition accuracy is not measured here: the weights are synthetic.

    python tools/lexicon_match_bench.py [--rows 512] [--n 8] [--words 90000] [--rounds 5] [--iters 10] [--out profiles/lexicon_match.md]
"""
from __future__ import annotations

import argparse
import os
import random
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from lexicon_bench import synthetic_words  # noqa: E402
from oracle.synth import CONFIGS, synth_images, synth_state_dict  # noqa: E402

# The kernel's own counts (parseq_amd/csrc/lexicon_match.h), kept with the benchmark: instructions of one column step of the bit-parallel
# distance for a tile of four crops, counted in the gfx950 ISA of the inner block (one ds_read_b128, the byte extraction, four steps), and the
# vector rate of the device: 256 compute units x 4 SIMDs x 16 lanes a clock.
STEP_INSTRUCTIONS_PER_TILE = 82
CROPS_PER_TILE = 4
CHUNK = 64
VALU_LANES_PER_CLOCK = 256 * 4 * 16
CLOCK_HZ = 2.4e9
HBM_BYTES_PER_S = 8e12


def timed(fn, iters: int) -> float:
    """Seconds per call, one call at a time."""
    t0 = time.perf_counter()
    for _ in range(iters):
        fn()
        torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters


def noisy_readings(words, count, seed):
    """`count` readings: a word of the list with zero to three random edits each, as a free reading of a crop of that word would be."""
    rng = random.Random(seed)
    letters = 'etaoinshrdlucmfwypvbgkqjxz'
    out = []
    for _ in range(count):
        w = list(rng.choice(words))
        for _ in range(rng.randint(0, 3)):
            k = rng.randrange(len(w) + 1)
            w = w[:k] + [rng.choice(letters)] * rng.randint(0, 1) + w[k + rng.randint(0, 1):]
        out.append(''.join(w)[:32])
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--rows', type=int, default=512)
    ap.add_argument('--n', type=int, default=8)
    ap.add_argument('--words', type=int, default=90000)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'lexicon_match.md'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('lexicon_match_bench.py measures on the GPU; none is visible')
    from parseq_amd import create_model
    from parseq_amd.lexicon import Lexicon
    cfg = CONFIGS['parseq']
    ml = cfg.max_label_length
    N, rows = args.n, args.rows
    B = rows // N
    m = create_model('parseq', decode_ar=True, refine_iters=1, precision='bf16x3')
    m.model.load_state_dict(synth_state_dict(cfg, 0), strict=True)
    m = m.eval().to('cuda')
    words = synthetic_words(args.words)
    lex = Lexicon(words, m.tokenizer).to('cuda')
    lex.match_table('cuda')
    x = synth_images(rows, cfg, seed=1).to('cuda')

    # ---- the operator alone -------------------------------------------------------------------------------------------
    readings = noisy_readings(words, rows, 3)
    tok = lex.encode_readings(readings)[0].to('cuda')      # token rows: a reading ends at its <eos>

    def op():
        lex.nearest(tok, N, device='cuda')
    _, dist = lex.nearest(tok, N, device='cuda')
    torch.cuda.synchronize()
    near = int((dist[:, 0] <= 3).sum())
    for _ in range(3):
        op()
    torch.cuda.synchronize()
    op_ms = sorted(timed(op, args.iters * 5) * 1e3 for _ in range(args.rounds))
    op_med = statistics.median(op_ms)
    pairs = rows * lex.num_rows
    chars = sum(len(w) for w in words)
    tiles = (rows + CROPS_PER_TILE - 1) // CROPS_PER_TILE
    lane_instr = chars * tiles * STEP_INSTRUCTIONS_PER_TILE                   # one lane-instruction per word character, tile and instruction
    valu_s = lane_instr / (VALU_LANES_PER_CLOCK * CLOCK_HZ)
    chunks = (lex.num_rows + CHUNK - 1) // CHUNK
    table_bytes = lex.rows_nbytes
    hbm_bytes = table_bytes + 2 * rows * chunks * N * 4 + rows * 32 * 4      # the table once (later tiles hit the caches), the partial lists written and read
    l2_bytes = table_bytes * tiles
    mem_s = hbm_bytes / HBM_BYTES_PER_S

    # ---- the whole call beside forward and the constrained search ------------------------------------------------------
    xb = x[:B]

    def run_forward():
        with torch.inference_mode():
            m(xb, ml)

    def run_match():
        with torch.inference_mode():
            m.lexicon_match(xb, lex, N)

    def run_match_plain():
        with torch.inference_mode():
            m.lexicon_match(xb, lex, N, rescore=False)

    def run_trie():
        with torch.inference_mode():
            m.beam_search(xb, N, ml, lexicon=lex, refine='score')
    cases = {'forward': run_forward, 'match': run_match, 'match_norescore': run_match_plain, 'trie_score': run_trie}
    for fn in cases.values():
        fn()
        fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in cases}
    for _ in range(args.rounds):
        for k, fn in cases.items():
            samples[k].append(timed(fn, args.iters) * 1e3)
    med = {k: statistics.median(v) for k, v in samples.items()}
    spread = {k: (min(v), max(v)) for k, v in samples.items()}

    f = med['forward']
    lines = [
        '# Lexicon matching: measured times (tools/lexicon_match_bench.py)',
        '',
        f'PARSeq-S, bf16x3, synthetic weights, one MI355X.  {args.rounds} rounds, the cases alternated, {args.iters} calls per sample (the operator: '
        f'{args.iters * 5}), a synchronisation after every call; median (min .. max) of the samples.  Recognition accuracy of matching against the '
        'trie search is NOT measured: there are no trained weights here, and nothing below says anything about it.',
        '',
        '## The matching operator alone',
        '',
        f'`Lexicon.nearest`: {rows} readings (words of the list with 0 to 3 random edits; {near} of them end within distance 3 of a word) x '
        f'{lex.num_rows} words (the 90 k synthetic list of tools/lexicon_bench.py, {chars / len(words):.2f} characters a word), N = {N}: the match kernel, '
        'the merge kernel and the allocation of its outputs.',
        '',
        '| | |',
        '|---|---|',
        f'| time per call | {op_med:.3f} ms ({op_ms[0]:.3f} .. {op_ms[-1]:.3f}) |',
        f'| word pairs per second | {pairs / (op_med * 1e-3):.3e} ({pairs:.3e} pairs a call) |',
        '',
        '### What bounds it',
        '',
        f'Counted from the kernel, not measured: a column step of the bit-parallel distance is {STEP_INSTRUCTIONS_PER_TILE} vector instructions for a '
        f'tile of {CROPS_PER_TILE} crops (gfx950 ISA of the inner block: one 16-byte LDS read of the masks, the byte extraction, four steps), and it runs '
        f'once per word character and tile: {chars} characters x {tiles} tiles = {lane_instr:.3e} lane-instructions, {valu_s * 1e3:.3f} ms at '
        f'{VALU_LANES_PER_CLOCK} lanes a clock and {CLOCK_HZ / 1e9:.1f} GHz.  Memory: the table is {table_bytes / 1e6:.2f} MB, read from the caches once per '
        f'tile ({l2_bytes / 1e6:.0f} MB of cache traffic); to HBM go the table once and the partial lists written and read, {hbm_bytes / 1e6:.1f} MB = '
        f'{mem_s * 1e3:.4f} ms at {HBM_BYTES_PER_S / 1e12:.0f} TB/s.  The vector-instruction bound is {valu_s / max(mem_s, 1e-12):.0f} x the memory bound: '
        f'the kernel is bound by vector integer instructions, and the measured call is {op_med / (valu_s * 1e3):.2f} x that bound (the selection, the '
        'merge, divergence between words of different lengths and the launches are the rest).',
        '',
        '## The whole call',
        '',
        f'B = {B} crops, N = {N}: B * N = {rows} decoder rows, the plan the search fills too.  `refine_iters = 1`, AR decoding.',
        '',
        '| call | ms | against `forward` |',
        '|---|---|---|',
    ]
    names = {'forward': f'`forward` (B = {B})', 'match': f'`lexicon_match(n={N})`, rescored', 'match_norescore': f'`lexicon_match(n={N}, rescore=False)`',
             'trie_score': f"`beam_search(lexicon=, beam_width={N}, refine='score')`"}
    for k in cases:
        lines.append(f'| {names[k]} | {med[k]:.3f} ({spread[k][0]:.3f} .. {spread[k][1]:.3f}) | {med[k] / f:.2f} x |')
    lines += [
        '',
        '## Table bytes',
        '',
        f'| packed word table ({lex.num_rows} rows x 32 bytes, + 4 bytes a row of word ids) | {(table_bytes + 4 * lex.num_rows) / 1e6:.2f} MB |',
        '|---|---|',
        f'| trie table ({lex.num_nodes} nodes x {lex.num_classes} classes x 4 bytes) | {lex.nbytes / 1e6:.1f} MB |',
        '',
    ]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as fh:
        fh.write('\n'.join(lines))
    print('\n'.join(lines))


if __name__ == '__main__':
    main()
