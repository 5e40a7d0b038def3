#!/usr/bin/env python3
"""Choose the fusion weights of a weighted automaton (DESIGN.md sections 24 and 26) on labelled data: `alpha` (--lm-weight) and `beta`
(--char-bonus) over a grid, one `BeamEvaluator` pass over every dataset under --data_root per grid point.

    tools/tune_fusion.py <checkpoint> --data_root DIR (--lm FILE [--lm-order N] | --lexicon FILE --priors) --beam W \\
        --alphas a0:a1:n --betas b0:b1:n [--out grid.json] [--batch_size 512] [name:type=value ...]

`a0:a1:n` is n values from a0 to a1, evenly spaced (n = 1: a0).  Prints the grid of accuracy and 1 - NED (of the first hypothesis, over all
samples of all datasets) and the best point: by accuracy, then 1 - NED, then the smallest alpha, then the smallest beta.  Writes the grid as
JSON.  Every grid point runs the whole forward again: the encoder's output is not reused across points.  The automaton is built once.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def parse_range(text: str):
    """`a0:a1:n` as a list of n floats."""
    try:
        a0, a1, n = text.split(':')
        a0, a1, n = float(a0), float(a1), int(n)
        if n < 1:
            raise ValueError
    except ValueError:
        raise argparse.ArgumentTypeError(f'expected a0:a1:n with n >= 1, got {text!r}') from None
    return [a0 + (a1 - a0) * i / (n - 1) for i in range(n)] if n > 1 else [a0]


def choose(grid):
    """The best point of `grid` (dicts with accuracy, ned, alpha, beta): accuracy, then 1 - NED, then the smallest alpha, then the smallest beta."""
    return min(grid, key=lambda p: (-p['accuracy'], -p['ned'], p['alpha'], p['beta']))


def evaluate_point(model, batches, automaton, beam, alpha, beta):
    """One pass over `batches` [(images, labels)] at (alpha, beta): the `BeamEvalResult` of all of them together."""
    from parseq_amd.evaluate import BeamEvaluator
    evaluator = BeamEvaluator(model, beam_width=beam, automaton=automaton, alpha=alpha, beta=beta)
    for images, labels in batches:
        evaluator.update(images, labels)
    return evaluator.result()


def load_batches(model, data_root, batch_size):
    """Every dataset under `data_root` (test.py's layout and label filter) as uint8 batches on the device, loaded once for all grid points."""
    import numpy as np
    import torch
    from PIL import Image
    from parseq_amd.data import read_gt
    from parseq_amd.preprocess import resize_batch
    hp = model.hparams
    batches = []
    for name in sorted(d for d in os.listdir(data_root) if os.path.isfile(os.path.join(data_root, d, 'gt.txt'))):
        samples = read_gt(os.path.join(data_root, name), hp.charset_test, hp.max_label_length)
        for at in range(0, len(samples), batch_size):
            chunk = samples[at:at + batch_size]
            crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(model.device) for f, _ in chunk]
            batches.append((resize_batch(crops, tuple(hp.img_size)), [label for _, label in chunk]))
    return batches


def main(argv=None):
    import string
    import torch
    from parseq_amd import load_from_checkpoint, parse_model_args
    from parseq_amd.search_flags import add_evaluation_flags, build_automaton, resolve_evaluation_flags
    parser = argparse.ArgumentParser()
    parser.add_argument('checkpoint', help="Model checkpoint (or 'pretrained=<model_id>')")
    parser.add_argument('--data_root', default='data')
    parser.add_argument('--batch_size', type=int, default=512)
    parser.add_argument('--cased', action='store_true', default=False)
    parser.add_argument('--punctuation', action='store_true', default=False)
    parser.add_argument('--device', default='cuda')
    parser.add_argument('--alphas', type=parse_range, required=True, metavar='a0:a1:n')
    parser.add_argument('--betas', type=parse_range, required=True, metavar='b0:b1:n')
    parser.add_argument('--out', default=None, help='Where the grid goes as JSON (default: <checkpoint>.fusion.json)')
    add_evaluation_flags(parser)
    args, unknown = parser.parse_known_args(argv)
    kwargs = parse_model_args(unknown)
    if args.lm_weight is not None or args.char_bonus is not None:
        parser.error('--lm-weight and --char-bonus are what the grid is over: give --alphas and --betas')
    flags = resolve_evaluation_flags(parser, args)
    if flags is None or flags.kind is None:
        parser.error('the fusion weights belong to a weighted automaton: give --lm FILE, --lexicon FILE --priors or --pattern REGEX')
    charset_test = string.digits + string.ascii_lowercase + (string.ascii_uppercase if args.cased else '') + (string.punctuation if args.punctuation else '')
    model = load_from_checkpoint(args.checkpoint, charset_test=charset_test, **kwargs).eval().to(args.device)
    automaton = build_automaton(model, flags.kind, args)
    with torch.inference_mode():
        batches = load_batches(model, args.data_root, args.batch_size)
    if not batches:
        raise SystemExit(f'no dataset (a sub-directory with a gt.txt) under {args.data_root!r}')
    grid = []
    for alpha in args.alphas:
        for beta in args.betas:
            r = evaluate_point(model, batches, automaton, flags.beam, alpha, beta)
            grid.append(dict(alpha=alpha, beta=beta, num_samples=r.num_samples, accuracy=100 * r.accuracy, ned=100 * (1 - r.ned),
                             hit=100 * r.hit_at(flags.beam), oracle_ned=100 * (1 - r.oracle_ned), mrr=r.mrr))
    best = choose(grid)
    print(f'accuracy / 1 - NED over {grid[0]["num_samples"]} samples, beam {flags.beam}; rows: alpha, columns: beta')
    print('| alpha \\ beta | ' + ' | '.join(f'{b:g}' for b in args.betas) + ' |')
    print('|---:|' + '---:|' * len(args.betas))
    for i, alpha in enumerate(args.alphas):
        cells = grid[i * len(args.betas):(i + 1) * len(args.betas)]
        print(f'| {alpha:g} | ' + ' | '.join(f'{p["accuracy"]:.2f} / {p["ned"]:.2f}' for p in cells) + ' |')
    print(f'best: --lm-weight {best["alpha"]:g} --char-bonus {best["beta"]:g}  (accuracy {best["accuracy"]:.2f}, 1 - NED {best["ned"]:.2f})')
    out = args.out or args.checkpoint + '.fusion.json'
    with open(out, 'w') as fh:
        json.dump(dict(kind=flags.kind, beam=flags.beam, alphas=args.alphas, betas=args.betas, grid=grid, best=best), fh, indent=1)
    return grid, best


if __name__ == '__main__':
    main()
