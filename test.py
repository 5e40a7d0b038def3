#!/usr/bin/env python3
"""Accuracy / 1 - NED / confidence / label-length table over labelled image sets — the command line of the reference's
`test.py:71-92` on the MI355X backend.

    ./test.py pretrained=parseq --data_root data [--batch_size 512] [--cased] [--punctuation] [--rotation 90] [name:type=value ...]
    ./test.py path/to/lightning.ckpt --data_root data refine_iters:int=2

A dataset is a sub-directory of `--data_root` that holds a `gt.txt`: one sample per line, the image path (relative to that
sub-directory) and the label separated by the first run of whitespace — the input format of the reference's
`tools/create_lmdb_dataset.py:40-45`.  The reference reads LMDB archives made from such files; LMDB is out of scope here (the
data layer is not part of this repository), so the archives' source form is read directly.  Every such
sub-directory is evaluated, in name order, and one table with a `Combined` row is printed and written to `<checkpoint>.log.txt`.

Labels go through the reference dataset's filter (`strhub/data/dataset.py:105-117`): whitespace removed, NFKD-normalised to ASCII,
dropped if longer than `max_label_length`, mapped into the test charset, dropped if nothing is left.  Images are decoded on the
host (PIL) and uploaded as they are; the rotation of `--rotation` (`img.rotate(rotation, expand=True)` of the reference transform,
`strhub/data/module.py:72-73`), the bicubic resize, the model and the metrics (parseq_amd.evaluate.Evaluator, one per dataset) run on
the device with no copy back until a dataset is done.
"""
import argparse
import os
import string
import sys
from dataclasses import dataclass
from typing import List, Tuple

import numpy as np
import torch
from PIL import Image

from parseq_amd import load_from_checkpoint, parse_model_args
from parseq_amd.data import parse_gt_line, preprocess_label, read_gt  # noqa: F401  (the first two keep their names here)
from parseq_amd.evaluate import Evaluator
from parseq_amd.preprocess import resize_batch
from parseq_amd.tokenizer import CharsetAdapter  # noqa: F401


@dataclass
class Result:
    dataset: str
    num_samples: int
    accuracy: float
    ned: float
    confidence: float
    label_length: float


def read_dataset(root: str, name: str, charset_test: str, max_label_length: int) -> List[Tuple[str, str]]:
    """[(image file, label)] of the samples of `root/name/gt.txt` that survive the label filter (parseq_amd.data.read_gt: the filter is
    the one the training loader applies with `charset_train`)."""
    return read_gt(os.path.join(root, name), charset_test, max_label_length)


def find_datasets(root: str) -> List[str]:
    return sorted(d for d in os.listdir(root) if os.path.isfile(os.path.join(root, d, 'gt.txt')))


def load_crops(files, device):
    return [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]


def evaluate_dataset(model, root: str, name: str, batch_size: int = 512, rotation: int = 0) -> Result:
    hp = model.hparams
    samples = read_dataset(root, name, hp.charset_test, hp.max_label_length)
    evaluator = Evaluator(model)
    for at in range(0, len(samples), batch_size):
        chunk = samples[at:at + batch_size]
        images = resize_batch(load_crops([f for f, _ in chunk], model.device), tuple(hp.img_size), rotation=rotation)      # uint8 [N, 3, H, W]
        evaluator.update(images, [label for _, label in chunk])
    r = evaluator.result()
    n = r.num_samples
    if not n:
        return Result(name, 0, 0.0, 0.0, 0.0, 0.0)
    return Result(name, n, 100 * r.correct / n, 100 * (1 - r.ned / n), 100 * r.confidence / n, r.label_length / n)


def print_results_table(results: List[Result], file=None) -> None:
    """The reference's Markdown table (test.py:40-66): one row per dataset, then the sample-weighted `Combined` row."""
    width = max([len(r.dataset) for r in results] + [len('Combined')])
    heads = ('# samples', 'Accuracy', '1 - NED', 'Confidence', 'Label Length')

    def row(r: Result) -> str:
        cells = (f'{r.num_samples:d}', f'{r.accuracy:.2f}', f'{r.ned:.2f}', f'{r.confidence:.2f}', f'{r.label_length:.2f}')
        return ' | '.join(['| ' + r.dataset.ljust(width)] + [c.rjust(len(h)) for c, h in zip(cells, heads)]) + ' |'

    print(' | '.join(['| ' + 'Dataset'.ljust(width)] + list(heads)) + ' |', file=file)
    print('|:' + '-' * width + ':|' + '|'.join('-' * (len(h) + 1) + ':' for h in heads) + '|', file=file)
    total = sum(r.num_samples for r in results)
    for r in results:
        print(row(r), file=file)

    def mean(field: str) -> float:
        return sum(r.num_samples * getattr(r, field) for r in results) / total if total else 0.0
    print('|-' + '-' * width + '-|' + '|'.join('-' * (len(h) + 2) for h in heads) + '|', file=file)
    print(row(Result('Combined', total, mean('accuracy'), mean('ned'), mean('confidence'), mean('label_length'))), file=file)


@torch.inference_mode()
def main(argv=None) -> List[Result]:
    parser = argparse.ArgumentParser()
    parser.add_argument('checkpoint', help="Model checkpoint (or 'pretrained=<model_id>')")
    parser.add_argument('--data_root', default='data')
    parser.add_argument('--batch_size', type=int, default=512)
    parser.add_argument('--cased', action='store_true', default=False, help='Cased comparison')
    parser.add_argument('--punctuation', action='store_true', default=False, help='Check punctuation')
    parser.add_argument('--rotation', type=int, default=0, help='Angle of rotation (counter clockwise) in degrees.')
    parser.add_argument('--device', default='cuda')
    args, unknown = parser.parse_known_args(argv)
    kwargs = parse_model_args(unknown)

    charset_test = string.digits + string.ascii_lowercase
    if args.cased:
        charset_test += string.ascii_uppercase
    if args.punctuation:
        charset_test += string.punctuation
    kwargs['charset_test'] = charset_test
    print(f'Additional keyword arguments: {kwargs}')

    model = load_from_checkpoint(args.checkpoint, **kwargs).eval().to(args.device)
    results = [evaluate_dataset(model, args.data_root, name, args.batch_size, args.rotation) for name in find_datasets(args.data_root)]
    if not results:
        raise SystemExit(f'no dataset (a sub-directory with a gt.txt) under {args.data_root!r}')
    with open(args.checkpoint + '.log.txt', 'w') as log:
        for out in (log, sys.stdout):
            print_results_table(results, out)
    return results


if __name__ == '__main__':
    main()
