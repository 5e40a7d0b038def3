#!/usr/bin/env python3
"""Accuracy / 1 - NED / confidence / label-length table over labelled image sets — the command line of the reference's
`test.py:71-92` on the MI355X backend.

    ./test.py pretrained=parseq --data_root data [--batch_size 512] [--cased] [--punctuation] [--rotation 90] [name:type=value ...]
    ./test.py path/to/lightning.ckpt --data_root data refine_iters:int=2
    ./test.py pretrained=parseq --data_root data --beam 5     a beam search instead of the greedy decode: the table gains Hit@5, Oracle 1 - NED, MRR
    ./test.py pretrained=parseq --data_root data --lexicon words.txt [--beam 8] [--match [N]] [--priors] [--refine-beams score]
    ./test.py pretrained=parseq --data_root data --lm corpus.txt [--lm-order 3] [--lm-weight 0.3] [--char-bonus 0.5]     or --pattern REGEX
    ./test.py pretrained=parseq --data_root data --rotation 180 --auto-rotate flip [--upright-bias 0.1]     read every crop in several quarter turns, score the best
    ./test.py pretrained=parseq --data_root data --analyse [K]     after the table: which characters are confused, dropped or made up, and at which label lengths
    ./test.py pretrained=parseq --data_root data --audit [K] [--orders both] [--length-norm]     after the table: the K labels the model disagrees with most

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

With a search flag (the flags, their composition and their refusals are read.py's: parseq_amd/search_flags.py) a dataset is evaluated by
`parseq_amd.evaluate.BeamEvaluator` instead: the five columns then describe the first hypothesis of the list, and
three more say how often the label is anywhere in the W hypotheses, how near the nearest of them comes, and the mean reciprocal rank.
ONE lexicon / language model / pattern serves every dataset; per-image lexicons (the 50-word protocol of IIIT5k / SVT) are out of scope.
Without a search flag the table and the log are what they were.

With `--auto-rotate MODE` every crop, after `--rotation`, is read in the quarter turns of MODE in one forward, the
view the model reads best is chosen on the device, and its logits go to the same `Evaluator`; one more line per dataset says how many
crops were read turned.  It does not combine with a search flag.  Without the flag nothing changes.

With `--analyse [K]` (K = 20 by default) every dataset's `Evaluator` carries an `ErrorAnalysis`: the edit scripts between
readings and labels are made on the device beside the metrics.  After the table — which, like the log, is what it is without the flag — the
operation totals, the accuracy by label length and the K most frequent confusions, deletions and insertions are printed per dataset and for
all datasets together, and every table is written to `<checkpoint>.errors.json`.  It composes with --cased, --punctuation, --rotation and
--auto-rotate; the analysis of an N-best is out of scope, so with a search flag it is refused.

With `--audit [K]` (K = 20 by default) every dataset's `Evaluator` carries a `LabelAudit`: label and raw reading of every
sample are scored by the model (`parseq_score`, two candidates per crop) beside the metrics.  After the table — which, like the log, is what
it is without the flag — the K samples whose reading the model prefers most over their label are printed per dataset: path, label, reading,
both log-probabilities; only samples whose adapted reading differs from the label are listed.  Everything goes to `<checkpoint>.audit.json`.
It is refused next to a search flag and --auto-rotate.
"""
import argparse
import json
import os
import string
import sys
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch
from PIL import Image

from parseq_amd import load_from_checkpoint, parse_model_args
from parseq_amd.data import parse_gt_line, preprocess_label, read_gt  # noqa: F401  (the first two keep their names here)
from parseq_amd.evaluate import BeamEvaluator, ErrorAnalysis, ErrorReport, Evaluator, LabelAudit
from parseq_amd.preprocess import orientation_views, resize_batch
from parseq_amd.search_flags import (add_analysis_flag, add_audit_flag, add_evaluation_flags, add_orientation_flags, evaluation_width, evaluator_arguments,
                                      orientation_prior, resolve_analysis, resolve_audit, resolve_evaluation_flags, resolve_orientation)
from parseq_amd.tokenizer import CharsetAdapter  # noqa: F401


@dataclass
class Result:
    dataset: str
    num_samples: int
    accuracy: float
    ned: float
    confidence: float
    label_length: float


@dataclass
class BeamTableResult(Result):
    """A row of the extended table: the reference's five columns for the first hypothesis, then the N-best's."""
    hit: float = 0.0             # 100 * share of the images whose label is among the W hypotheses
    oracle_ned: float = 0.0      # 100 * (1 - mean smallest normalised edit distance over the list)
    mrr: float = 0.0             # mean reciprocal rank of the label


def read_dataset(root: str, name: str, charset_test: str, max_label_length: int) -> List[Tuple[str, str]]:
    """[(image file, label)] of the samples of `root/name/gt.txt` that survive the label filter (parseq_amd.data.read_gt: the filter is
    the one the training loader applies with `charset_train`)."""
    return read_gt(os.path.join(root, name), charset_test, max_label_length)


def find_datasets(root: str) -> List[str]:
    return sorted(d for d in os.listdir(root) if os.path.isfile(os.path.join(root, d, 'gt.txt')))


def load_crops(files, device):
    return [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]


class UprightReader:
    """What the unchanged `Evaluator` sees of a model under --auto-rotate: a system whose `forward` takes the views
    [B, K, 3, H, W] of `orientation_views`, chooses every crop's best view on the device (`orient`) and returns the chosen logits.
    `note(angles)` hands over the angles of the next batch's views; `turned` counts, on the device, the crops whose chosen view was not at
    0 degrees."""

    def __init__(self, model, bias: float = 0.0) -> None:
        self._model, self._bias, self._angles = model, bias, None
        self.turned = torch.zeros((), dtype=torch.int64, device=model.device)

    def __getattr__(self, name):
        return getattr(self._model, name)

    def note(self, angles) -> None:
        self._angles = torch.tensor(angles, dtype=torch.int32).to(self._model.device) % 360

    def forward(self, views):
        result = self._model.orient(views, prior=orientation_prior(self._bias, views.shape[1]))
        self.turned += (self._angles.gather(1, result.view.long().unsqueeze(1)) != 0).sum()
        return result.logits


def evaluate_dataset(model, root: str, name: str, batch_size: int = 512, rotation: int = 0, search: Optional[dict] = None, width: int = 0,
                     orient=None, reports: Optional[dict] = None, audit=None, audits: Optional[dict] = None) -> Result:
    """One dataset's row.  `search`: the keywords of `BeamEvaluator` (a beam search or a lexicon match instead of the greedy decode); the row is
    then a `BeamTableResult` whose Hit column counts the first `width` hypotheses per image (`search_flags.evaluation_width`).  `orient`: the
    (mode, bias) of --auto-rotate: every crop — turned by `rotation` first — is read in the views of that mode, the best view is what the
    evaluator scores, and the share of crops read turned is printed under the dataset's name.  `reports`: a dict that receives this dataset's
    `ErrorReport` under `name` (--analyse; greedy evaluation only).  `audit`: the (K, orders, normalize) of --audit; `audits` then receives
    (image files, `AuditReport`) under `name`."""
    hp = model.hparams
    samples = read_dataset(root, name, hp.charset_test, hp.max_label_length)
    system = model if orient is None else UprightReader(model, orient[1])
    errors = ErrorAnalysis(model) if reports is not None and search is None else None
    label_audit = LabelAudit(model, orders=audit[1], normalize=audit[2]) if audit is not None and search is None else None
    if search is not None:
        evaluator = BeamEvaluator(model, **search)
    else:
        evaluator = Evaluator(system, errors=errors) if label_audit is None else Evaluator(system, errors=errors, audit=label_audit)
    for at in range(0, len(samples), batch_size):
        chunk = samples[at:at + batch_size]
        crops = load_crops([f for f, _ in chunk], model.device)
        if orient is None:
            images = resize_batch(crops, tuple(hp.img_size), rotation=rotation)      # uint8 [N, 3, H, W]
        else:
            images, angles = orientation_views(crops, orient[0], tuple(hp.img_size), rotation=rotation)      # uint8 [N, K, 3, H, W]
            system.note(angles)
        evaluator.update(images, [label for _, label in chunk])
    r = evaluator.result()
    if errors is not None:
        reports[name] = errors.result()
    if label_audit is not None:
        audits[name] = ([f for f, _ in samples], label_audit.result())
    if orient is not None:
        turned = int(system.turned)
        print(f'{name}: {turned} of {len(samples)} crops read turned ({100 * turned / max(len(samples), 1):.2f} %)')
    n = r.num_samples
    if search is None:
        row, cells = Result, (100 * r.correct / n, 100 * (1 - r.ned / n), 100 * r.confidence / n, r.label_length / n) if n else ()
    else:
        row, cells = BeamTableResult, (100 * r.accuracy, 100 * (1 - r.ned), 100 * r.confidence, r.label_length, 100 * r.hit_at(width), 100 * (1 - r.oracle_ned), r.mrr)
    return row(name, n, *cells) if n else row(name, 0, 0.0, 0.0, 0.0, 0.0)      # an empty dataset: a row of zeros, in either table


_HEADS = ('# samples', 'Accuracy', '1 - NED', 'Confidence', 'Label Length')
_FIELDS = ('accuracy', 'ned', 'confidence', 'label_length')


def _print_table(results: List[Result], heads, fields, formats, widths, file) -> None:
    """One Markdown table: a row per dataset — its name, its samples under `heads[0]`, then `fields` in `formats` under the other
    `heads`, right-aligned in `widths` — then the sample-weighted `Combined` row."""
    name_width = max([len(r.dataset) for r in results] + [len('Combined')])
    total = sum(r.num_samples for r in results)

    def row(name: str, samples: int, values) -> str:
        cells = [f'{samples:d}'] + [format(v, f) for v, f in zip(values, formats)]
        return ' | '.join(['| ' + name.ljust(name_width)] + [c.rjust(w) for c, w in zip(cells, widths)]) + ' |'

    print(' | '.join(['| ' + 'Dataset'.ljust(name_width)] + [h.rjust(w) for h, w in zip(heads, widths)]) + ' |', file=file)
    print('|:' + '-' * name_width + ':|' + '|'.join('-' * (w + 1) + ':' for w in widths) + '|', file=file)
    for r in results:
        print(row(r.dataset, r.num_samples, [getattr(r, f) for f in fields]), file=file)
    print('|-' + '-' * name_width + '-|' + '|'.join('-' * (w + 2) for w in widths) + '|', file=file)
    print(row('Combined', total, [sum(r.num_samples * getattr(r, f) for r in results) / total if total else 0.0 for f in fields]), file=file)


def print_results_table(results: List[Result], file=None) -> None:
    """The reference's Markdown table (test.py:40-66): one row per dataset, then the sample-weighted `Combined` row."""
    _print_table(results, _HEADS, _FIELDS, ('.2f',) * 4, [len(h) for h in _HEADS], file)


def print_beam_results_table(results: List[BeamTableResult], width: int, file=None) -> None:
    """The table of an N-best evaluation: the reference's columns, then Hit@W, Oracle 1 - NED and MRR; the same layout and `Combined` row."""
    heads = _HEADS + (f'Hit@{width}', 'Oracle 1 - NED', 'MRR')
    widths = [max(len(h), 6) for h in heads]             # '100.00' and '0.1234' fit under the short heads too
    _print_table(results, heads, _FIELDS + ('hit', 'oracle_ned', 'mrr'), ('.2f',) * 6 + ('.4f',), widths, file)


def print_error_report(name: str, report: ErrorReport, top: int, file=None) -> None:
    """What --analyse prints for one dataset (or for all of them together): the four operation totals, the accuracy by label length, and the
    `top` most frequent confusions, deletions and insertions."""
    print(f'\n{name}: {report.samples} samples, {report.exact} read exactly; {report.matches} matches, {report.substitutions} substitutions, '
          f'{report.insertions} insertions, {report.deletions} deletions', file=file)
    print('| Label length | # samples | Accuracy |', file=file)
    print('|-------------:|----------:|---------:|', file=file)
    for length, samples, share in report.accuracy_by_length():
        print(f"| {str(length) + ('+' if length == 32 else ''):>12} | {samples:>9d} | {100 * share:>8.2f} |", file=file)
    for title, rows in (('confusions (label -> read)', [(f'{a!r} -> {b!r}', c) for a, b, c in report.top_confusions(top)]),
                        ('deletions (label characters not read)', [(repr(a), c) for a, c in report.top_deleted(top)]),
                        ('insertions (characters read that the label lacks)', [(repr(a), c) for a, c in report.top_inserted(top)])):
        print(f'Most frequent {title}: ' + (', '.join(f'{what} x {count}' for what, count in rows) if rows else 'none'), file=file)


def print_audit(name: str, files: List[str], report, top: int, file=None) -> List[dict]:
    """What --audit prints for one dataset: how many readings differ from their label, then the `top` most suspicious of them — the image,
    the label and its log-probability, the reading and its log-probability.  Returns those rows, the image path added."""
    rows = [dict(r, path=files[r['index']]) for r in report.top(top)]
    print(f'\n{name}: {int(report.mismatch.sum())} of {len(report.labels)} readings differ from their label, {report.unscorable} of them cannot be scored; '
          f'the {len(rows)} most suspicious labels:', file=file)
    for r in rows:
        print(f"    {r['suspicion']:9.4f}  {r['path']}  label {r['label']!r} {r['label_score']:.4f}  read {r['reading']!r} {r['reading_score']:.4f}", file=file)
    return rows


def build_parser() -> argparse.ArgumentParser:
    parser = argparse.ArgumentParser()
    parser.add_argument('checkpoint', help="Model checkpoint (or 'pretrained=<model_id>')")
    parser.add_argument('--data_root', default='data')
    parser.add_argument('--batch_size', type=int, default=512)
    parser.add_argument('--cased', action='store_true', default=False, help='Cased comparison')
    parser.add_argument('--punctuation', action='store_true', default=False, help='Check punctuation')
    parser.add_argument('--rotation', type=int, default=0, help='Angle of rotation (counter clockwise) in degrees.')
    parser.add_argument('--device', default='cuda')
    add_evaluation_flags(parser)
    add_orientation_flags(parser)
    add_analysis_flag(parser)
    add_audit_flag(parser)
    return parser


@torch.inference_mode()
def main(argv=None) -> List[Result]:
    parser = build_parser()
    args, unknown = parser.parse_known_args(argv)
    kwargs = parse_model_args(unknown)
    flags = resolve_evaluation_flags(parser, args)
    orient = resolve_orientation(parser, args)
    if orient is not None and flags is not None:
        parser.error('--auto-rotate scores the greedy reading of the chosen view: not with a search flag')
    top = resolve_analysis(parser, args, flags)
    reports = {} if top is not None else None
    audit = resolve_audit(parser, args, flags)
    audits = {} if audit is not None else None

    charset_test = string.digits + string.ascii_lowercase
    if args.cased:
        charset_test += string.ascii_uppercase
    if args.punctuation:
        charset_test += string.punctuation
    kwargs['charset_test'] = charset_test
    print(f'Additional keyword arguments: {kwargs}')

    model = load_from_checkpoint(args.checkpoint, **kwargs).eval().to(args.device)
    search = evaluator_arguments(model, args, flags) if flags is not None else None
    width = evaluation_width(flags) if flags is not None else 0
    results = [evaluate_dataset(model, args.data_root, name, args.batch_size, args.rotation, search, width, orient, reports, audit, audits) for name in find_datasets(args.data_root)]
    if not results:
        raise SystemExit(f'no dataset (a sub-directory with a gt.txt) under {args.data_root!r}')
    with open(args.checkpoint + '.log.txt', 'w') as log:
        for out in (log, sys.stdout):
            if flags is not None:
                print_beam_results_table(results, width, out)
            else:
                print_results_table(results, out)
    if reports is not None:
        combined = None
        for name, report in reports.items():
            print_error_report(name, report, top)
            combined = report if combined is None else combined + report
        print_error_report('All datasets', combined, top)
        with open(args.checkpoint + '.errors.json', 'w', encoding='utf-8') as f:
            json.dump({'top': top, 'datasets': {name: report.to_dict() for name, report in reports.items()}, 'combined': combined.to_dict()}, f, ensure_ascii=False)
    if audits is not None:
        listed = {name: print_audit(name, files, report, audit[0]) for name, (files, report) in audits.items()}
        with open(args.checkpoint + '.audit.json', 'w', encoding='utf-8') as f:
            json.dump({'top': audit[0], 'orders': audit[1], 'length_norm': audit[2],
                       'datasets': {name: {'samples': len(report.labels), 'mismatches': int(report.mismatch.sum()), 'unscorable': report.unscorable, 'top': listed[name]}
                                    for name, (_, report) in audits.items()}}, f, ensure_ascii=False)
    return results


if __name__ == '__main__':
    main()
