#!/usr/bin/env python3
"""Train a model on a folder of labelled crops — the command line of the reference's `train.py:53-108` on the MI355X backend.

    ./train.py parseq-tiny --train_dir data/train --val_dir data/val [--max_epochs 20] [--batch_size 384] [--val_check_interval 1000]
               [--accumulate_grad_batches 1] [--train_precision bf16x3] [--no_augment] [--augment_policy reference]
               [--ckpt_path run/checkpoints/last.ckpt]
               [name:type=value ...]
    ./train.py pretrained=parseq --train_dir ... --val_dir ...          # fine-tune the released weights

The first argument is an experiment (`parseq`, `parseq-tiny`, `parseq-patch16-224`, `vitstr`: a freshly initialised model) or
`pretrained=<experiment>`.  `--train_dir` and `--val_dir` each hold a `gt.txt` (one image path and label per line; the labels go through
the reference dataset's filter with `charset_train`).  Model overrides are `name:type=value` as for `test.py` (`parse_model_args`).
The run writes `outputs/<model name>/<timestamp>/checkpoints/{epoch=...-step=...-val_accuracy=...-val_NED=....ckpt, last.ckpt}` and
`log.jsonl` (`--out_dir` overrides the directory; with `--ckpt_path` the run continues in the checkpoint's own directory, as the reference
does).  Everything else — the loop, stochastic weight averaging, the checkpoint layout — is `parseq_amd.fit`.
"""
import argparse
import os

from parseq_amd import create_model, load_from_checkpoint, parse_model_args
from parseq_amd.data import LabelledFolder
from parseq_amd.fit import fit


def main(argv=None):
    parser = argparse.ArgumentParser()
    parser.add_argument('model', help="An experiment name, or 'pretrained=<experiment>'")
    parser.add_argument('--train_dir', required=True)
    parser.add_argument('--val_dir', required=True)
    parser.add_argument('--max_epochs', type=int, default=20)
    parser.add_argument('--batch_size', type=int, default=384)
    parser.add_argument('--val_check_interval', type=int, default=1000)
    parser.add_argument('--accumulate_grad_batches', type=int, default=1)
    parser.add_argument('--train_precision', default='bf16x3', choices=['fp32', 'bf16', 'bf16x3'])
    parser.add_argument('--no_augment', action='store_true', default=False)
    parser.add_argument('--augment_policy', default='fourteen', choices=['fourteen', 'reference'],
                        help="'reference': the reference's sixteen operators, GaussianBlur and PoissonNoise included")
    parser.add_argument('--swa_epoch_start', type=float, default=0.75)
    parser.add_argument('--ckpt_path', default=None, help='Resume from this checkpoint of an earlier run')
    parser.add_argument('--out_dir', default=None)
    parser.add_argument('--seed', type=int, default=0)
    parser.add_argument('--workers', type=int, default=8, help='Threads decoding images')
    parser.add_argument('--device', default='cuda')
    args, unknown = parser.parse_known_args(argv)
    kwargs = parse_model_args(unknown)
    kwargs['batch_size'] = args.batch_size
    print(f'Additional keyword arguments: {kwargs}')

    if args.model.startswith('pretrained='):
        system = load_from_checkpoint(args.model, **kwargs)
    else:
        system = create_model(args.model, **kwargs)
    system = system.to(args.device)
    system.train_precision = args.train_precision
    hp = system.hparams
    train_set = LabelledFolder(args.train_dir, hp.charset_train, hp.max_label_length)
    val_set = LabelledFolder(args.val_dir, hp.charset_train, hp.max_label_length)
    print(f'{len(train_set)} training and {len(val_set)} validation samples')
    out_dir = args.out_dir
    if out_dir is None and args.ckpt_path is not None:
        out_dir = os.path.dirname(os.path.dirname(os.path.abspath(args.ckpt_path)))
    result = fit(system, train_set, val_set, args.max_epochs, args.val_check_interval, out_dir=out_dir,
                 accumulate_grad_batches=args.accumulate_grad_batches, swa_epoch_start=args.swa_epoch_start, augment=not args.no_augment,
                 seed=args.seed, resume=args.ckpt_path, workers=args.workers, augment_policy=args.augment_policy)
    for record in result.log:
        if record['event'] in ('validation', 'epoch'):
            print(record)
    print(f'checkpoints in {os.path.join(result.out_dir, "checkpoints")}')
    return result


if __name__ == '__main__':
    main()
