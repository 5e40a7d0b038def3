#!/usr/bin/env python3
"""Read text from image files — the command line of the reference's `read.py:27-48` on the MI355X backend.

    ./read.py pretrained=parseq --images a.png b.jpg [--device cuda] [name:type=value ...]
    ./read.py path/to/lightning.ckpt --images *.png refine_iters:int=2 decode_ar:bool=false
    ./read.py pretrained=parseq --images a.png --nbest 5 [--beam 8]     the 5 best readings with their log-probabilities under each line
    ./read.py pretrained=parseq --images a.png --lexicon words.txt [--beam 8] [--nbest 3]     read only words of the list (one per line)

Differences from the reference, all on the device side of the same results: the files are decoded on the host (PIL),
everything after that — the bicubic resize of the reference transform (bit-exact with Pillow), ToTensor + Normalize, the
model, soft-max / greedy pick / EOS cut — runs in libparseq_hip, and all images go through ONE batched forward instead of a
Python loop of batch-1 calls.
"""
import argparse

import torch
from PIL import Image

from parseq_amd import load_from_checkpoint, parse_model_args
from parseq_amd.preprocess import resize_batch


@torch.inference_mode()
def read_files(model, files, device='cuda'):
    """[(file, label, confidence)] for image files, one batched forward."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    batch = resize_batch(crops, tuple(model.hparams.img_size))          # uint8 [N, 3, H, W], Pillow-exact bicubic
    labels, confidences = model.tokenizer.read(model(batch))             # normalisation happens inside the patch embedding
    return list(zip(files, labels, confidences.tolist()))


@torch.inference_mode()
def read_files_nbest(model, files, nbest, beam_width=None, device='cuda'):
    """[(file, [(label, log-probability)] best first, at most `nbest`)] through one beam search of width `beam_width` (default `nbest`)."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    batch = resize_batch(crops, tuple(model.hparams.img_size))
    beams = model.tokenizer.decode_beams(model.beam_search(batch, beam_width or nbest))
    return [(f, alts[:nbest]) for f, alts in zip(files, beams)]


LEXICON_BEAM = 8      # --beam under --lexicon when none is given


def load_word_list(path):
    """The words of a lexicon file: one per line, surrounding white space and empty lines dropped."""
    with open(path, encoding='utf-8') as fh:
        return [w for w in (line.strip() for line in fh) if w]


@torch.inference_mode()
def read_files_lexicon(model, files, words, nbest=1, beam_width=LEXICON_BEAM, device='cuda'):
    """[(file, [(word, log-probability)] best first, at most `nbest`)]: one beam search of width `beam_width` constrained to `words`
    (DESIGN.md section 19).  A finished reading is a word of the list in the list's spelling; case is folded when the model's charset has
    only one.  A crop for which no word of the list finishes keeps its unfinished prefixes, or nothing."""
    import numpy as np
    from parseq_amd.lexicon import Lexicon
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    lexicon = Lexicon(words, model.tokenizer, fold_case=True, max_label_length=model.model.max_label_length).to(device)
    batch = resize_batch(crops, tuple(model.hparams.img_size))
    beams = model.tokenizer.decode_beams(model.beam_search(batch, beam_width, lexicon=lexicon), lexicon)
    return [(f, alts[:nbest]) for f, alts in zip(files, beams)]


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('checkpoint', help="Model checkpoint (or 'pretrained=<model_id>')")
    parser.add_argument('--images', nargs='+', help='Images to read')
    parser.add_argument('--device', default='cuda')
    parser.add_argument('--nbest', type=int, default=0, help='Also print the N best readings with their log-probabilities (beam search)')
    parser.add_argument('--beam', type=int, default=None, help=f'Beam width of --nbest (default: N) or of --lexicon (default: {LEXICON_BEAM})')
    parser.add_argument('--lexicon', default=None, metavar='FILE',
                        help='Read only words of this list (one per line): a beam search constrained to the list; --nbest N prints the N best words')
    return parser


def resolve_search(parser, args):
    """(beam width, N) of the search the flags ask for, (None, 0) for none; a contradiction ends in parser.error."""
    if args.lexicon is not None:
        nbest = args.nbest if args.nbest > 0 else 1
        beam = args.beam if args.beam is not None else max(LEXICON_BEAM, nbest)
        if beam < nbest:
            parser.error('--beam must be at least --nbest')
        return beam, nbest
    if args.beam is not None and (args.nbest <= 0 or args.beam < args.nbest):
        parser.error('--beam needs --nbest N with N <= the beam width')
    return args.beam, args.nbest


def main(argv=None):
    parser = build_parser()
    args, unknown = parser.parse_known_args(argv)
    kwargs = parse_model_args(unknown)
    print(f'Additional keyword arguments: {kwargs}')

    beam, nbest = resolve_search(parser, args)
    model = load_from_checkpoint(args.checkpoint, **kwargs).eval().to(args.device)
    files = args.images or []
    if args.lexicon is not None:
        # the best word of the list where the greedy reading goes; the alternatives only where --nbest asks for them
        for fname, alts in read_files_lexicon(model, files, load_word_list(args.lexicon), nbest, beam, args.device):
            print(f'{fname}: {alts[0][0] if alts else ""}')
            for label, logp in (alts if args.nbest > 0 else []):
                print(f'    {logp:9.4f}  {label}')
        return
    alternatives = dict(read_files_nbest(model, files, args.nbest, args.beam, args.device)) if args.nbest > 0 else {}
    for fname, pred, _ in read_files(model, files, args.device):
        print(f'{fname}: {pred}')
        for label, logp in alternatives.get(fname, []):
            print(f'    {logp:9.4f}  {label}')


if __name__ == '__main__':
    main()
