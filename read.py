#!/usr/bin/env python3
"""Read text from image files — the command line of the reference's `read.py:27-48` on the MI355X backend.

    ./read.py pretrained=parseq --images a.png b.jpg [--device cuda] [name:type=value ...]
    ./read.py path/to/lightning.ckpt --images *.png refine_iters:int=2 decode_ar:bool=false
    ./read.py pretrained=parseq --images a.png --nbest 5 [--beam 8]     the 5 best readings with their log-probabilities under each line
    ./read.py pretrained=parseq --images a.png --lexicon words.txt [--beam 8] [--nbest 3]     read only words of the list (one per line)
    ./read.py pretrained=parseq --images a.png --nbest 5 --refine-beams edit [--refine-iters 2]     refine every alternative, rank them again
    ./read.py pretrained=parseq --images a.png --boxes     a second line per image: every character with its box in the image's own pixels

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
def read_files_nbest(model, files, nbest, beam_width=None, device='cuda', refine=None, refine_iters=1):
    """[(file, [(label, log-probability)] best first, at most `nbest`)] through one beam search of width `beam_width` (default `nbest`);
    `refine` ('edit' / 'score') refines the alternatives on the device and ranks them by their refined scores."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    batch = resize_batch(crops, tuple(model.hparams.img_size))
    search = {} if refine is None else {'refine': refine, 'refine_iters': refine_iters}
    beams = model.tokenizer.decode_beams(model.beam_search(batch, beam_width or nbest, **search))
    return [(f, alts[:nbest]) for f, alts in zip(files, beams)]


def scale_box(box, img_size, size):
    """A box (x0, y0, x1, y1) in pixels of the model's input (`img_size` = (h, w)) in pixels of the original crop (`size` = (h, w)): the resize
    of the input transform is a plain stretch, so each axis scales on its own."""
    sx, sy = size[1] / img_size[1], size[0] / img_size[0]
    return (box[0] * sx, box[1] * sy, box[2] * sx, box[3] * sy)


@torch.inference_mode()
def read_files_boxes(model, files, device='cuda'):
    """[(file, label, [(character, (x0, y0, x1, y1))])]: the greedy reading of every file and where each of its characters is (DESIGN.md
    section 21), boxes in pixels of the file's own image.  One batched call."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    img_size = tuple(model.hparams.img_size)
    batch = resize_batch(crops, img_size)
    labels, chars = model.tokenizer.decode_localization(model.localize(batch))
    return [(f, label, [(ch, scale_box(box, img_size, crop.shape[:2])) for ch, box in row]) for f, label, row, crop in zip(files, labels, chars, crops)]


LEXICON_BEAM = 8      # --beam under --lexicon when none is given


def load_word_list(path):
    """The words of a lexicon file: one per line, surrounding white space and empty lines dropped."""
    with open(path, encoding='utf-8') as fh:
        return [w for w in (line.strip() for line in fh) if w]


@torch.inference_mode()
def read_files_lexicon(model, files, words, nbest=1, beam_width=LEXICON_BEAM, device='cuda', refine=None):
    """[(file, [(word, log-probability)] best first, at most `nbest`)]: one beam search of width `beam_width` constrained to `words`
    (DESIGN.md section 19).  A finished reading is a word of the list in the list's spelling; case is folded when the model's charset has
    only one.  A crop for which no word of the list finishes keeps its unfinished prefixes, or nothing.  `refine='score'` ranks the words by
    their pseudo-log-likelihood (section 20)."""
    import numpy as np
    from parseq_amd.lexicon import Lexicon
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    lexicon = Lexicon(words, model.tokenizer, fold_case=True, max_label_length=model.model.max_label_length).to(device)
    batch = resize_batch(crops, tuple(model.hparams.img_size))
    search = {} if refine is None else {'refine': refine}
    beams = model.tokenizer.decode_beams(model.beam_search(batch, beam_width, lexicon=lexicon, **search), lexicon)
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
    parser.add_argument('--refine-beams', default=None, choices=['edit', 'score'], dest='refine_beams',
                        help="Refine the alternatives of --nbest / --lexicon with the model's cloze pass and rank them again: 'edit' replaces every "
                             "reading by its refined one, 'score' only rescores (the only mode under --lexicon)")
    parser.add_argument('--boxes', action='store_true',
                        help="Print a second line per image: every character of the reading with its box (x0,y0,x1,y1) in the image's own pixels; "
                             'not with --nbest or --lexicon')
    parser.add_argument('--refine-iters', type=int, default=None, dest='refine_iters', metavar='K', help='Iterations of --refine-beams edit (default 1)')
    return parser


def resolve_refine(parser, args):
    """(mode, iterations) of --refine-beams, (None, 1) for none; a contradiction ends in parser.error."""
    if args.refine_beams is None:
        if args.refine_iters is not None:
            parser.error('--refine-iters needs --refine-beams')
        return None, 1
    if args.lexicon is None and args.nbest <= 0:
        parser.error('--refine-beams needs --nbest N or --lexicon FILE')
    iters = 1 if args.refine_iters is None else args.refine_iters
    if iters < 1:
        parser.error('--refine-iters must be at least 1')
    if args.refine_beams == 'score' and iters != 1:
        parser.error('--refine-beams score runs once: --refine-iters must be 1')
    if args.refine_beams == 'edit' and args.lexicon is not None:
        parser.error('--refine-beams edit is not allowed with --lexicon (an edited reading can leave the list); use score')
    return args.refine_beams, iters


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

    if args.boxes and (args.nbest > 0 or args.lexicon is not None):
        parser.error('--boxes goes with the default reading only: not with --nbest or --lexicon')
    beam, nbest = resolve_search(parser, args)
    refine, refine_iters = resolve_refine(parser, args)
    model = load_from_checkpoint(args.checkpoint, **kwargs).eval().to(args.device)
    files = args.images or []
    if args.lexicon is not None:
        # the best word of the list where the greedy reading goes; the alternatives only where --nbest asks for them
        for fname, alts in read_files_lexicon(model, files, load_word_list(args.lexicon), nbest, beam, args.device, refine):
            print(f'{fname}: {alts[0][0] if alts else ""}')
            for label, logp in (alts if args.nbest > 0 else []):
                print(f'    {logp:9.4f}  {label}')
        return
    if args.boxes:
        for fname, pred, chars in read_files_boxes(model, files, args.device):
            print(f'{fname}: {pred}')
            print('    ' + ' '.join(f'{ch}[{x0:.1f},{y0:.1f},{x1:.1f},{y1:.1f}]' for ch, (x0, y0, x1, y1) in chars))
        return
    alternatives = dict(read_files_nbest(model, files, args.nbest, args.beam, args.device, refine, refine_iters)) if args.nbest > 0 else {}
    for fname, pred, _ in read_files(model, files, args.device):
        print(f'{fname}: {pred}')
        for label, logp in alternatives.get(fname, []):
            print(f'    {logp:9.4f}  {label}')


if __name__ == '__main__':
    main()
