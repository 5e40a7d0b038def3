#!/usr/bin/env python3
"""Read text from image files — the command line of the reference's `read.py:27-48` on the MI355X backend.

    ./read.py pretrained=parseq --images a.png b.jpg [--device cuda] [name:type=value ...]
    ./read.py path/to/lightning.ckpt --images *.png refine_iters:int=2 decode_ar:bool=false
    ./read.py pretrained=parseq --images a.png --nbest 5 [--beam 8]     the 5 best readings with their log-probabilities under each line
    ./read.py pretrained=parseq --images a.png --lexicon words.txt [--beam 8] [--nbest 3]     read only words of the list (one per line)
    ./read.py pretrained=parseq --images a.png --lexicon words.txt --match [8] [--nbest 3]     read freely, then choose among the list's 8 nearest words
    ./read.py pretrained=parseq --images a.png --lexicon counts.txt --priors [--lm-weight 0.5]     the list's second column is a count: a prior over the words
    ./read.py pretrained=parseq --images a.png --lm corpus.txt [--lm-order 3] [--lm-weight 0.3] [--char-bonus 0.5]     fuse a character n-gram model into the search
    ./read.py pretrained=parseq --images a.png --pattern '[A-Z]{2}[0-9]{4}'     read only what the pattern matches
    ./read.py pretrained=parseq --images a.png --nbest 5 --refine-beams edit [--refine-iters 2]     refine every alternative, rank them again
    ./read.py pretrained=parseq --images a.png --boxes     a second line per image: every character with its box in the image's own pixels
    ./read.py pretrained=parseq --images scene.jpg --regions scene.txt [--boxes]     read every quadrilateral of the file (x1,y1,..,x4,y4 per line)
    ./read.py pretrained=parseq --images scene.jpg --polygons scene.txt [--boxes]     read every polygon of the file (x1,y1,..,xK,yK per line): curved text
    ./read.py pretrained=parseq --images a.png --auto-rotate flip [--upright-bias 0.1]     read every crop upright and upside down, keep the better reading
    ./read.py pretrained=parseq --images line.png --lines [--line-overlap 0.25] [--line-sep 0.25] [--boxes]     read a whole text line as stitched windows
    ./read.py pretrained=parseq --images a.png b.png --candidates cands.txt [--orders both] [--length-norm]     score the tab-separated strings of line i for image i, best first
    ./read.py pretrained=parseq --images a.png --expect AB1234     how likely is this string for the crop, and how likely is what the model reads instead

Differences from the reference, all on the device side of the same results: the files are decoded on the host (PIL),
everything after that — the bicubic resize of the reference transform (bit-exact with Pillow), ToTensor + Normalize, the
model, soft-max / greedy pick / EOS cut — runs in libparseq_hip, and all images go through ONE batched forward instead of a
Python loop of batch-1 calls.
"""
import argparse

import torch
from PIL import Image

from parseq_amd import load_from_checkpoint, parse_model_args
from parseq_amd.preprocess import resize_batch, rotated_size, unrotate_points
from parseq_amd.search_flags import (LEXICON_BEAM, LM_ORDER, MATCH_N, add_line_flags, add_orientation_flags, add_score_flags, build_automaton, load_candidates,  # noqa: F401
                                      load_word_counts, load_word_list, orientation_prior, resolve_lines, resolve_automaton, resolve_flags, resolve_match,
                                      resolve_orientation, resolve_refine, resolve_score, resolve_search)


def turned_name(name, angle):
    """How --auto-rotate names a reading: the name itself for a crop read as it came, `name@angle` for one read turned by `angle` degrees
    counter clockwise."""
    return name if angle % 360 == 0 else f'{name}@{angle % 360}'


def crop_batch(model, crops, orient=None):
    """(batch, angles, result): the model's input for `crops`.  Without `orient` the resized crops, angles all 0 and no result; with
    `orient` = (mode, bias) of --auto-rotate the view of every crop that the model reads best, the angle it was
    turned by, and the `OrientedResult` of that choice."""
    img_size = tuple(model.hparams.img_size)
    if orient is None:
        return resize_batch(crops, img_size), [0] * len(crops), None
    from parseq_amd.preprocess import orientation_views
    views, angles = orientation_views(crops, orient[0], img_size)
    result = model.orient(views, prior=orientation_prior(orient[1], views.shape[1]))
    return result.images, [a[k] for a, k in zip(angles, result.view.cpu().tolist())], result


@torch.inference_mode()
def read_files(model, files, device='cuda', orient=None):
    """[(file, label, confidence)] for image files, one batched forward.  `orient`: see `crop_batch`; a turned crop is named `file@angle`."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    if orient is not None:
        _, angles, result = crop_batch(model, crops, orient)
        labels, confidences = model.tokenizer.read(result.logits)
        return list(zip([turned_name(f, a) for f, a in zip(files, angles)], labels, confidences.tolist()))
    batch = resize_batch(crops, tuple(model.hparams.img_size))          # uint8 [N, 3, H, W], Pillow-exact bicubic
    labels, confidences = model.tokenizer.read(model(batch))             # normalisation happens inside the patch embedding
    return list(zip(files, labels, confidences.tolist()))


@torch.inference_mode()
def read_files_nbest(model, files, nbest, beam_width=None, device='cuda', refine=None, refine_iters=1, orient=None):
    """[(file, [(label, log-probability)] best first, at most `nbest`)] through one beam search of width `beam_width` (default `nbest`);
    `refine` ('edit' / 'score') refines the alternatives on the device and ranks them by their refined scores."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    batch, angles, _ = crop_batch(model, crops, orient)
    search = {} if refine is None else {'refine': refine, 'refine_iters': refine_iters}
    beams = model.tokenizer.decode_beams(model.beam_search(batch, beam_width or nbest, **search))
    return [(turned_name(f, a), alts[:nbest]) for f, a, alts in zip(files, angles, beams)]


def scale_box(box, img_size, size):
    """A box (x0, y0, x1, y1) in pixels of the model's input (`img_size` = (h, w)) in pixels of the original crop (`size` = (h, w)): the resize
    of the input transform is a plain stretch, so each axis scales on its own."""
    sx, sy = size[1] / img_size[1], size[0] / img_size[0]
    return (box[0] * sx, box[1] * sy, box[2] * sx, box[3] * sy)


def unturned_box(box, angle, size):
    """A box (x0, y0, x1, y1) in pixels of a crop of `size` = (h, w) turned by `angle` (a multiple of 90 degrees), in pixels of the crop itself."""
    (xa, ya), (xb, yb) = unrotate_points(angle, size, ((box[0], box[1]), (box[2], box[3])))
    return (min(xa, xb), min(ya, yb), max(xa, xb), max(ya, yb))


@torch.inference_mode()
def read_files_boxes(model, files, device='cuda', orient=None):
    """[(file, label, [(character, (x0, y0, x1, y1))])]: the greedy reading of every file and where each of its characters is (DESIGN.md
    section 21), boxes in pixels of the file's own image.  One batched call.  With `orient` the boxes of a turned crop are led back through
    `unrotate_points`."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    img_size = tuple(model.hparams.img_size)
    batch, angles, _ = crop_batch(model, crops, orient)
    labels, chars = model.tokenizer.decode_localization(model.localize(batch))
    return [(turned_name(f, a), label, [(ch, unturned_box(scale_box(box, img_size, rotated_size(a, crop.shape[:2])), a, crop.shape[:2])) for ch, box in row])
            for f, a, label, row, crop in zip(files, angles, labels, chars, crops)]


def load_regions(path):
    """The quadrilaterals of an ICDAR-2015 style file: every non-empty line is `x1,y1,x2,y2,x3,y3,x4,y4[,transcription]`, the corners
    clockwise from the text's top-left; whatever follows an eighth comma is ignored.  Returns [((x1, y1), .. (x4, y4))] as floats; a line
    that is not eight finite numbers is a ValueError naming file and line."""
    import math
    quads = []
    with open(path, encoding='utf-8-sig') as fh:
        for number, line in enumerate(fh, 1):
            if not line.strip():
                continue
            try:
                v = [float(field) for field in line.split(',')[:8]]
                if len(v) != 8 or not all(math.isfinite(x) for x in v):
                    raise ValueError
            except ValueError:
                raise ValueError(f'{path}, line {number}: expected eight comma-separated numbers x1,y1,..,x4,y4, got {line.strip()!r}') from None
            quads.append(tuple(zip(v[0::2], v[1::2])))
    return quads


def load_polygons(path):
    """The polygons of a Total-Text / CTW1500 style file: every non-empty line is `x1,y1,..,xK,yK[,transcription]`, K = 2N >= 4 points, N
    along the text's upper edge from its top-left, then N back along its lower edge.  The coordinates are the longest leading run of fields
    that parse as finite numbers; if that run is odd, its last field belongs to the transcription (a numeric one) and is dropped.  Returns
    [((x1, y1), .. (xK, yK))] as floats; a line that leaves anything but an even number of points, at least 4, is a ValueError naming
    file and line."""
    import math
    polygons = []
    with open(path, encoding='utf-8-sig') as fh:
        for number, line in enumerate(fh, 1):
            if not line.strip():
                continue
            v = []
            for field in line.split(','):
                try:
                    value = float(field)
                except ValueError:
                    break
                if not math.isfinite(value):
                    break
                v.append(value)
            v = v[:len(v) - len(v) % 2]
            if len(v) < 8 or len(v) % 4:
                raise ValueError(f'{path}, line {number}: expected an even number of points, at least 4, as comma-separated numbers '
                                 f'x1,y1,..,xK,yK, got {len(v) // 2} in {line.strip()!r}')
            polygons.append(tuple(zip(v[0::2], v[1::2])))
    return polygons


@torch.inference_mode()
def load_region_batch(model, files, region_files, device='cuda', polygons=False, orient=None):
    """The regions of `region_files[i]` cut out of `files[i]` and straightened, as one batch for the model: every
    scene is decoded and uploaded once, all regions of all scenes go through ONE rectify-and-resize call.  Returns (names, batch, back):
    `file#k` per region, k counting from 0 within its file; uint8 [N, 3, H, W] (None without regions); per region the (coefficients, (h, w))
    with which `map_to_source` leads from the model's input back into the scene.  With `polygons` the files hold polygons (`load_polygons`),
    straightened strip by strip (section 25), and `back` holds per region the (strips, (h, w)) of `mesh_to_source`.
    With `orient` = (mode, bias) of --auto-rotate every quadrilateral is cut in the views of `orientation_regions` — its corner list shifted —
    still in ONE rectify-and-resize call; the batch is the view of every region the model reads best, `back` that view's map, and a region
    read at a shift k other than 0 is named `file#i@angle`, angle = 90 k."""
    import numpy as np
    from parseq_amd.preprocess import mesh_rectify_resize_batch, orientation_regions, polygon_descs, rectify_resize_batch, region_descs
    load, describe, rectify = (load_polygons, polygon_descs, mesh_rectify_resize_batch) if polygons else (load_regions, region_descs, rectify_resize_batch)
    names, regions = [], []
    for i, (f, rf) in enumerate(zip(files, region_files)):
        for k, quad in enumerate(load(rf)):
            names.append(f'{f}#{k}')
            regions.append((i, quad))
    if not regions:
        return [], None, []
    shifts = None
    if orient is not None:
        regions, shifts = orientation_regions(regions, orient[0])
    described = describe(regions, n_images=len(files))
    scenes = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    batch = rectify(scenes, [(index, coeffs, size) for index, size, coeffs in described], tuple(model.hparams.img_size))
    if shifts is not None:
        K = len(shifts[0])
        result = model.orient(batch.view(len(names), K, *batch.shape[1:]), prior=orientation_prior(orient[1], K))
        view = result.view.cpu().tolist()
        names = [turned_name(name, 90 * per_region[k]) for name, per_region, k in zip(names, shifts, view)]
        batch, described = result.images, [described[i * K + k] for i, k in enumerate(view)]
    return names, batch, [(coeffs, size) for _, size, coeffs in described]


@torch.inference_mode()
def read_regions(model, files, region_files, beam=None, nbest=0, words=None, list_words=False, refine=None, refine_iters=1, boxes=False, device='cuda',
                 match=None, prior=None, polygons=False, orient=None):
    """The lines `--regions` prints, for the same flags as the whole-crop readings above, on the batch of `load_region_batch`: `words` is the
    list of --lexicon (its alternatives are listed only with `list_words`), `boxes` adds every character's quadrilateral in the scene, `match`
    the N of --match, `prior` the (automaton, alpha, beta) of --priors / --lm / --pattern; `polygons` makes the files those of --polygons; `orient` is the (mode, bias) of
    --auto-rotate (`load_region_batch`)."""
    from parseq_amd.preprocess import map_to_source, mesh_to_source
    to_source = mesh_to_source if polygons else map_to_source
    names, batch, back = load_region_batch(model, files, region_files, device, polygons, orient)
    if not names:
        return []
    lines = []
    if prior is not None:
        for name, alts in zip(names, automaton_batch(model, batch, beam, *prior)):
            lines += automaton_lines(name, alts[:nbest], list_words)
        return lines
    if words is not None and match is not None:
        for name, alts in zip(names, match_batch(model, batch, words, match, device)):
            lines += match_lines(name, alts[:nbest], list_words)
        return lines
    if words is not None:
        from parseq_amd.lexicon import Lexicon
        lexicon = Lexicon(words, model.tokenizer, fold_case=True, max_label_length=model.model.max_label_length).to(device)
        search = {} if refine is None else {'refine': refine}
        beams = model.tokenizer.decode_beams(model.beam_search(batch, beam, lexicon=lexicon, **search), lexicon)
        for name, alts in zip(names, beams):
            alts = alts[:nbest]
            lines.append(f'{name}: {alts[0][0] if alts else ""}')
            lines += [f'    {logp:9.4f}  {label}' for label, logp in (alts if list_words else [])]
        return lines
    if boxes:
        img_size = tuple(model.hparams.img_size)
        labels, chars = model.tokenizer.decode_localization(model.localize(batch))
        for name, label, row, (coeffs, size) in zip(names, labels, chars, back):
            lines.append(f'{name}: {label}')
            quads = [(ch, to_source(coeffs, size, img_size, ((x0, y0), (x1, y0), (x1, y1), (x0, y1)))) for ch, (x0, y0, x1, y1) in row]
            lines.append('    ' + ' '.join(f'{ch}[' + ','.join(f'{v:.1f}' for p in quad for v in p) + ']' for ch, quad in quads))
        return lines
    alternatives = [[]] * len(names)
    if nbest > 0:
        search = {} if refine is None else {'refine': refine, 'refine_iters': refine_iters}
        alternatives = [alts[:nbest] for alts in model.tokenizer.decode_beams(model.beam_search(batch, beam or nbest, **search))]
    labels, _ = model.tokenizer.read(model(batch))
    for name, label, alts in zip(names, labels, alternatives):
        lines.append(f'{name}: {label}')
        lines += [f'    {logp:9.4f}  {alt}' for alt, logp in alts]
    return lines


@torch.inference_mode()
def read_files_lexicon(model, files, words, nbest=1, beam_width=LEXICON_BEAM, device='cuda', refine=None, orient=None):
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
    batch, angles, _ = crop_batch(model, crops, orient)
    search = {} if refine is None else {'refine': refine}
    beams = model.tokenizer.decode_beams(model.beam_search(batch, beam_width, lexicon=lexicon, **search), lexicon)
    return [(turned_name(f, a), alts[:nbest]) for f, a, alts in zip(files, angles, beams)]


def automaton_batch(model, batch, beam_width, automaton, alpha, beta):
    """Per crop of `batch` [(label, fused score, model log-probability, prior)] best first: one beam search over `automaton`."""
    result = model.beam_search(batch, beam_width, automaton=automaton, alpha=alpha, beta=beta)
    beams = model.tokenizer.decode_beams(result, automaton)
    parts = torch.stack([result.model_scores, result.priors], -1).cpu().tolist()
    return [[(label, f, m, p) for (label, f), (m, p) in zip(alts, rows)] for alts, rows in zip(beams, parts)]      # dead beams come last in both


def automaton_lines(name, alts, list_all):
    """What a search over an automaton prints for one image: the best reading; with --nbest the alternatives — fused score, the model's
    log-probability and the prior first."""
    lines = [f'{name}: {alts[0][0] if alts else ""}']
    return lines + [f'    {f:9.4f}  lp={m:9.4f} prior={p:9.4f}  {label}' for label, f, m, p in (alts if list_all else [])]


@torch.inference_mode()
def read_files_automaton(model, files, automaton, beam_width=8, alpha=1.0, beta=0.0, device='cuda', orient=None):
    """[(file, [(label, fused score, model log-probability, prior)] best first)] for image files: one batched search over `automaton`."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    batch, angles, _ = crop_batch(model, crops, orient)
    return list(zip([turned_name(f, a) for f, a in zip(files, angles)], automaton_batch(model, batch, beam_width, automaton, alpha, beta)))


def match_batch(model, batch, words, n, device='cuda'):
    """Per crop of `batch` [(word, pseudo-log-likelihood, distance)] best first: the free reading, the `n` words of `words` nearest to it in
    edit distance, rescored by the model.  Fewer than `n` where the list is shorter."""
    from parseq_amd.lexicon import Lexicon
    lexicon = Lexicon(words, model.tokenizer, fold_case=True, max_label_length=model.model.max_label_length).to(device)
    result = model.lexicon_match(batch, lexicon, n)
    beams = model.tokenizer.decode_beams(result, lexicon)
    distances = result.distances.cpu().tolist()
    return [[(label, logp, d) for (label, logp), d in zip(alts, dist)] for alts, dist in zip(beams, distances)]      # dead slots come last in both


def match_lines(name, alts, list_all):
    """What --match prints for one image: the best word where the greedy reading goes; with --nbest the candidates, score and distance first."""
    lines = [f'{name}: {alts[0][0] if alts else ""}']
    return lines + [f'    {logp:9.4f}  d={d:<2d} {label}' for label, logp, d in (alts if list_all else [])]


@torch.inference_mode()
def read_files_match(model, files, words, n=MATCH_N, device='cuda', orient=None):
    """[(file, [(word, pseudo-log-likelihood, distance)] best first)] for image files: one batched `lexicon_match` call."""
    import numpy as np
    crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    if not crops:
        return []
    batch, angles, _ = crop_batch(model, crops, orient)
    return list(zip([turned_name(f, a) for f, a in zip(files, angles)], match_batch(model, batch, words, n, device)))


@torch.inference_mode()
def read_lines_lines(model, files, lines, region_files=None, boxes=False, device='cuda'):
    """The lines `--lines` prints: every file — or, with `region_files`, every quadrilateral of every file, cut out
    at its own size by `rectify_batch` and named `file#k` — is one text line, read by `model.read_lines` with `lines` = (overlap, sep).
    `boxes` adds every character's box in the file's own pixels; a region's boxes are led back through `map_to_source` as quadrilaterals."""
    import numpy as np
    from parseq_amd.preprocess import map_to_source, rectify_batch, region_descs
    scenes = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
    names, crops, back = list(files), scenes, None
    if region_files is not None:
        names, regions = [], []
        for i, (f, rf) in enumerate(zip(files, region_files)):
            for k, quad in enumerate(load_regions(rf)):
                names.append(f'{f}#{k}')
                regions.append((i, quad))
        if regions:
            described = region_descs(regions, n_images=len(files))
            crops = rectify_batch(scenes, [(index, coeffs, size) for index, size, coeffs in described])
            back = [(coeffs, size) for _, size, coeffs in described]
    if not names:
        return []
    result = model.read_lines(crops, overlap=lines[0], min_sep=lines[1])
    decoded = model.tokenizer.decode_lines(result, boxes=boxes)
    out = []
    for i, (name, label) in enumerate(zip(names, decoded[0])):
        out.append(f'{name}: {label}')
        if boxes and back is None:
            out.append('    ' + ' '.join(f'{ch}[{x0:.1f},{y0:.1f},{x1:.1f},{y1:.1f}]' for ch, (x0, y0, x1, y1) in decoded[2][i]))
        elif boxes:
            coeffs, size = back[i]       # the boxes are in pixels of the rectified region already: no stretch to undo
            quads = [(ch, map_to_source(coeffs, size, size, ((x0, y0), (x1, y0), (x1, y1), (x0, y1)))) for ch, (x0, y0, x1, y1) in decoded[2][i]]
            out.append('    ' + ' '.join(f'{ch}[' + ','.join(f'{v:.1f}' for p in quad for v in p) + ']' for ch, quad in quads))
    return out


@torch.inference_mode()
def score_lines(model, names, batch, score):
    """The lines --candidates / --expect print for the crops of `batch`, named `names`; `score` is the ScoreFlags of
    `resolve_score`.  --candidates: per crop its best candidate where the reading goes, then every candidate best first with its
    log-probability.  --expect: per crop the free reading, then the log-probability of the expected string and of the reading, one
    `score` call on the pair.  A list that does not hold one entry per crop, or a character outside the training charset, is a ValueError."""
    if score.expect is not None:
        if len(score.expect) != len(names):
            raise ValueError(f'--expect takes one string per crop: {len(score.expect)} strings for {len(names)} crops')
        readings, _ = model.tokenizer.read(model(batch))
        limit = model.model.max_label_length
        pairs = [[want] + ([got] if len(got) <= limit else []) for want, got in zip(score.expect, readings)]
        scores = model.score(batch, pairs, orders=score.orders, normalize=score.normalize).scores.cpu().tolist()
        lines = []
        for name, pair, row in zip(names, pairs, scores):
            lines.append(f'{name}: {pair[1] if len(pair) > 1 else ""}')
            lines.append(f'    {row[0]:9.4f}  expected  {pair[0]}')
            lines += [f'    {row[1]:9.4f}  read      {pair[1]}'] if len(pair) > 1 else []
        return lines
    candidates = load_candidates(score.candidates)
    if len(candidates) != len(names):
        raise ValueError(f'{score.candidates}: one line of candidates per crop: {len(candidates)} lines for {len(names)} crops')
    ranked = model.tokenizer.decode_scores(model.score(batch, candidates, orders=score.orders, normalize=score.normalize), candidates)
    lines = []
    for name, alts in zip(names, ranked):
        lines.append(f'{name}: {alts[0][0] if alts else ""}')
        lines += [f'    {logp:9.4f}  {label}' for label, logp, _ in alts]
    return lines


@torch.inference_mode()
def score_files(model, files, score, region_files=None, polygons=False, device='cuda'):
    """`score_lines` for image files, or with `region_files` for every region of every file (`load_region_batch`)."""
    import numpy as np
    if region_files is not None:
        names, batch, _ = load_region_batch(model, files, region_files, device, polygons)
    else:
        crops = [torch.from_numpy(np.asarray(Image.open(f).convert('RGB')).copy()).to(device) for f in files]
        names, batch = list(files), (resize_batch(crops, tuple(model.hparams.img_size)) if crops else None)
    return score_lines(model, names, batch, score) if names else []


def build_parser():
    parser = argparse.ArgumentParser()
    parser.add_argument('checkpoint', help="Model checkpoint (or 'pretrained=<model_id>')")
    parser.add_argument('--images', nargs='+', help='Images to read')
    parser.add_argument('--device', default='cuda')
    parser.add_argument('--nbest', type=int, default=0, help='Also print the N best readings with their log-probabilities (beam search)')
    parser.add_argument('--beam', type=int, default=None, help=f'Beam width of --nbest (default: N) or of --lexicon (default: {LEXICON_BEAM})')
    parser.add_argument('--lexicon', default=None, metavar='FILE',
                        help='Read only words of this list (one per line): a beam search constrained to the list; --nbest N prints the N best words')
    parser.add_argument('--match', type=int, nargs='?', const=MATCH_N, default=None, metavar='N',
                        help=f'With --lexicon: read freely, then let the model choose among the N (default {MATCH_N}) words of the list nearest to the '
                             'reading in edit distance, instead of a search constrained to the list; --nbest K prints the K best with score and distance; '
                             'not with --beam or --refine-beams edit')
    parser.add_argument('--refine-beams', default=None, choices=['edit', 'score'], dest='refine_beams',
                        help="Refine the alternatives of --nbest / --lexicon with the model's cloze pass and rank them again: 'edit' replaces every "
                             "reading by its refined one, 'score' only rescores (the only mode under --lexicon)")
    parser.add_argument('--boxes', action='store_true',
                        help="Print a second line per image: every character of the reading with its box (x0,y0,x1,y1) in the image's own pixels; "
                             'not with --nbest or --lexicon')
    parser.add_argument('--regions', nargs='+', default=None, metavar='FILE',
                        help='One file of quadrilaterals per image, in order (ICDAR-2015 style: x1,y1,x2,y2,x3,y3,x4,y4[,text] per line, clockwise '
                             "from the text's top-left): read every region of the scene, printed as image#k; with --boxes every character's "
                             "quadrilateral in the scene's pixels")
    parser.add_argument('--polygons', nargs='+', default=None, metavar='FILE',
                        help='One file of polygons per image, in order (Total-Text / CTW1500 style: x1,y1,..,xK,yK[,text] per line, K = 2N >= 4 points, '
                             "N along the text's upper edge from its top-left, then N back along its lower edge): read every curved region of the "
                             'scene like --regions does; not together with --regions')
    parser.add_argument('--priors', action='store_true',
                        help='With --lexicon: the list has a second white-space separated column, a count; the words are then a prior (their smoothed '
                             'relative frequencies enter the ranking), not only a constraint')
    parser.add_argument('--lm', default=None, metavar='FILE',
                        help='Fuse a character n-gram model counted from this text file (one sequence per line, blank lines skipped) into a beam search (open vocabulary)')
    parser.add_argument('--lm-order', type=int, default=None, dest='lm_order', metavar='N', help=f'Order of --lm, 1 to 4 (default {LM_ORDER})')
    parser.add_argument('--pattern', default=None, metavar='REGEX',
                        help='Read only what fully matches this regular expression (literals, ., [...], \\d, \\w, groups, |, ? * + {m} {m,n})')
    parser.add_argument('--lm-weight', type=float, default=None, dest='lm_weight', metavar='A',
                        help='Weight of the prior of --priors / --lm / --pattern in the ranking (default 1)')
    parser.add_argument('--char-bonus', type=float, default=None, dest='char_bonus', metavar='B',
                        help='Added to the ranking per character read, with --priors / --lm / --pattern (default 0)')
    parser.add_argument('--refine-iters', type=int, default=None, dest='refine_iters', metavar='K', help='Iterations of --refine-beams edit (default 1)')
    add_orientation_flags(parser)      # --auto-rotate MODE [--upright-bias X]: a crop read turned is printed as file@angle
    add_line_flags(parser)             # --lines [--line-overlap F] [--line-sep F]: every image is a whole text line
    add_score_flags(parser)            # --candidates FILE / --expect STRING .. [--orders O] [--length-norm]: score given strings
    return parser


def main(argv=None):
    parser = build_parser()
    args, unknown = parser.parse_known_args(argv)
    kwargs = parse_model_args(unknown)
    print(f'Additional keyword arguments: {kwargs}')

    if args.boxes and (args.nbest > 0 or args.lexicon is not None):
        parser.error('--boxes goes with the default reading only: not with --nbest or --lexicon')
    score = resolve_score(parser, args)
    lines = resolve_lines(parser, args)
    kind, alpha, beta, match, beam, nbest, refine, refine_iters = resolve_flags(parser, args)
    files = args.images or []
    if args.regions is not None and args.polygons is not None:
        parser.error('--polygons and --regions are two ways to cut the same scenes: give one of them')
    polygons = args.polygons is not None
    orient = resolve_orientation(parser, args)
    region_files = args.polygons if polygons else args.regions
    if region_files is not None and len(region_files) != len(files):
        parser.error(f'--{"polygons" if polygons else "regions"} takes one file per image, in order: {len(region_files)} files for {len(files)} images')
    if score is not None and score.expect is not None and region_files is None and len(score.expect) != len(files):
        parser.error(f'--expect takes one string per image, in order: {len(score.expect)} strings for {len(files)} images')
    model = load_from_checkpoint(args.checkpoint, **kwargs).eval().to(args.device)
    if score is not None:
        try:
            for line in score_files(model, files, score, region_files, polygons, args.device):
                print(line)
        except ValueError as e:
            raise SystemExit(f'read.py: {e}') from None
        return
    if lines is not None:
        for line in read_lines_lines(model, files, lines, region_files, args.boxes, args.device):
            print(line)
        return
    if kind is not None:
        automaton = build_automaton(model, kind, args)
        if region_files is not None:
            lines = read_regions(model, files, region_files, beam, nbest, list_words=args.nbest > 0, device=args.device, prior=(automaton, alpha, beta),
                                 polygons=polygons, orient=orient)
        else:
            lines = [line for fname, alts in read_files_automaton(model, files, automaton, beam, alpha, beta, args.device, orient)
                     for line in automaton_lines(fname, alts[:nbest], args.nbest > 0)]
        for line in lines:
            print(line)
        return
    if region_files is not None:
        words = load_word_list(args.lexicon) if args.lexicon is not None else None
        for line in read_regions(model, files, region_files, beam, nbest, words, args.nbest > 0, refine, refine_iters, args.boxes, args.device, match,
                                 polygons=polygons, orient=orient):
            print(line)
        return
    if match is not None:
        for fname, alts in read_files_match(model, files, load_word_list(args.lexicon), match, args.device, orient):
            for line in match_lines(fname, alts[:nbest], args.nbest > 0):
                print(line)
        return
    if args.lexicon is not None:
        # the best word of the list where the greedy reading goes; the alternatives only where --nbest asks for them
        for fname, alts in read_files_lexicon(model, files, load_word_list(args.lexicon), nbest, beam, args.device, refine, orient):
            print(f'{fname}: {alts[0][0] if alts else ""}')
            for label, logp in (alts if args.nbest > 0 else []):
                print(f'    {logp:9.4f}  {label}')
        return
    if args.boxes:
        for fname, pred, chars in read_files_boxes(model, files, args.device, orient):
            print(f'{fname}: {pred}')
            print('    ' + ' '.join(f'{ch}[{x0:.1f},{y0:.1f},{x1:.1f},{y1:.1f}]' for ch, (x0, y0, x1, y1) in chars))
        return
    alternatives = dict(read_files_nbest(model, files, args.nbest, args.beam, args.device, refine, refine_iters, orient)) if args.nbest > 0 else {}
    for fname, pred, _ in read_files(model, files, args.device, orient):
        print(f'{fname}: {pred}')
        for label, logp in alternatives.get(fname, []):
            print(f'    {logp:9.4f}  {label}')


if __name__ == '__main__':
    main()
