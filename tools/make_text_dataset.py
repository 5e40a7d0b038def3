#!/usr/bin/env python3
"""Write a labelled folder of rendered words, from a seed: PNG crops plus the `gt.txt` that `train.py`, `test.py` and
`parseq_amd.data.LabelledFolder` read.

    python tools/make_text_dataset.py out/train --count 2048 --seed 0
    python tools/make_text_dataset.py out/val/words --count 256 --seed 1

Random lower-case strings of 1 - 6 characters in Pillow's built-in font (`ImageFont.load_default()`: nothing to download), dark on
light or light on dark grey, with margins and an overall scale drawn per word so the crops differ in size and aspect.  Small enough
for a test to render in a fraction of a second, and learnable: the data set the end-to-end training tests and the README example use.
"""
from __future__ import annotations

import argparse
import os
import string
from typing import List, Tuple

import numpy as np


def render_words(count: int, seed: int = 0, min_len: int = 1, max_len: int = 6) -> Tuple[List[np.ndarray], List[str]]:
    """(crops, labels): `count` uint8 [H_i, W_i, 3] arrays and the words on them."""
    from PIL import Image, ImageDraw, ImageFont
    rng = np.random.default_rng(seed)
    font = ImageFont.load_default()
    letters = np.array(list(string.ascii_lowercase))
    crops, labels = [], []
    for _ in range(count):
        word = ''.join(rng.choice(letters, size=int(rng.integers(min_len, max_len + 1))))
        left, top, right, bottom = font.getbbox(word)
        mx, my = (int(v) for v in rng.integers(1, 5, size=2))
        w, h = right - left + 2 * mx, bottom - top + 2 * my
        bg = int(rng.integers(0, 256))
        fg = int(rng.integers(0, 96)) if bg >= 128 else int(rng.integers(160, 256))      # at least 32 grey levels apart
        im = Image.new('RGB', (w, h), (bg, bg, bg))
        ImageDraw.Draw(im).text((mx - left, my - top), word, fill=(fg, fg, fg), font=font)
        scale = float(rng.uniform(1.0, 3.0))
        stretch = float(rng.uniform(0.8, 1.25))
        im = im.resize((max(4, round(w * scale * stretch)), max(4, round(h * scale))), Image.BILINEAR)
        crops.append(np.asarray(im).copy())
        labels.append(word)
    return crops, labels


def write_dataset(folder: str, count: int, seed: int = 0) -> List[str]:
    """Render `count` words into `folder` (created): 000000.png ... and gt.txt.  Returns the labels."""
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    crops, labels = render_words(count, seed)
    with open(os.path.join(folder, 'gt.txt'), 'w', encoding='utf-8') as gt:
        for i, (crop, label) in enumerate(zip(crops, labels)):
            name = f'{i:06d}.png'
            Image.fromarray(crop).save(os.path.join(folder, name))
            gt.write(f'{name} {label}\n')
    return labels


def main(argv=None) -> None:
    ap = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    ap.add_argument('folder')
    ap.add_argument('--count', type=int, default=256)
    ap.add_argument('--seed', type=int, default=0)
    args = ap.parse_args(argv)
    write_dataset(args.folder, args.count, args.seed)
    print(f'{args.count} words in {args.folder}')


if __name__ == '__main__':
    main()
