"""Mint the rotation fixtures: Pillow's own `Image.rotate(angle, expand=True)` on seeded inputs, and (`--resized`, the default)
`.resize((W, H), BICUBIC)` on the result for the ragged batch of tests/test_rotate.py — the first two steps of the reference's
evaluation transform (strhub/data/module.py:72-77).

Run where Pillow is installed.  Inputs are regenerated from their seed by the tests (tests/rotate_reference.py); only Pillow's
outputs are stored.
    python tools/make_rotate_golden.py [--no-resized]   ->  tests/golden/rotate_pillow.npz
"""
import argparse
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from rotate_reference import ANGLES, BATCH, SIZES, TARGETS, make_input  # noqa: E402


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--no-resized', action='store_true', help='store the rotated images only')
    args = parser.parse_args()
    out = {}
    for h, w in SIZES:
        img = Image.fromarray(make_input(h, w), 'RGB')
        for angle in ANGLES:
            out[f'{h}x{w}_{angle}'] = np.asarray(img.rotate(angle, expand=True))
    if not args.no_resized:
        for i, ((h, w), angle) in enumerate(BATCH):
            rotated = Image.fromarray(make_input(h, w), 'RGB').rotate(angle, expand=True)
            for th, tw in TARGETS:
                out[f'batch{i}_{th}x{tw}'] = np.asarray(rotated.resize((tw, th), Image.BICUBIC))
    path = os.path.join(ROOT, 'tests', 'golden', 'rotate_pillow.npz')
    np.savez_compressed(path, pillow_version=np.array(PIL.__version__), **out)
    print(path, len(out), 'cases, Pillow', PIL.__version__, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
