"""Mint the GaussianBlur fixtures: Pillow's own `Image.filter(ImageFilter.GaussianBlur(radius))` (the call of the reference's
gaussian_blur, strhub/data/augment.py:45-49) on the seeded inputs of tests/augment_reference.py, at the sizes and radii of
tests/augment_blur_reference.py (`BLUR_SIZES`, `BLUR_RADII`).

Run where Pillow is installed.  Inputs are regenerated from their seed by the tests; only Pillow's outputs are stored.
    python tools/make_augment_blur_golden.py   ->  tests/golden/augment_blur_pillow.npz
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageFilter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from augment_blur_reference import BLUR_RADII, BLUR_SIZES, blur_key  # noqa: E402
from augment_reference import make_input  # noqa: E402


def pillow_blur(img: np.ndarray, radius) -> np.ndarray:
    """The Pillow call the operator must equal, on uint8 [h, w, 3]."""
    return np.asarray(Image.fromarray(img, 'RGB').filter(ImageFilter.GaussianBlur(radius)))


def main():
    out = {}
    for h, w in BLUR_SIZES:
        img = make_input(h, w)
        for radius in BLUR_RADII:
            out[blur_key(h, w, radius)] = pillow_blur(img, radius)
    path = os.path.join(ROOT, 'tests', 'golden', 'augment_blur_pillow.npz')
    np.savez_compressed(path, pillow_version=np.array(PIL.__version__), **out)
    print(path, len(out), 'cases, Pillow', PIL.__version__, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
