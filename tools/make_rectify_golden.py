"""Mint the rectification fixtures: Pillow's own `Image.transform((w, h), Image.PERSPECTIVE, coeffs, Image.BICUBIC)` on seeded inputs, and
`.resize((128, 32), BICUBIC)` on the result — what a caller with a text detector does on the host today.

Run where Pillow is installed.  Inputs are regenerated from their seed by the tests (tests/rectify_reference.py); the file holds sizes,
the coefficients the outputs were made with (so that no test depends on a linear solver's last bit) and Pillow's bytes.
    python tools/make_rectify_golden.py   ->  tests/golden/rectify_pillow.npz
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from rectify_reference import CASES, MANY_SOURCE, SOURCES, TARGET, make_input, many_regions, quad_coeffs  # noqa: E402


def pillow_rectify(img: np.ndarray, h: int, w: int, coeffs) -> Image.Image:
    return Image.fromarray(img, 'RGB').transform((w, h), Image.PERSPECTIVE, tuple(float(c) for c in coeffs), Image.BICUBIC)


def main():
    out = {}
    for name, source, (h, w), quad in CASES:
        coeffs = quad_coeffs(quad, h, w)
        crop = pillow_rectify(make_input(*SOURCES[source]), h, w, coeffs)
        out[f'{name}_coef'] = np.array(coeffs, np.float64)
        out[f'{name}_out'] = np.asarray(crop)
        out[f'{name}_resized'] = np.ascontiguousarray(np.asarray(crop.resize((TARGET[1], TARGET[0]), Image.BICUBIC)).transpose(2, 0, 1))
    src = make_input(*SOURCES[MANY_SOURCE])
    coefs, crops = [], []
    for (h, w), quad in many_regions():
        coefs.append(quad_coeffs(quad, h, w))
        crops.append(np.asarray(pillow_rectify(src, h, w, coefs[-1])).reshape(-1))
    out['many_coef'] = np.array(coefs, np.float64)
    out['many_out'] = np.concatenate(crops)
    path = os.path.join(ROOT, 'tests', 'golden', 'rectify_pillow.npz')
    np.savez_compressed(path, pillow_version=np.array(PIL.__version__), **out)
    print(path, len(out), 'arrays, Pillow', PIL.__version__, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
