"""Mint the augmentation fixtures: Pillow's own outputs for every RandAugment operator of the reference's training transform
(strhub/data/augment.py, aa_overrides.py: timm's auto_augment operators) on seeded inputs, at the sizes and arguments of
tests/augment_reference.py (`SIZES`, `single_cases`).

Run where Pillow is installed.  Inputs are regenerated from their seed by the tests; only Pillow's outputs are stored.
    python tools/make_augment_golden.py   ->  tests/golden/augment_pillow.npz
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image, ImageEnhance, ImageOps

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from augment_reference import SIZES, case_key, make_input, single_cases  # noqa: E402

FILL = dict(fillcolor=(128, 128, 128))


def pillow_op(img: Image.Image, name: str, *args) -> Image.Image:
    """The Pillow call each operator must equal (timm's auto_augment functions, written out)."""
    w, h = img.size
    if name == 'AutoContrast':
        return ImageOps.autocontrast(img)
    if name == 'Equalize':
        return ImageOps.equalize(img)
    if name == 'Invert':
        return ImageOps.invert(img)
    if name == 'Posterize':
        return img if args[0] >= 8 else ImageOps.posterize(img, args[0])
    if name == 'Solarize':
        return ImageOps.solarize(img, args[0])
    if name == 'SolarizeAdd':
        return img.point([min(255, i + args[0]) if i < 128 else i for i in range(256)] * 3)
    if name in ('Color', 'Contrast', 'Brightness'):
        return getattr(ImageEnhance, name)(img).enhance(args[0])
    if name == 'Rotate':
        return img.rotate(args[0], resample=args[1], expand=True, **FILL)
    matrix = {'ShearX': (1, args[0], 0, 0, 1, 0), 'ShearY': (1, 0, 0, args[0], 1, 0), 'TranslateXRel': (1, 0, args[0] * w, 0, 1, 0),
              'TranslateYRel': (1, 0, 0, 0, 1, args[0] * h)}[name]
    return img.transform(img.size, Image.AFFINE, matrix, resample=args[1], **FILL)


def main():
    out = {}
    for h, w in SIZES:
        img = Image.fromarray(make_input(h, w), 'RGB')
        for name, args in single_cases():
            out[case_key(h, w, name, args)] = np.asarray(pillow_op(img, name, *args))
    path = os.path.join(ROOT, 'tests', 'golden', 'augment_pillow.npz')
    np.savez_compressed(path, pillow_version=np.array(PIL.__version__), **out)
    print(path, len(out), 'cases, Pillow', PIL.__version__, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
