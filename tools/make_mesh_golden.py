"""Mint the polygon rectification fixtures: Pillow's own `Image.transform((w, h), Image.MESH, [(box, quad), ...], Image.BICUBIC)` on
seeded inputs, and `.resize((128, 32), BICUBIC)` on the result — what a caller with a detector of curved text does on the host today
(DESIGN.md section 25).

Run where Pillow is installed.  Inputs are regenerated from their seed by the tests (tests/rectify_reference.py make_input); the file holds
the strips the outputs were made with — x0, x1 and the eight numbers Pillow derives for QUAD from each box and quad — and Pillow's bytes.
    python tools/make_mesh_golden.py   ->  tests/golden/mesh_pillow.npz
"""
import os
import sys

import numpy as np
import PIL
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
from mesh_reference import CASES, MANY_SOURCE, RESIZED, SOURCES, TARGET, make_input, many_regions, polygon_mesh, polygon_quads, strips_to_array  # noqa: E402


def pillow_mesh(img: np.ndarray, h: int, w: int, quads) -> Image.Image:
    """`quads`: [((x0, 0, x1, h), (NW, SW, SE, NE))], mesh_reference.polygon_quads."""
    data = [(box, tuple(v for p in quad for v in p)) for box, quad in quads]
    return Image.fromarray(img, 'RGB').transform((w, h), Image.MESH, data, Image.BICUBIC)


def main():
    out = {}
    for name, source, (h, w), polygon in CASES:
        crop = pillow_mesh(make_input(*SOURCES[source]), h, w, polygon_quads(polygon, h, w))
        out[f'{name}_strips'] = strips_to_array(polygon_mesh(polygon, h, w))
        out[f'{name}_out'] = np.asarray(crop)
        if name in RESIZED:
            out[f'{name}_resized'] = np.ascontiguousarray(np.asarray(crop.resize((TARGET[1], TARGET[0]), Image.BICUBIC)).transpose(2, 0, 1))
    src = make_input(*SOURCES[MANY_SOURCE])
    strips, counts, crops = [], [], []
    for (h, w), polygon in many_regions():
        rows = strips_to_array(polygon_mesh(polygon, h, w))
        strips.append(rows)
        counts.append(len(rows))
        crops.append(np.asarray(pillow_mesh(src, h, w, polygon_quads(polygon, h, w))).reshape(-1))
    out['many_strips'] = np.concatenate(strips)
    out['many_counts'] = np.array(counts, np.int32)
    out['many_out'] = np.concatenate(crops)
    path = os.path.join(ROOT, 'tests', 'golden', 'mesh_pillow.npz')
    np.savez_compressed(path, pillow_version=np.array(PIL.__version__), **out)
    print(path, len(out), 'arrays, Pillow', PIL.__version__, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
