"""NumPy restatement (test infrastructure) of the first step of the reference's evaluation transform,
`img.rotate(rotation, expand=True)` (strhub/data/module.py:72-73): Pillow's `Image.rotate` with its defaults, i.e. nearest
resampling and black fill.  Pinned against Pillow's own outputs in tests/golden/rotate_pillow.npz (tools/make_rotate_golden.py).

Published algorithm (Pillow's Image.rotate and the nearest-neighbour affine transform of its Geometry.c), restated:
  * the angle is reduced modulo 360; 0 is a copy, 180 flips both axes, 90 and 270 are exact transposes;
  * any other angle builds the inverse map (output pixel -> source position) in float64 from cos / sin rounded to 15 decimals,
    takes the expanded size from the four transformed corners, re-centres the map, and samples in 16.16 fixed point:
    FIX(v) = floor(v * 65536 + 0.5), half a pixel folded into the two offsets, an arithmetic shift by 16, black outside.
`SIZES`, `ANGLES`, `BATCH` and `make_input` are the seeded cases the fixtures and tests/test_rotate.py share.
"""
import math

import numpy as np

NONE, QUARTER, HALF, THREE_QUARTER, AFFINE = range(5)

SIZES = [(1, 1), (1, 7), (7, 1), (2, 3), (3, 2), (5, 5), (8, 8), (31, 100), (64, 17)]        # (height, width)
ANGLES = [0, 90, 180, 270, 360, -90, 450, 1, 7.5, 45, 89, 91, 135, 179.5, 359]
# the ragged batch of the rotate-then-resize fixtures: every size, a different map per image, two unrotated images, every exact mode
BATCH = [((31, 100), 0), ((1, 1), 45), ((1, 7), 90), ((7, 1), 180), ((2, 3), 270), ((3, 2), 7.5), ((5, 5), 0), ((8, 8), 135),
         ((31, 100), 89), ((64, 17), 91), ((64, 17), 359), ((31, 100), 179.5)]
TARGETS = [(32, 128), (16, 64)]


def make_input(h: int, w: int) -> np.ndarray:
    """Seeded uint8 [h, w, 3]: sixteen grey levels per channel (neighbours differ almost surely; the fixtures still compress)."""
    return (np.random.default_rng(7000 * h + w).integers(0, 16, (h, w, 3)) * 17).astype(np.uint8)


def fix(v: float) -> int:
    return math.floor(v * 65536.0 + 0.5)


def affine_map(h: int, w: int, angle: float):
    """(mode, nh, nw, six ints) of Image.rotate(angle, expand=True) on a w x h image, written from the published algorithm."""
    angle = angle % 360.0
    if angle == 0:
        return NONE, h, w, (0,) * 6
    if angle == 180:
        return HALF, h, w, (0,) * 6
    if angle in (90, 270):
        return (QUARTER if angle == 90 else THREE_QUARTER), w, h, (0,) * 6
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def t(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2], m[5] = t(-w / 2.0, -h / 2.0)
    m[2] += w / 2.0
    m[5] += h / 2.0
    xs, ys = zip(*(t(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs))
    nh = math.ceil(max(ys)) - math.floor(min(ys))
    m[2], m[5] = t(-(nw - w) / 2.0, -(nh - h) / 2.0)
    ints = (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))
    return AFFINE, nh, nw, ints


def apply_map(img: np.ndarray, mode: int, nh: int, nw: int, ints) -> np.ndarray:
    """uint8 [h, w, 3] -> uint8 [nh, nw, 3] through one map (the five modes of `affine_map`)."""
    if mode == NONE:
        return img.copy()
    if mode == QUARTER:
        return np.ascontiguousarray(img.transpose(1, 0, 2)[::-1])
    if mode == HALF:
        return np.ascontiguousarray(img[::-1, ::-1])
    if mode == THREE_QUARTER:
        return np.ascontiguousarray(img.transpose(1, 0, 2)[:, ::-1])
    h, w = img.shape[:2]
    a0, a1, a2, a3, a4, a5 = (int(v) for v in ints)
    y, x = np.mgrid[0:nh, 0:nw].astype(np.int64)
    sx = (a2 + a0 * x + a1 * y) >> 16
    sy = (a5 + a3 * x + a4 * y) >> 16
    inside = (sx >= 0) & (sx < w) & (sy >= 0) & (sy < h)
    out = np.zeros((nh, nw, 3), np.uint8)
    out[inside] = img[sy[inside], sx[inside]]
    return out


def rotate_u8(img: np.ndarray, angle: float) -> np.ndarray:
    """Bit-exact with np.asarray(Image.fromarray(img).rotate(angle, expand=True))."""
    return apply_map(img, *affine_map(img.shape[0], img.shape[1], angle))
