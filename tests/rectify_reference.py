"""NumPy restatement (test infrastructure) of the rectification of quadrilateral regions: Pillow's
`Image.transform((w, h), Image.PERSPECTIVE, coeffs, Image.BICUBIC)` on RGB images, fill 0, in float64, and the host geometry in front of
and behind it.  It never calls the library.  Pinned against Pillow's own outputs in tests/golden/rectify_pillow.npz
(tools/make_rectify_golden.py), which holds sizes, coefficients and Pillow's bytes only: the inputs come from `make_input`.

Published algorithm, restated: output pixel (x, y) reads the source at
    ((a0 X + a1 Y + a2) / (a6 X + a7 Y + 1), (a3 X + a4 Y + a5) / (a6 X + a7 Y + 1)),  X = x + 0.5, Y = y + 0.5;
a position outside [0, W) x [0, H) (NaN included) keeps the fill; otherwise Pillow's bicubic filter around the position minus a half:
sixteen taps, columns clamped, a ROW outside the image repeating the value of the row above, clipped to 0 .. 255, truncated.
`CASES`, `MANY` and `make_input` are the seeded cases the fixtures, tests/test_rectify_host.py and tests/test_rectify.py share.
"""
import math

import numpy as np

from augment_reference import _cubic

TARGET = (32, 128)                           # the model's input the fused path is pinned at


def make_input(h: int, w: int) -> np.ndarray:
    """Seeded uint8 [h, w, 3]: a ramp of 6 x 4 blocks over the whole range with one pixel in eight displaced — edges that over- and
    undershoot under the bicubic filter (the clip at both ends is exercised), and fixtures that still compress."""
    rng = np.random.default_rng(7000 * h + w)
    y, x = np.mgrid[0:h, 0:w]
    base = (17 * ((x // 6 + 5 * (y // 4)) % 16))[..., None] + np.array([0, 0, 0])
    base = np.where(((x // 6 + y // 4) % 2)[..., None] == 0, base, 255 - base) + np.array([0, -9, 9])
    noise = 40 * rng.integers(-2, 3, (h, w, 3)) * (rng.integers(0, 8, (h, w, 1)) == 0)
    return np.clip(base + noise, 0, 255).astype(np.uint8)


# ---- host geometry ------------------------------------------------------------------------------------------------------------
def region_size(quad, max_side=1024):
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(float(x), float(y)) for x, y in quad]
    w = math.floor(max(math.hypot(x1 - x0, y1 - y0), math.hypot(x2 - x3, y2 - y3)) + 0.5)
    h = math.floor(max(math.hypot(x3 - x0, y3 - y0), math.hypot(x2 - x1, y2 - y1)) + 0.5)
    return min(max(h, 1), max_side), min(max(w, 1), max_side)


def corners(h, w):
    return ((0.0, 0.0), (float(w), 0.0), (float(w), float(h)), (0.0, float(h)))


def denominators(coeffs, h, w):
    return [coeffs[6] * X + coeffs[7] * Y + 1.0 for X, Y in corners(h, w)]


def quad_coeffs(quad, h, w):
    """Pillow's PERSPECTIVE data taking (0, 0), (w, 0), (w, h), (0, h) to TL, TR, BR, BL; the closed form for a parallelogram."""
    pts = [(float(x), float(y)) for x, y in quad]
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = pts
    if x0 + x2 == x1 + x3 and y0 + y2 == y1 + y3:
        a = ((x1 - x0) / w, (x3 - x0) / h, x0, (y1 - y0) / w, (y3 - y0) / h, y0, 0.0, 0.0)
    else:
        m, rhs = [], []
        for (X, Y), (x, y) in zip(corners(h, w), pts):
            m += [[X, Y, 1, 0, 0, 0, -X * x, -Y * x], [0, 0, 0, X, Y, 1, -X * y, -Y * y]]
            rhs += [x, y]
        a = tuple(np.linalg.solve(np.array(m, np.float64), np.array(rhs, np.float64)).tolist())
    if not all(math.isfinite(c) for c in a) or not all(d > 0.0 for d in denominators(a, h, w)):
        raise ValueError(f'no usable projective map for {pts}')
    return a


def apply_coeffs(coeffs, X, Y):
    a = coeffs
    den = a[6] * X + a[7] * Y + 1.0
    return (a[0] * X + a[1] * Y + a[2]) / den, (a[3] * X + a[4] * Y + a[5]) / den


def map_to_source(coeffs, size, img_size, points):
    return [apply_coeffs([float(c) for c in coeffs], x * size[1] / img_size[1], y * size[0] / img_size[0]) for x, y in points]


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------
def transform_perspective(img, nh, nw, coeffs):
    """Image.fromarray(img).transform((nw, nh), Image.PERSPECTIVE, coeffs, Image.BICUBIC) on uint8 [h, w, 3]."""
    h, w = img.shape[:2]
    a = [float(c) for c in coeffs]
    y, x = np.mgrid[0:nh, 0:nw]
    xin, yin = x + 0.5, y + 0.5
    with np.errstate(all='ignore'):
        den = a[6] * xin + a[7] * yin + 1.0
        sx = (a[0] * xin + a[1] * yin + a[2]) / den
        sy = (a[3] * xin + a[4] * yin + a[5]) / den
        inside = (sx >= 0.0) & (sx < w) & (sy >= 0.0) & (sy < h)          # NaN compares false: outside
    sx, sy = sx[inside] - 0.5, sy[inside] - 0.5
    fx, fy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    dx, dy = (sx - fx)[..., None], (sy - fy)[..., None]
    src = img.astype(np.float64)

    def cx(v):
        return np.clip(v, 0, w - 1)

    def row(yy):
        yy = np.clip(yy, 0, h - 1)
        return _cubic(src[yy, cx(fx - 1)], src[yy, cx(fx)], src[yy, cx(fx + 1)], src[yy, cx(fx + 2)], dx)
    v1 = row(fy - 1)
    v2 = np.where(((fy >= 0) & (fy < h))[..., None], row(fy), v1)
    v3 = np.where(((fy + 1 >= 0) & (fy + 1 < h))[..., None], row(fy + 1), v2)
    v4 = np.where(((fy + 2 >= 0) & (fy + 2 < h))[..., None], row(fy + 2), v3)
    val = np.clip(_cubic(v1, v2, v3, v4, dy), 0.0, 255.0).astype(np.int64)
    out = np.zeros((nh, nw, 3), np.uint8)
    out[inside] = val.astype(np.uint8)
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------
SOURCES = [(1, 1), (1, 2), (2, 3), (5, 7), (37, 53)]            # (height, width); a call of every case names them by this index
_INSIDE = ((8.3, 6.1), (44.7, 9.2), (42.1, 30.4), (6.5, 26.8))


def _shift(quad, dx, dy):
    return tuple((x + dx, y + dy) for x, y in quad)


# (name, index into SOURCES, (h, w) of the output, quad TL TR BR BL)
CASES = [
    ('one_pixel', 0, (1, 1), ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0))),
    ('one_pixel_up', 0, (9, 1), ((0.1, -0.2), (0.8, 0.1), (0.9, 1.3), (0.2, 0.9))),
    ('two_pixels', 1, (1, 9), ((-0.5, -0.3), (2.4, -0.2), (2.6, 1.1), (-0.4, 1.2))),
    ('two_by_three', 2, (9, 1), ((0.4, 0.1), (2.7, 0.3), (2.9, 1.8), (0.2, 2.2))),
    ('two_by_three_wide', 2, (17, 33), ((-0.6, -0.4), (3.5, -0.1), (3.2, 2.3), (-0.2, 2.6))),
    ('five_by_seven', 3, (17, 33), ((0.6, 0.4), (6.3, 1.1), (6.8, 4.2), (0.2, 4.9))),
    ('five_by_seven_small', 3, (1, 1), ((2.2, 1.3), (4.9, 1.6), (4.6, 3.3), (2.4, 3.1))),
    ('inside', 4, (17, 33), _INSIDE),
    ('over_left', 4, (17, 33), _shift(_INSIDE, -15.0, 0.0)),
    ('over_right', 4, (17, 33), _shift(_INSIDE, 20.0, 0.0)),
    ('over_top', 4, (17, 33), _shift(_INSIDE, 0.0, -12.0)),
    ('over_bottom', 4, (17, 33), _shift(_INSIDE, 0.0, 15.0)),
    ('outside', 4, (9, 1), _shift(_INSIDE, 100.0, 80.0)),
    ('foreshortened', 4, (40, 70), ((10.0, 3.0), (45.0, 13.0), (45.0, 23.0), (10.0, 33.0))),          # left edge 30, right edge 10
    ('rotated_rectangle', 4, (13, 26), ((12.5, 3.25), (36.5, 13.25), (31.5, 25.25), (7.5, 15.25))),    # sides (24, 10) and (-5, 12): 26 x 13
    ('upside_down', 4, (1, 9), (_INSIDE[2], _INSIDE[3], _INSIDE[0], _INSIDE[1])),
    ('vertical_text', 4, (33, 17), (_INSIDE[3], _INSIDE[0], _INSIDE[1], _INSIDE[2])),
]
MANY = 300                                   # regions of the call whose tile table outgrows a workgroup's 256 work-items
MANY_SOURCE = 4


def many_regions():
    """[((h, w), quad)] x MANY on SOURCES[MANY_SOURCE]: perturbed rectangles of every small size, some hanging over an edge."""
    rng = np.random.default_rng(2210)
    sh, sw = SOURCES[MANY_SOURCE]
    out = []
    for i in range(MANY):
        h, w = 1 + i % 5, 1 + (i // 5) % 7
        cx, cy = rng.uniform(-2.0, sw + 2.0), rng.uniform(-2.0, sh + 2.0)
        hw, hh = rng.uniform(1.0, 9.0), rng.uniform(1.0, 5.0)
        rect = ((cx - hw, cy - hh), (cx + hw, cy - hh), (cx + hw, cy + hh), (cx - hw, cy + hh))
        out.append(((h, w), tuple((x + rng.uniform(-0.3, 0.3) * hw, y + rng.uniform(-0.3, 0.3) * hh) for x, y in rect)))
    return out
