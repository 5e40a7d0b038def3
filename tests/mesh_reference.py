"""NumPy restatement (test infrastructure) of the rectification of polygon regions: Pillow's
`Image.transform((w, h), Image.MESH, [((x0, 0, x1, h), quad), ...], Image.BICUBIC)` on RGB images, fill 0, in float64, and the host
geometry in front of and behind it.  It never calls the library.  Pinned against Pillow's own outputs in tests/golden/mesh_pillow.npz
(tools/make_mesh_golden.py), which holds the strips and Pillow's bytes only: the inputs come from rectify_reference.make_input.

Published algorithm, restated: a polygon of 2N points (top left to right, bottom right to left) is N - 1 quadrilaterals, each painted
into its own strip of output columns x0 .. x1 - 1.  Output pixel (x, y) of a strip reads the source at
    (a0 + a1 X + a2 Y + a3 X Y,  a4 + a5 X + a6 Y + a7 X Y),   X = (x - x0) + 0.5, Y = y + 0.5,
with the eight numbers Pillow derives for QUAD from the strip's box and quad; a position outside [0, W) x [0, H) (NaN included) keeps the
fill; otherwise Pillow's bicubic filter around the position minus a half, as in rectify_reference.
`CASES`, `MANY` and `many_regions` are the seeded cases the fixtures, tests/test_mesh_rectify_host.py and tests/test_mesh_rectify.py share.
"""
import math

import numpy as np

from augment_reference import _cubic
from rectify_reference import TARGET, make_input  # noqa: F401   (re-exported: the tests take both from here)

MAX_STRIPS = 64


# ---- host geometry ------------------------------------------------------------------------------------------------------------
def sides(polygon):
    """(top, bottom), both left to right."""
    pts = [(float(x), float(y)) for x, y in polygon]
    n = len(pts) // 2
    return pts[:n], pts[n:][::-1]


def _dist(p, q):
    return math.hypot(q[0] - p[0], q[1] - p[1])


def polygon_size(polygon, max_side=1024):
    top, bottom = sides(polygon)
    w = math.floor(max(sum(_dist(s[i], s[i + 1]) for i in range(len(s) - 1)) for s in (top, bottom)) + 0.5)
    h = math.floor(max(_dist(t, b) for t, b in zip(top, bottom)) + 0.5)
    return min(max(h, 1), max_side), min(max(w, 1), max_side)


def quad_data(x0, x1, h, nw, sw, se, ne):
    """Image.__transformer's QUAD data for the box (x0, 0, x1, h), in its expression order."""
    As, At = 1.0 / (x1 - x0), 1.0 / h
    return (nw[0], (ne[0] - nw[0]) * As, (sw[0] - nw[0]) * At, (se[0] - sw[0] - ne[0] + nw[0]) * As * At,
            nw[1], (ne[1] - nw[1]) * As, (sw[1] - nw[1]) * At, (se[1] - sw[1] - ne[1] + nw[1]) * As * At)


def polygon_cuts(polygon, w):
    top, bottom = sides(polygon)
    weights = [0.5 * (_dist(top[i], top[i + 1]) + _dist(bottom[i], bottom[i + 1])) for i in range(len(top) - 1)]
    total = 0.0
    for v in weights:
        total += v
    cuts, cum = [0], 0.0
    for v in weights[:-1]:
        cum += v
        cuts.append(math.floor(cum / total * w + 0.5))
    return cuts + [w]


def polygon_quads(polygon, h, w):
    """[((x0, 0, x1, h), (NW, SW, SE, NE))]: the `data` of Image.transform(MESH) for the polygon; a segment of no width yields none."""
    top, bottom = sides(polygon)
    cuts = polygon_cuts(polygon, w)
    return [((cuts[i], 0, cuts[i + 1], h), (top[i], bottom[i], bottom[i + 1], top[i + 1])) for i in range(len(top) - 1) if cuts[i + 1] > cuts[i]]


def polygon_mesh(polygon, h, w):
    """[(x0, x1, coef8)]"""
    return [(box[0], box[2], quad_data(box[0], box[2], h, *quad)) for box, quad in polygon_quads(polygon, h, w)]


def apply_strip(a, u, Y):
    return a[0] + a[1] * u + a[2] * Y + a[3] * u * Y, a[4] + a[5] * u + a[6] * Y + a[7] * u * Y


def mesh_to_source(strips, size, img_size, points):
    out = []
    for x, y in points:
        X, Y = x * size[1] / img_size[1], y * size[0] / img_size[0]
        k = 0
        while k + 1 < len(strips) and X >= strips[k][1]:
            k += 1
        out.append(apply_strip(strips[k][2], X - strips[k][0], Y))
    return out


def strips_to_array(strips):
    """[n, 10] float64: x0, x1, the eight coefficients (the form the fixtures store)."""
    return np.array([[x0, x1, *coef] for x0, x1, coef in strips], np.float64).reshape(-1, 10)


def strips_from_array(rows):
    return [(int(r[0]), int(r[1]), tuple(float(c) for c in r[2:])) for r in np.asarray(rows)]


# ---- stage 1 ------------------------------------------------------------------------------------------------------------------
def _sample(img, sx, sy):
    """Pillow's bicubic transform filter at the source positions (sx, sy), any shape: (inside, uint8 values of the inside ones)."""
    h, w = img.shape[:2]
    with np.errstate(all='ignore'):
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
    return inside, np.clip(_cubic(v1, v2, v3, v4, dy), 0.0, 255.0).astype(np.int64).astype(np.uint8)


def transform_mesh(img, nh, nw, strips):
    """Image.fromarray(img).transform((nw, nh), Image.MESH, the boxes and quads of `strips`, Image.BICUBIC) on uint8 [h, w, 3]."""
    out = np.zeros((nh, nw, 3), np.uint8)
    for x0, x1, a in strips:
        a = [float(c) for c in a]
        y, x = np.mgrid[0:nh, 0:x1 - x0]
        xin, yin = x + 0.5, y + 0.5
        with np.errstate(all='ignore'):
            sx = a[0] + a[1] * xin + a[2] * yin + a[3] * xin * yin
            sy = a[4] + a[5] * xin + a[6] * yin + a[7] * xin * yin
        inside, val = _sample(img, sx, sy)
        block = np.zeros((nh, x1 - x0, 3), np.uint8)
        block[inside] = val
        out[:, x0:x1] = block
    return out


# ---- the cases ----------------------------------------------------------------------------------------------------------------
SOURCES = [(1, 1), (2, 3), (5, 7), (37, 53)]            # (height, width); a call of every case names them by this index


def arc(n, x0, x1, y, height, bend, lean=0.0):
    """A text-like polygon of 2n points: the top edge from (x0, y) to (x1, y) bowed upwards by `bend` in the middle, the bottom edge
    `height` below it, its ends pulled in by `lean` — t0 .. t(n-1), b(n-1) .. b0."""
    ts = [i / (n - 1) for i in range(n)]
    top = [(x0 + (x1 - x0) * t, y - bend * (1.0 - (2.0 * t - 1.0) ** 2)) for t in ts]
    bottom = [(x + lean * (1.0 - 2.0 * t), yy + height) for (x, yy), t in zip(top, ts)]
    return tuple(top) + tuple(bottom[::-1])


def _shift(polygon, dx, dy):
    return tuple((x + dx, y + dy) for x, y in polygon)


_ARC10 = arc(5, 6.3, 45.1, 12.4, 14.2, 5.5, 2.0)

# (name, index into SOURCES, (h, w) of the output, polygon)
CASES = [
    ('one_pixel', 0, (1, 1), ((0.0, 0.0), (1.0, 0.0), (1.0, 1.0), (0.0, 1.0))),
    ('one_pixel_arc', 0, (9, 5), arc(3, -0.3, 1.2, 0.1, 0.9, 0.2)),
    ('two_by_three', 1, (9, 5), arc(3, 0.2, 2.8, 0.4, 1.4, 0.3)),
    ('five_by_seven', 2, (17, 33), arc(3, 0.4, 6.5, 1.3, 3.1, 0.9, 0.3)),
    ('quad', 3, (17, 33), ((8.3, 6.1), (44.7, 9.2), (42.1, 30.4), (6.5, 26.8))),
    ('arc6', 3, (17, 33), arc(3, 5.2, 47.6, 10.3, 15.5, 4.0, 1.5)),
    ('arc10', 3, (20, 50), _ARC10),
    ('arc14', 3, (13, 70), arc(7, 3.4, 49.8, 14.0, 12.5, 7.5, 2.5)),
    ('over_left', 3, (20, 50), _shift(_ARC10, -18.0, 0.0)),
    ('over_right', 3, (20, 50), _shift(_ARC10, 22.0, 0.0)),
    ('over_top', 3, (20, 50), _shift(_ARC10, 0.0, -14.0)),
    ('over_bottom', 3, (20, 50), _shift(_ARC10, 0.0, 17.0)),
    ('outside', 3, (9, 5), _shift(_ARC10, 100.0, 80.0)),
    # t1 and t2 (b1 and b2) are 0.05 apart on a polygon 40 long: the middle segment's two cuts coincide and it yields no strip
    ('vanishing', 3, (17, 33), ((5.0, 8.0), (24.0, 5.0), (24.05, 5.0), (45.0, 9.0), (44.0, 24.0), (24.05, 20.0), (24.0, 20.0), (6.0, 23.0))),
    ('one_wide', 3, (9, 1), arc(6, 8.0, 40.0, 12.0, 10.0, 3.0)),                # five segments, one column: one strip survives
    ('one_high', 3, (1, 33), arc(3, 5.2, 47.6, 10.3, 15.5, 4.0, 1.5)),
    ('several_tiles', 3, (40, 70), _ARC10),                                     # 3 x 5 tiles, the cuts inside tiles
    ('three_in_a_tile', 3, (17, 20), arc(7, 3.4, 49.8, 14.0, 12.5, 7.5, 2.5)),  # six strips over 20 columns
    ('cut_on_a_tile_edge', 3, (17, 32), ((5.0, 5.0), (20.0, 3.0), (35.0, 5.0), (35.0, 20.0), (20.0, 18.0), (5.0, 20.0))),      # two equal segments: the cut is 16
    ('sixty_four_strips', 3, (7, 97), tuple((2.0 + 0.75 * i, 9.0 + 3.0 * math.sin(0.21 * i)) for i in range(65))
     + tuple((2.5 + 0.75 * i, 21.0 + 3.0 * math.sin(0.21 * i)) for i in range(64, -1, -1))),
]
# the cases whose Pillow resize to TARGET is stored too (every output size once: the resized bytes are most of a fixture's weight)
RESIZED = ('one_pixel', 'two_by_three', 'five_by_seven', 'quad', 'arc14', 'over_top', 'outside', 'one_wide', 'one_high', 'several_tiles',
           'three_in_a_tile', 'sixty_four_strips')
MANY = 300                          # regions of the call whose tile table outgrows a workgroup's 256 work-items
MANY_SOURCE = 3


def many_regions():
    """[((h, w), polygon)] x MANY on SOURCES[MANY_SOURCE]: bowed 6-point polygons of every small size, some hanging over an edge."""
    rng = np.random.default_rng(2511)
    sh, sw = SOURCES[MANY_SOURCE]
    out = []
    for i in range(MANY):
        h, w = 1 + i % 5, 1 + (i // 5) % 7
        cx, cy = rng.uniform(-2.0, sw + 2.0), rng.uniform(-2.0, sh + 2.0)
        hw, hh = rng.uniform(1.0, 9.0), rng.uniform(1.0, 5.0)
        out.append(((h, w), arc(3, cx - hw, cx + hw, cy - hh, 2.0 * hh, rng.uniform(-0.3, 0.3) * hh, rng.uniform(-0.2, 0.2) * hw)))
    return out
