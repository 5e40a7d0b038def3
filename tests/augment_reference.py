"""NumPy restatement (test infrastructure) of the RandAugment operators of the reference's training transform
(strhub/data/augment.py, aa_overrides.py; the operators themselves are timm's auto_augment calls into Pillow).  It never calls the
library.  Pinned against Pillow's own outputs in tests/golden/augment_pillow.npz (tools/make_augment_golden.py).

Published algorithms, restated:
  * ImageOps.autocontrast / equalize / invert / posterize / solarize and timm's solarize_add: one 256-entry table per channel;
  * ImageEnhance.Color / Contrast / Brightness: Image.blend(degenerate, image, factor) in SINGLE precision, out = a + f (b - a),
    truncated for 0 <= f <= 1 and clipped to 0 .. 255 first otherwise; the degenerate image is convert('L') of the image (Color), the
    rounded mean of convert('L') (Contrast), black (Brightness); L = (R 19595 + G 38470 + B 7471 + 0x8000) >> 16;
  * Image.transform(AFFINE) with BILINEAR / BICUBIC: the inverse map at the pixel centre in float64, a pixel whose source position
    lies outside [0, W) x [0, H) keeps the fill colour, neighbours clamped at the edges (missing ROWS repeat the previous row's
    value), bilinear truncated, bicubic clipped then truncated;
  * Image.rotate(expand=True): 0 / 90 / 180 / 270 are exact copies / transposes whatever the filter, any other angle is that
    transform on the expanded canvas.
`SIZES`, `single_cases`, `CHAINS`, `BATCH` and `make_input` are the seeded cases the fixtures and tests/test_augment.py share.
"""
import math

import numpy as np

BILINEAR, BICUBIC = 2, 3                    # Pillow's Image.Resampling values
FILL = 128
GEOMETRIC = ('ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel', 'Rotate')
OPS = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast', 'Brightness',
       'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')

SIZES = [(1, 1), (1, 9), (3, 7), (17, 40), (32, 128), (61, 200)]        # (height, width)


def make_input(h: int, w: int) -> np.ndarray:
    """Seeded uint8 [h, w, 3]: a coarse ramp of 16 x 8 blocks, 40 .. 215, with one pixel in sixteen displaced by up to 45 — edges and
    isolated pixels for the filters, no degenerate statistics, and fixtures that still compress."""
    rng = np.random.default_rng(9000 * h + w)
    y, x = np.mgrid[0:h, 0:w]
    base = (40 + 8 * ((x // 16 + 3 * (y // 8)) % 16))[..., None] + np.array([0, 20, 40])
    noise = 15 * rng.integers(0, 4, (h, w, 3)) * (rng.integers(0, 16, (h, w, 1)) == 0)
    return (base + noise).astype(np.uint8)


def single_cases():
    """[(name, args)]: the magnitude-5 arguments with both signs, the extremes, both resamples."""
    cases = [('AutoContrast', ()), ('Equalize', ()), ('Invert', ())]
    cases += [('Posterize', (b,)) for b in (2, 0, 8)]
    cases += [('Solarize', (t,)) for t in (128, 0, 256)]
    cases += [('SolarizeAdd', (55,))]
    for name in ('Color', 'Contrast', 'Brightness'):
        cases += [(name, (f,)) for f in (1.45, 0.55, 0.1)]
    for name, mag in (('ShearX', 0.45), ('ShearY', 0.1), ('TranslateXRel', 0.05), ('TranslateYRel', 0.15), ('Rotate', 15.0)):
        cases += [(name, (sign * mag, r)) for sign in (1, -1) for r in (BILINEAR, BICUBIC)]
    return cases


def case_key(h, w, name, args):
    return f'{h}x{w}_{name}_' + '_'.join(str(a) for a in args)


# three operators each: one statistics, one table, one geometric; Rotate first, in the middle and last
CHAINS = [
    [('Rotate', 15.0, BICUBIC), ('AutoContrast',), ('Posterize', 2)],
    [('Equalize',), ('Rotate', -15.0, BILINEAR), ('Solarize', 128)],
    [('Contrast', 1.45), ('SolarizeAdd', 55), ('Rotate', 15.0, BILINEAR)],
    [('Invert',), ('ShearX', 0.45, BICUBIC), ('Equalize',)],
]
# the ragged batch of the fused augment-then-resize test: (size, chain)
BATCH = [((1, 1), [('Rotate', 15.0, BILINEAR)]), ((32, 128), []), ((17, 40), CHAINS[0]), ((61, 200), [('Color', 0.55)]),
         ((3, 7), [('TranslateYRel', 0.15, BICUBIC), ('Brightness', 1.45)]), ((1, 9), [('Equalize',), ('ShearY', -0.1, BILINEAR)]),
         ((32, 128), CHAINS[2])]


# ---- tables ---------------------------------------------------------------------------------------------------------------
def blend_f32(a, b, factor):
    """Image.blend(a, b, factor) on integer arrays: Pillow's ImagingBlend, float32 arithmetic."""
    f = np.float32(factor)
    a = np.asarray(a, np.int32)
    b = np.asarray(b, np.int32)
    if f == np.float32(1.0):
        return b.astype(np.uint8)
    t = a.astype(np.float32) + f * (b - a).astype(np.float32)
    if np.float32(0.0) <= f <= np.float32(1.0):
        return t.astype(np.int32).astype(np.uint8)
    return np.clip(t, np.float32(0.0), np.float32(255.0)).astype(np.int32).astype(np.uint8)


def table(name, arg=None):
    """The 256-entry table of a statistics-free operator."""
    i = np.arange(256)
    if name == 'Invert':
        return (255 - i).astype(np.uint8)
    if name == 'Posterize':
        return i.astype(np.uint8) if arg >= 8 else (i & ~(2 ** (8 - arg) - 1) & 255).astype(np.uint8)
    if name == 'Solarize':
        return np.where(i < arg, i, 255 - i).astype(np.uint8)
    if name == 'SolarizeAdd':
        return np.where(i < 128, np.minimum(255, i + arg), i).astype(np.uint8)
    if name == 'Brightness':
        return blend_f32(np.zeros(256, np.int32), i, arg)
    raise ValueError(name)


def luma(img):
    v = img.astype(np.int64)
    return (v[..., 0] * 19595 + v[..., 1] * 38470 + v[..., 2] * 7471 + 0x8000) >> 16


def autocontrast_table(hist):
    nz = np.nonzero(hist)[0]
    lo, hi = int(nz[0]), int(nz[-1])
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(ix * scale + offset))) for ix in range(256)], np.uint8)


def equalize_table(hist):
    nz = [int(v) for v in hist if v]
    if len(nz) <= 1:
        return np.arange(256, dtype=np.uint8)
    step = (sum(nz) - nz[-1]) // 255
    if not step:
        return np.arange(256, dtype=np.uint8)
    out, n = [], step // 2
    for i in range(256):
        out.append(n // step)
        n += int(hist[i])
    return np.minimum(np.array(out, np.int64), 255).astype(np.uint8)          # Image.point clips a table entry to 8 bits


# ---- geometry -------------------------------------------------------------------------------------------------------------
def affine_coeffs(name, h, w, arg):
    if name == 'ShearX':
        return (1, arg, 0, 0, 1, 0)
    if name == 'ShearY':
        return (1, 0, 0, arg, 1, 0)
    if name == 'TranslateXRel':
        return (1, 0, arg * w, 0, 1, 0)
    if name == 'TranslateYRel':
        return (1, 0, 0, 0, 1, arg * h)
    raise ValueError(name)


def rotate_matrix(h, w, angle):
    """(nh, nw, six float64) of Image.rotate(angle, expand=True) for an angle that is no multiple of 90 degrees."""
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
    return nh, nw, tuple(m)


def _cubic(v1, v2, v3, v4, d):
    p2 = -v1 + v3
    p3 = 2 * (v1 - v2) + v3 - v4
    p4 = -v1 + v2 - v3 + v4
    return v2 + d * (p2 + d * (p3 + d * p4))


def transform_affine(img, nh, nw, coeffs, resample):
    """Image.transform((nw, nh), AFFINE, coeffs, resample, fillcolor=(128, 128, 128)) on uint8 [h, w, 3]."""
    h, w = img.shape[:2]
    a = [float(c) for c in coeffs]
    y, x = np.mgrid[0:nh, 0:nw]
    xin, yin = x + 0.5, y + 0.5
    sx = a[0] * xin + a[1] * yin + a[2]
    sy = a[3] * xin + a[4] * yin + a[5]
    inside = (sx >= 0.0) & (sx < w) & (sy >= 0.0) & (sy < h)
    sx, sy = sx[inside] - 0.5, sy[inside] - 0.5          # only the pixels that are filtered: the rest keep the fill colour
    fx, fy = np.floor(sx).astype(np.int64), np.floor(sy).astype(np.int64)
    dx, dy = (sx - fx)[..., None], (sy - fy)[..., None]
    src = img.astype(np.float64)

    def cx(v):
        return np.clip(v, 0, w - 1)
    if resample == BILINEAR:
        def row(yy):
            yy = np.clip(yy, 0, h - 1)
            p, q = src[yy, cx(fx)], src[yy, cx(fx + 1)]
            return p + (q - p) * dx
        v1 = row(fy)
        v2 = np.where(((fy + 1 >= 0) & (fy + 1 < h))[..., None], row(fy + 1), v1)
        val = (v1 + (v2 - v1) * dy).astype(np.int64)
    elif resample == BICUBIC:
        def row(yy):
            yy = np.clip(yy, 0, h - 1)
            return _cubic(src[yy, cx(fx - 1)], src[yy, cx(fx)], src[yy, cx(fx + 1)], src[yy, cx(fx + 2)], dx)
        v1 = row(fy - 1)
        v2 = np.where(((fy >= 0) & (fy < h))[..., None], row(fy), v1)
        v3 = np.where(((fy + 1 >= 0) & (fy + 1 < h))[..., None], row(fy + 1), v2)
        v4 = np.where(((fy + 2 >= 0) & (fy + 2 < h))[..., None], row(fy + 2), v3)
        val = np.clip(_cubic(v1, v2, v3, v4, dy), 0.0, 255.0).astype(np.int64)
    else:
        raise ValueError(f'resample {resample}')
    out = np.full((nh, nw, 3), FILL, np.uint8)
    out[inside] = val.astype(np.uint8)
    return out


def rotate_expand(img, angle, resample):
    h, w = img.shape[:2]
    angle = angle % 360.0
    if angle == 0:
        return img.copy()
    if angle == 180:
        return np.ascontiguousarray(img[::-1, ::-1])
    if angle == 90:
        return np.ascontiguousarray(img.transpose(1, 0, 2)[::-1])
    if angle == 270:
        return np.ascontiguousarray(img.transpose(1, 0, 2)[:, ::-1])
    nh, nw, m = rotate_matrix(h, w, angle)
    return transform_affine(img, nh, nw, m, resample)


# ---- the operators --------------------------------------------------------------------------------------------------------
def apply_op(img: np.ndarray, name: str, *args) -> np.ndarray:
    """One operator of the table in the module docstring on uint8 [h, w, 3]."""
    h, w = img.shape[:2]
    if name in ('Invert', 'Posterize', 'Solarize', 'SolarizeAdd', 'Brightness'):
        return table(name, *args)[img]
    if name in ('AutoContrast', 'Equalize'):
        make = autocontrast_table if name == 'AutoContrast' else equalize_table
        return np.stack([make(np.bincount(img[..., c].ravel(), minlength=256))[img[..., c]] for c in range(3)], axis=-1)
    if name == 'Color':
        return blend_f32(luma(img)[..., None], img, args[0])
    if name == 'Contrast':
        lum = luma(img)
        mean = int(float(lum.sum()) / lum.size + 0.5)
        return blend_f32(np.full(256, mean), np.arange(256), args[0])[img]
    if name == 'Rotate':
        return rotate_expand(img, args[0], args[1])
    return transform_affine(img, h, w, affine_coeffs(name, h, w, args[0]), args[1])


def apply_chain(img: np.ndarray, chain) -> np.ndarray:
    for op in chain:
        img = apply_op(img, op[0], *op[1:])
    return img
