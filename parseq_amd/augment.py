"""Training augmentation on the device: the RandAugment operators of the reference's training transform, bit-exact with Pillow.

The reference trains on `rand_augment_transform()` -> Resize(img_size, BICUBIC) -> ToTensor -> Normalize (strhub/data/module.py:69-82;
strhub/data/augment.py, aa_overrides.py: timm's auto_augment operators, i.e. calls into Pillow).  `augment_resize_batch` is the first
two steps on a ragged batch of uint8 HWC crops that already live in device memory: every image's chain of up to three operators runs
stage by stage (one launch per stage for the whole batch, csrc/augment.h), and the augmented crops go straight into the bicubic resize
of `preprocess.resize_batch` — the same kernel — so uint8 [N, 3, H, W] comes out with no host round trip.  `apply_batch` returns the
augmented crops themselves (parseq_op_augment, the kernel tests' view).

A chain is a list of at most three `(name, *args)` tuples:
    ('AutoContrast',)  ('Equalize',)  ('Invert',)                       ImageOps.autocontrast / equalize / invert
    ('Posterize', bits)  ('Solarize', thresh)  ('SolarizeAdd', add)     ImageOps.posterize (identity for bits >= 8) / solarize, timm's solarize_add
    ('Color', f)  ('Contrast', f)  ('Brightness', f)                    ImageEnhance.<Name>(img).enhance(f), f >= 0.1
    ('ShearX', f, r)  ('ShearY', f, r)                                  img.transform(img.size, AFFINE, ..., resample=r, fillcolor=(128,) * 3)
    ('TranslateXRel', pct, r)  ('TranslateYRel', pct, r)                the same, by pct of the width / height
    ('Rotate', deg, r)                                                  img.rotate(deg, resample=r, expand=True, fillcolor=(128,) * 3)
    ('GaussianBlur', radius)                                            img.filter(ImageFilter.GaussianBlur(radius)), 0 <= radius <= 4
    ('PoissonNoise', lam, seed)                                         imgaug's AdditivePoissonNoise(lam), restated; lam in 1 .. 41
with r = BILINEAR or BICUBIC.  The host halves are public: `lut_for` (the 256-entry tables, from Pillow's own integer and single-precision
steps), `affine_coeffs` and `rotate_expand_map` (the six float64 coefficients, from the Python expressions Pillow evaluates) and
`gaussian_box` (the radius and the two fixed-point weights of Pillow's box passes, from its single-precision steps).

PoissonNoise is a stated definition, not a pinned one (imgaug is not an oracle here): imgaug publishes AdditivePoissonNoise(lam) as
AddElementwise(RandomSign(Poisson(lam)), per_channel=False), so per pixel ONE draw n = +-k, k ~ Poisson(lam), both signs equally likely,
is added to R, G and B and the result clipped to 0 .. 255.  The draw is Philox4x32-10 keyed by `seed` (an unsigned 64-bit integer) with
the pixel's index as the counter: word 0 is the uniform, bit 31 of word 1 the sign, k the number of cumulative float64 thresholds at or
below the uniform (csrc/augment.h) — a function of (seed, pixel) alone, the same bytes every run.

`RandAugment` is the policy over the fourteen operators that were there first (`RandAugment.missing` names the other two; its draws are
what existing runs were trained with and do not change); `ReferenceRandAugment` is the reference's policy over all sixteen
(DESIGN.md sections 14 and 17).
"""
from __future__ import annotations

import math
from typing import Sequence

import numpy as np
import torch
from torch import Tensor

from . import _native
from .preprocess import MAX_SIDE, ROTATE_90, ROTATE_180, ROTATE_270, _checked, _workspace

BILINEAR, BICUBIC = 2, 3                                 # Pillow's Image.Resampling values (PARSEQ_AUG_BILINEAR / _BICUBIC)
OP_TABLE, OP_AUTOCONTRAST, OP_EQUALIZE, OP_CONTRAST, OP_COLOR, OP_AFFINE, OP_TURN = range(1, 8)      # PARSEQ_AUG_*
OP_GAUSSIAN_BLUR, OP_POISSON_NOISE = 8, 10               # 9 is no operator: the library refuses it
MAX_BLUR_RADIUS, MAX_NOISE_LAM = 4, 41                   # the policy's largest radius (magnitude 10); 40 | 1
MAX_OPS = 3                                              # PARSEQ_AUGMENT_MAX_OPS
TABLE_OPS = ('Invert', 'Posterize', 'Solarize', 'SolarizeAdd', 'Brightness')
GEOMETRIC_OPS = ('ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel', 'Rotate')
_ARITY = {'AutoContrast': 0, 'Equalize': 0, 'Invert': 0, 'Posterize': 1, 'Solarize': 1, 'SolarizeAdd': 1, 'Color': 1, 'Contrast': 1,
          'Brightness': 1, 'ShearX': 2, 'ShearY': 2, 'TranslateXRel': 2, 'TranslateYRel': 2, 'Rotate': 2, 'GaussianBlur': 1, 'PoissonNoise': 2}


def _factor(name: str, factor) -> np.float32:
    f = np.float32(factor)                               # Image.blend takes a C float
    if not (np.isfinite(f) and f >= np.float32(0.1)):
        raise ValueError(f'{name}: factor {factor} must be finite and at least 0.1')
    return f


def _int_arg(name: str, arg, lo: int, hi: int) -> int:
    if int(arg) != arg or not lo <= arg <= hi:
        raise ValueError(f'{name}: argument {arg} must be an integer in {lo} .. {hi}')
    return int(arg)


def lut_for(name: str, arg=None) -> np.ndarray:
    """The uint8 [256] table of a statistics-free operator, as Pillow builds it (Brightness: ImagingBlend's single-precision
    0 + f * (i - 0), truncated for f <= 1, clipped first above)."""
    i = np.arange(256, dtype=np.int32)
    if name == 'Invert':
        return (255 - i).astype(np.uint8)
    if name == 'Posterize':
        bits = _int_arg(name, arg, 0, 8)
        return (i & ~(2 ** (8 - bits) - 1) & 255).astype(np.uint8)       # bits = 8: the mask is ~0, the identity timm returns early
    if name == 'Solarize':
        thresh = _int_arg(name, arg, 0, 256)
        return np.where(i < thresh, i, 255 - i).astype(np.uint8)
    if name == 'SolarizeAdd':
        add = _int_arg(name, arg, 0, 128)
        return np.where(i < 128, np.minimum(255, i + add), i).astype(np.uint8)
    if name == 'Brightness':
        f = _factor(name, arg)
        if f == np.float32(1.0):
            return i.astype(np.uint8)
        t = np.float32(0.0) + f * i.astype(np.float32)
        if f > np.float32(1.0):
            t = np.clip(t, np.float32(0.0), np.float32(255.0))
        return t.astype(np.int32).astype(np.uint8)
    raise ValueError(f'{name} is not a table operator (one of {TABLE_OPS})')


def affine_coeffs(name: str, h: int, w: int, arg) -> tuple:
    """The six coefficients timm hands Image.transform(img.size, AFFINE, ...) for a shear or a relative translation of an h x w image:
    output pixel centre (x, y) samples the source at (a0 x + a1 y + a2, a3 x + a4 y + a5)."""
    arg = float(arg)
    if not math.isfinite(arg):
        raise ValueError(f'{name}: argument {arg} must be finite')
    if name == 'ShearX':
        return (1.0, arg, 0.0, 0.0, 1.0, 0.0)
    if name == 'ShearY':
        return (1.0, 0.0, 0.0, arg, 1.0, 0.0)
    if name == 'TranslateXRel':
        return (1.0, 0.0, arg * w, 0.0, 1.0, 0.0)
    if name == 'TranslateYRel':
        return (1.0, 0.0, 0.0, 0.0, 1.0, arg * h)
    raise ValueError(f'{name} is not a shear or a translation')


def rotate_expand_map(h: int, w: int, deg) -> tuple:
    """(turn, nh, nw, (a0 .. a5)) of PIL's Image.rotate(deg, resample, expand=True) with a BILINEAR or BICUBIC filter on an image of height
    h and width w.  Multiples of 90 degrees are Pillow's exact copies / transposes whatever the filter: turn is ROTATE_NONE (0),
    ROTATE_90, ROTATE_180 or ROTATE_270 and the coefficients are unused.  Any other angle gives turn = None and the float64 inverse map
    on the expanded nh x nw canvas, from the expressions Image.rotate evaluates."""
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f'image of {h} x {w}: each side must be in 1 .. {MAX_SIDE}')
    deg = float(deg)
    if not math.isfinite(deg):
        raise ValueError(f'Rotate: angle {deg} must be finite')
    angle = deg % 360.0
    if angle == 0:
        return 0, h, w, (0.0,) * 6
    if angle == 180:
        return ROTATE_180, h, w, (0.0,) * 6
    if angle in (90, 270):
        return (ROTATE_90 if angle == 90 else ROTATE_270), w, h, (0.0,) * 6
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def transform(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2], m[5] = transform(-w / 2.0, -h / 2.0)
    m[2] += w / 2.0
    m[5] += h / 2.0
    xs, ys = zip(*(transform(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs))
    nh = math.ceil(max(ys)) - math.floor(min(ys))
    if nh > MAX_SIDE or nw > MAX_SIDE:
        raise ValueError(f'image of {h} x {w} rotated by {deg} degrees is {nh} x {nw}: each side must be at most {MAX_SIDE}')
    m[2], m[5] = transform(-(nw - w) / 2.0, -(nh - h) / 2.0)
    return None, nh, nw, tuple(m)


def gaussian_box(radius) -> tuple:
    """(r, ww, fw) of the box pass Pillow runs three times along x and three times along y for ImageFilter.GaussianBlur(radius): the integer
    radius, the 8.24 fixed-point weight of the 2 r + 1 inner samples and that of the two samples at distance r + 1.  Pillow's
    _gaussian_blur_radius(radius, passes=3) and ImagingBoxBlur, in their single-precision steps."""
    f = np.float32
    radius = f(radius)
    if not (np.isfinite(radius) and 0 <= radius <= MAX_BLUR_RADIUS):
        raise ValueError(f'GaussianBlur: radius {radius} must be finite and in 0 .. {MAX_BLUR_RADIUS}')
    sigma2 = f(radius * radius / f(3.0))
    big = f(np.sqrt(f(f(12.0) * sigma2 + f(1.0))))
    l = f(np.floor(f((big - f(1.0)) / f(2.0))))
    a = f(f(f(2.0) * l + f(1.0)) * f(f(l * f(l + f(1.0))) - f(f(3.0) * sigma2)))
    a = f(a / f(f(6.0) * f(sigma2 - f(f(l + f(1.0)) * f(l + f(1.0))))))
    fr = f(l + a)
    r = int(fr)
    ww = int(np.uint32(f(1 << 24) / f(fr * f(2.0) + f(1.0))))
    fw = ((1 << 24) - (2 * r + 1) * ww) // 2
    return r, ww, fw


def _fill_op(op, h: int, w: int, name: str, args) -> tuple:
    """Writes one chain entry into `op` (an _native.AugmentOp); returns (used, nh, nw): used is False where the entry is the identity."""
    if name not in _ARITY:
        raise ValueError(f'unknown operator {name!r} (one of {tuple(_ARITY)})')
    if len(args) != _ARITY[name]:
        raise ValueError(f'{name} takes {_ARITY[name]} argument(s), got {len(args)}')
    op.mode, op.out_height, op.out_width = 0, h, w
    if name in TABLE_OPS:
        op.op = OP_TABLE
        op.arg.table[:] = lut_for(name, *args).tolist()
    elif name in ('AutoContrast', 'Equalize'):
        op.op = OP_AUTOCONTRAST if name == 'AutoContrast' else OP_EQUALIZE
    elif name in ('Color', 'Contrast'):
        op.op = OP_COLOR if name == 'Color' else OP_CONTRAST
        op.arg.factor = float(_factor(name, args[0]))
    elif name == 'GaussianBlur':
        r, ww, fw = gaussian_box(args[0])
        if float(args[0]) == 0:                          # ImageFilter.GaussianBlur(0) is a copy
            return False, h, w
        op.op = OP_GAUSSIAN_BLUR
        op.arg.blur.r, op.arg.blur.ww, op.arg.blur.fw = r, ww, fw
    elif name == 'PoissonNoise':
        lam = _int_arg(name, args[0], 1, MAX_NOISE_LAM)
        seed = args[1]
        if int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError(f'{name}: seed {seed} must be an unsigned 64-bit integer')
        op.op = OP_POISSON_NOISE
        op.arg.noise.p0, op.arg.noise.seed, op.arg.noise.lam = math.exp(-lam), int(seed), lam
    else:
        resample = args[1]
        if resample not in (BILINEAR, BICUBIC):
            raise ValueError(f'{name}: resample {resample} must be BILINEAR ({BILINEAR}) or BICUBIC ({BICUBIC})')
        if name == 'Rotate':
            turn, nh, nw, coef = rotate_expand_map(h, w, args[0])
            if turn == 0:
                return False, h, w
            op.out_height, op.out_width = nh, nw
            if turn is not None:
                op.op, op.mode = OP_TURN, turn
                return True, nh, nw
        else:
            coef = affine_coeffs(name, h, w, args[0])
        op.op, op.mode = OP_AFFINE, int(resample)
        op.arg.coef[:] = coef
    return True, op.out_height, op.out_width


def _descs(images, chains):
    """The descriptor array of `images` (checked) under `chains`, and every image's size after its chain."""
    chains = list(chains)
    if len(chains) != len(images):
        raise ValueError(f'{len(chains)} chains for {len(images)} images')
    descs = (_native.AugmentDesc * len(images))()
    sizes = []
    for i, (d, im, chain) in enumerate(zip(descs, images, chains)):
        chain = list(chain)
        if len(chain) > MAX_OPS:
            raise ValueError(f'image {i}: a chain holds at most {MAX_OPS} operators, got {len(chain)}')
        h, w = im.shape[0], im.shape[1]
        if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
            raise ValueError(f'image {i} of {h} x {w}: each side must be in 1 .. {MAX_SIDE}')
        d.data = im.data_ptr()
        d.height, d.width, d.row_stride = h, w, im.stride(0)
        n = 0
        for entry in chain:
            used, h, w = _fill_op(d.ops[n], h, w, entry[0], tuple(entry[1:]))
            n += used
        d.num_ops = n
        sizes.append((h, w))
    return descs, sizes


def apply_batch(images: Sequence[Tensor], chains) -> list:
    """images: CUDA uint8 tensors [H_i, W_i, 3]; chains[i]: at most three (name, *args) tuples.  Returns the augmented uint8
    [H'_i, W'_i, 3] tensors, each bit for bit what the Pillow calls of the module docstring give (parseq_op_augment, one chain per call)."""
    keep = _checked(images, 'apply_batch')
    dev = keep[0].device
    lib = _native.lib()
    outs, hold = [], []
    with _native.guard(dev):
        chains = list(chains)
        if len(chains) != len(keep):
            raise ValueError(f'{len(chains)} chains for {len(keep)} images')
        for im, chain in zip(keep, chains):
            descs, sizes = _descs([im], [chain])
            need = lib.parseq_augment_workspace_bytes(descs, 1)
            ws = _workspace(need, dev)
            out = torch.empty(sizes[0] + (3,), dtype=torch.uint8, device=dev)
            _native.check(lib.parseq_op_augment(descs, _native.ptr(out), _native.ptr(ws), need, _native.stream_ptr(dev)))
            outs.append(out)
            hold.append((descs, ws))
    torch.cuda.current_stream(dev).synchronize()         # the descriptors are host memory read by asynchronous copies
    return outs


def augment_resize_batch(images: Sequence[Tensor], chains, size=(32, 128)) -> Tensor:
    """images: CUDA uint8 tensors [H_i, W_i, 3] (sizes may differ); chains as for `apply_batch`.  Returns uint8 [N, 3, size[0], size[1]]:
    every image augmented, then resized as `resize_batch` resizes it, in one call (one launch per chain stage, then the resize kernel)."""
    keep = _checked(images, 'augment_resize_batch')
    dev = keep[0].device
    n = len(keep)
    descs, _ = _descs(keep, chains)
    lib = _native.lib()
    out = torch.empty((n, 3, size[0], size[1]), dtype=torch.uint8, device=dev)
    with _native.guard(dev):
        need = lib.parseq_augment_workspace_bytes(descs, n)
        ws = _workspace(need, dev)
        _native.check(lib.parseq_augment_resize_bicubic(descs, n, size[0], size[1], _native.ptr(out), _native.ptr(ws), need, _native.stream_ptr(dev)))
    torch.cuda.current_stream(dev).synchronize()         # the descriptor array is host memory read by an asynchronous copy
    return out


class RandAugment:
    """The policy of the reference's rand_augment_transform(magnitude, num_layers): per image, `num_layers` DISTINCT operators drawn
    uniformly (timm's RandAugment with choice weights, i.e. without replacement) from timm's increasing set minus SharpnessIncreasing,
    each applied with probability 0.5, signed arguments negated with probability 0.5, geometric operators with BILINEAR or BICUBIC at
    random (timm's _RANDOM_INTERPOLATION), fill colour (128, 128, 128).  The reference's set has two more operators, GaussianBlur and
    PoissonNoise (`missing`): the draw is among the fourteen of `ops`; `ReferenceRandAugment` draws among all sixteen.
    The generator is numpy's, seeded by `seed`; it makes no claim to reproduce the stream of timm's `random` / `np.random` calls."""

    ops = ('AutoContrast', 'Equalize', 'Invert', 'Rotate', 'Posterize', 'Solarize', 'SolarizeAdd', 'Color', 'Contrast', 'Brightness',
           'ShearX', 'ShearY', 'TranslateXRel', 'TranslateYRel')
    missing = ('GaussianBlur', 'PoissonNoise')
    _LEVEL_DENOM = 10.0
    # strhub/data/augment.py:102-108
    _SIGNED_MAX = {'Rotate': 30, 'ShearX': 0.9, 'ShearY': 0.2, 'TranslateXRel': 0.10, 'TranslateYRel': 0.30}

    def __init__(self, magnitude: float = 5, num_layers: int = 3, seed=None):
        if not 0 <= magnitude <= self._LEVEL_DENOM:
            raise ValueError(f'magnitude {magnitude} must be in 0 .. 10')
        if not 1 <= num_layers <= MAX_OPS:
            raise ValueError(f'num_layers {num_layers} must be in 1 .. {MAX_OPS}')
        self.magnitude, self.num_layers = magnitude, num_layers
        self.rng = np.random.default_rng(seed)

    def _negate(self, v):
        return -v if self.rng.random() > 0.5 else v

    def _args(self, name: str, h: int = 0, w: int = 0) -> tuple:
        """The arguments of `name` on an image of h x w (only the operators of `ReferenceRandAugment` look at the size)."""
        level = self.magnitude / self._LEVEL_DENOM
        if name in self._SIGNED_MAX:                       # aa_overrides.py _level_to_arg: (level / _LEVEL_DENOM) * max, randomly negated
            arg = self._negate(level * self._SIGNED_MAX[name])
            return (arg, BILINEAR if self.rng.random() < 0.5 else BICUBIC)
        if name == 'Posterize':                            # timm _posterize_increasing_level_to_arg
            return (4 - int(level * 4),)
        if name == 'Solarize':                             # timm _solarize_increasing_level_to_arg
            return (256 - min(256, int(level * 256)),)
        if name == 'SolarizeAdd':                          # timm _solarize_add_level_to_arg
            return (min(128, int(level * 110)),)
        if name in ('Color', 'Contrast', 'Brightness'):    # timm _enhance_increasing_level_to_arg
            return (max(0.1, 1.0 + self._negate(level * 0.9)),)
        return ()

    def sample(self, sizes) -> list:
        """One chain per (height, width) of `sizes`.  The size is followed through the chain — a Rotate expands it — and handed to `_args`:
        the fourteen operators of this class take relative arguments and draw the same whatever it is."""
        pool = self.ops
        chains = []
        for h, w in sizes:
            chain = []
            for j in self.rng.choice(len(pool), self.num_layers, replace=False):
                name = pool[j]
                if self.rng.random() > 0.5:                # timm AugmentOp: prob = 0.5
                    continue
                entry = (name,) + self._args(name, h, w)
                chain.append(entry)
                if name == 'Rotate':
                    _, h, w, _ = rotate_expand_map(h, w, entry[1])
            chains.append(chain)
        return chains


class ReferenceRandAugment(RandAugment):
    """The reference's whole policy: the sixteen operators of rand_augment_transform() (strhub/data/augment.py:78-112), GaussianBlur and
    PoissonNoise included, so `missing` is empty.  Their arguments follow strhub/data/augment.py:40-70 on the image as it is when the
    operator is reached: radius = round(min(4 m / 10, max(1, 0.02 max(h, w)))), lam = round(min(40 m / 10, max(1, 0.2 max(h, w)))) | 1,
    with Python's round.  The noise's seed is drawn from the policy's generator."""

    ops = RandAugment.ops + ('GaussianBlur', 'PoissonNoise')
    missing = ()

    @staticmethod
    def _param(level: float, h: int, w: int, max_dim_factor: float, min_level: float = 1) -> int:      # strhub/data/augment.py _get_param
        return round(min(level, max(min_level, max_dim_factor * max(h, w))))

    def _args(self, name: str, h: int = 0, w: int = 0) -> tuple:
        if name == 'GaussianBlur':                         # _level_to_arg: max * level / _LEVEL_DENOM
            return (self._param(4 * self.magnitude / self._LEVEL_DENOM, h, w, 0.02),)
        if name == 'PoissonNoise':
            return (self._param(40 * self.magnitude / self._LEVEL_DENOM, h, w, 0.2) | 1, int(self.rng.integers(0, 2 ** 64, dtype=np.uint64)))
        return super()._args(name, h, w)
