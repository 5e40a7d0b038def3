"""Input step on the device.

The reference's evaluation transform (strhub/data/module.py:69-82) is img.rotate(rotation, expand=True) when `rotation` is non-zero
-> Resize(img_size, BICUBIC) -> ToTensor -> Normalize(0.5, 0.5) on PIL images.  `resize_batch` is the first two steps (Pillow's
nearest-neighbour rotation and its 8-bit bicubic resampling, both bit-exact) as ONE HIP kernel over a ragged batch of uint8 HWC
images that already live in device memory; its uint8 [N, 3, H, W] result goes straight into `model(images)`, whose patch-embed
loader applies ToTensor + Normalize (images_dtype = PARSEQ_U8).  `rotation_map` is the host half of the rotation: Pillow's inverse
map as six 16.16 fixed-point integers, from the same float64 expressions Pillow evaluates, so the device does integer work only.

`rectify_resize_batch` is the step in front of all that for a caller with a text detector: quadrilateral regions
of full scenes, straightened as Pillow's Image.transform(PERSPECTIVE, BICUBIC) straightens them and resized, in one library call on
scenes that were uploaded once.  `region_size`, `quad_coeffs` and `map_to_source` are its host geometry, in float64.
"""
from __future__ import annotations

import math
import numbers
from typing import Sequence

import torch
from torch import Tensor

from . import _native

ROTATE_NONE, ROTATE_90, ROTATE_180, ROTATE_270, ROTATE_AFFINE = range(5)      # parseq_rotated_image_desc.mode
MAX_SIDE = 16384          # PARSEQ_ROTATE_MAX_SIDE: the map's 32-bit arithmetic holds to here (Pillow's own 16.16 fixed point to 32767)


def rotation_map(h: int, w: int, angle):
    """(mode, nh, nw, (a0 .. a5)) of PIL's Image.rotate(angle, expand=True) on an image of height h and width w: the rotated size
    and, for ROTATE_AFFINE, the integers with which output pixel (x, y) reads source pixel ((a2 + a0 x + a1 y) >> 16,
    (a5 + a3 x + a4 y) >> 16), black outside the source.  Multiples of 90 degrees are exact flips / transposes and carry no integers."""
    if not (1 <= h <= MAX_SIDE and 1 <= w <= MAX_SIDE):
        raise ValueError(f'image of {h} x {w}: each side must be in 1 .. {MAX_SIDE}')
    angle = angle % 360.0
    if angle == 0:
        return ROTATE_NONE, h, w, (0,) * 6
    if angle == 180:
        return ROTATE_180, h, w, (0,) * 6
    if angle in (90, 270):
        return (ROTATE_90 if angle == 90 else ROTATE_270), w, h, (0,) * 6
    a = -math.radians(angle)
    m = [round(math.cos(a), 15), round(math.sin(a), 15), 0.0, round(-math.sin(a), 15), round(math.cos(a), 15), 0.0]

    def transform(x, y):
        return m[0] * x + m[1] * y + m[2], m[3] * x + m[4] * y + m[5]
    m[2], m[5] = transform(-w / 2.0, -h / 2.0)          # rotate about the centre
    m[2] += w / 2.0
    m[5] += h / 2.0
    xs, ys = zip(*(transform(x, y) for x, y in ((0, 0), (w, 0), (w, h), (0, h))))
    nw = math.ceil(max(xs)) - math.floor(min(xs))
    nh = math.ceil(max(ys)) - math.floor(min(ys))
    if nh > MAX_SIDE or nw > MAX_SIDE:
        raise ValueError(f'image of {h} x {w} rotated by {angle} degrees is {nh} x {nw}: each side must be at most {MAX_SIDE}')
    m[2], m[5] = transform(-(nw - w) / 2.0, -(nh - h) / 2.0)      # expand=True: the same centre in the larger canvas

    def fix(v):
        return math.floor(v * 65536.0 + 0.5)
    return ROTATE_AFFINE, nh, nw, (fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5),
                                   fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def _checked(images: Sequence[Tensor]):
    if len(images) == 0:
        raise ValueError('empty batch')
    keep = []
    for i, im in enumerate(images):
        if not im.is_cuda:
            raise RuntimeError('resize_batch runs on the GPU (no CPU fallback); move the decoded images to the device first')
        if im.dtype != torch.uint8 or im.dim() != 3 or im.shape[2] != 3:
            raise ValueError(f'image {i}: expected uint8 [H, W, 3], got {im.dtype} {list(im.shape)}')
        if im.stride(2) != 1 or im.stride(1) != 3:
            im = im.contiguous()
        keep.append(im)
    return keep


def _angles(rotation, n: int):
    if isinstance(rotation, numbers.Real):
        return [rotation] * n
    angles = list(rotation)
    if len(angles) != n:
        raise ValueError(f'{len(angles)} rotations for {n} images')
    return angles


def _rotated_descs(images, angles):
    """The descriptor array of `images` (checked) turned by `angles`, and the rotated sizes."""
    descs = (_native.RotatedImageDesc * len(images))()
    sizes = []
    for d, im, angle in zip(descs, images, angles):
        mode, nh, nw, ints = rotation_map(im.shape[0], im.shape[1], angle)
        d.data = im.data_ptr()
        d.height, d.width, d.row_stride = im.shape[0], im.shape[1], im.stride(0)
        d.mode, d.rot_height, d.rot_width = mode, nh, nw
        d.a[:] = ints
        sizes.append((nh, nw))
    return descs, sizes


def rotate_batch(images: Sequence[Tensor], angle) -> list:
    """images: CUDA uint8 tensors [H_i, W_i, 3]; angle: degrees counter clockwise, one value or one per image.  Returns the uint8
    [nh_i, nw_i, 3] tensors PIL's Image.rotate(angle, expand=True) gives (parseq_op_rotate, one launch per image: the rotation on
    its own is the kernel tests' view of the map — `resize_batch(..., rotation=)` never materialises these)."""
    keep = _checked(images)
    dev = keep[0].device
    descs, sizes = _rotated_descs(keep, _angles(angle, len(keep)))
    lib = _native.lib()
    outs = [torch.empty((nh, nw, 3), dtype=torch.uint8, device=dev) for nh, nw in sizes]
    with _native.guard(dev):
        for i, out in enumerate(outs):
            _native.check(lib.parseq_op_rotate(descs[i], _native.ptr(out), _native.stream_ptr(dev)))
    return outs


def resize_batch(images: Sequence[Tensor], size=(32, 128), rotation=0) -> Tensor:
    """images: CUDA uint8 tensors [H_i, W_i, 3] (sizes may differ).  Returns uint8 [N, 3, size[0], size[1]].
    rotation: degrees counter clockwise (int or float), or one value per image: each image is first turned as PIL's
    Image.rotate(rotation, expand=True) turns it, inside the same launch."""
    keep = _checked(images)
    dev = keep[0].device
    n = len(keep)
    angles = _angles(rotation, n)
    plain = all(a % 360.0 == 0 for a in angles)          # nothing turns: the resize alone, as before there was a rotation
    descs = (_native.ImageDesc * n)() if plain else _rotated_descs(keep, angles)[0]
    lib = _native.lib()
    out = torch.empty((n, 3, size[0], size[1]), dtype=torch.uint8, device=dev)
    if plain:
        for d, im in zip(descs, keep):
            d.data = im.data_ptr()
            d.height, d.width, d.row_stride = im.shape[0], im.shape[1], im.stride(0)
        ws = torch.empty((lib.parseq_resize_workspace_bytes(n),), dtype=torch.uint8, device=dev)
        with _native.guard(dev):
            _native.check(lib.parseq_resize_bicubic(descs, n, size[0], size[1], _native.ptr(out), _native.ptr(ws), _native.stream_ptr(dev)))
    else:
        ws = torch.empty((lib.parseq_rotate_resize_workspace_bytes(n),), dtype=torch.uint8, device=dev)
        with _native.guard(dev):
            _native.check(lib.parseq_rotate_resize_bicubic(descs, n, size[0], size[1], _native.ptr(out), _native.ptr(ws), _native.stream_ptr(dev)))
    # the descriptor array is host memory read by an asynchronous copy: keep it (and the inputs) alive until the stream has passed
    torch.cuda.current_stream(dev).synchronize()
    return out


# ---- quadrilateral regions of a scene ------------------------------------------------------------------------
# A region is (image_index, quad): four points TL, TR, BR, BL as (x, y) floats in pixels of source image `image_index`, clockwise from
# the TEXT's own top-left — the corner order carries the orientation.  The geometry lives here, on the host, in float64; the library
# receives Pillow's eight PERSPECTIVE coefficients and does none of its own (as with `rotation_map`).
REGION_MAX_SIDE = 1024


def region_size(quad, max_side: int = REGION_MAX_SIDE):
    """(h, w) of the rectified crop of `quad`: its longer top / bottom edge and its longer left / right edge, rounded half up, each
    clamped to 1 .. max_side."""
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = [(float(x), float(y)) for x, y in quad]
    w = math.floor(max(math.hypot(x1 - x0, y1 - y0), math.hypot(x2 - x3, y2 - y3)) + 0.5)
    h = math.floor(max(math.hypot(x3 - x0, y3 - y0), math.hypot(x2 - x1, y2 - y1)) + 0.5)
    return min(max(h, 1), max_side), min(max(w, 1), max_side)


def _denominators(coeffs, h, w):
    return [coeffs[6] * x + coeffs[7] * y + 1.0 for x, y in ((0.0, 0.0), (float(w), 0.0), (float(w), float(h)), (0.0, float(h)))]


def check_coeffs(coeffs, h: int, w: int):
    """The eight coefficients as floats, or ValueError: one that is not finite, or a denominator a6 X + a7 Y + 1 that is not > 0 at a
    corner of the w x h output (it is linear in X and Y, so the corners speak for every pixel)."""
    coeffs = tuple(float(c) for c in coeffs)
    if len(coeffs) != 8:
        raise ValueError(f'{len(coeffs)} coefficients, a projective map has 8')
    if h < 1 or w < 1:
        raise ValueError(f'region of {h} x {w}: each side must be at least 1')
    if not all(math.isfinite(c) for c in coeffs):
        raise ValueError(f'coefficients {coeffs} are not all finite')
    if not all(d > 0.0 for d in _denominators(coeffs, h, w)):
        raise ValueError(f'the denominator of the map is not positive over the {h} x {w} output: the quadrilateral is not convex, is turned '
                         'inside out, or its vanishing line crosses the output')
    return coeffs


def quad_coeffs(quad, h: int, w: int):
    """Pillow's PERSPECTIVE data (a0 .. a7) for `quad`: output coordinates (X, Y) in [0, w] x [0, h] go to the source point
    ((a0 X + a1 Y + a2) / (a6 X + a7 Y + 1), (a3 X + a4 Y + a5) / (a6 X + a7 Y + 1)), with (0, 0) -> TL, (w, 0) -> TR, (w, h) -> BR, (0, h) -> BL.
    A parallelogram (TL + BR == TR + BL exactly) takes the closed form with a6 = a7 = 0, so that an integer axis-aligned box of its own
    size gives exactly (1, 0, left, 0, 1, top, 0, 0) — Pillow's bicubic truncates, and 1.0000000000000002 in place of 1.0 can turn a 200
    into a 199; everything else is a float64 solve of the 8 x 8 system.  ValueError for a quad that is not clockwise (a mirrored text), and
    for what `check_coeffs` refuses: a quad that is not convex, a bow tie, a vanishing line inside the output, anything not finite."""
    pts = [(float(x), float(y)) for x, y in quad]
    if len(pts) != 4:
        raise ValueError(f'a quadrilateral has 4 points, got {len(pts)}')
    if not all(math.isfinite(v) for p in pts for v in p):
        raise ValueError(f'quadrilateral {pts} is not finite')
    (x0, y0), (x1, y1), (x2, y2), (x3, y3) = pts
    # shoelace sum, y pointing down: positive for TL, TR, BR, BL in clockwise order
    area2 = sum(pts[i][0] * pts[(i + 1) % 4][1] - pts[(i + 1) % 4][0] * pts[i][1] for i in range(4))
    if not area2 > 0.0:
        raise ValueError(f'quadrilateral {pts} is not clockwise from the top-left (it is flipped or has no area)')
    if x0 + x2 == x1 + x3 and y0 + y2 == y1 + y3:
        coeffs = ((x1 - x0) / w, (x3 - x0) / h, x0, (y1 - y0) / w, (y3 - y0) / h, y0, 0.0, 0.0)
    else:
        import numpy as np
        m, rhs = np.zeros((8, 8)), np.zeros(8)
        for k, ((X, Y), (x, y)) in enumerate(zip(((0.0, 0.0), (float(w), 0.0), (float(w), float(h)), (0.0, float(h))), pts)):
            m[2 * k] = (X, Y, 1.0, 0.0, 0.0, 0.0, -X * x, -Y * x)
            m[2 * k + 1] = (0.0, 0.0, 0.0, X, Y, 1.0, -X * y, -Y * y)
            rhs[2 * k], rhs[2 * k + 1] = x, y
        try:
            coeffs = tuple(np.linalg.solve(m, rhs).tolist())
        except np.linalg.LinAlgError as e:
            raise ValueError(f'quadrilateral {pts} has no projective map: {e}') from None
    return check_coeffs(coeffs, h, w)


def map_to_source(coeffs, size, img_size, points):
    """The way back from the model's input to the scene: `points` (x, y) in pixels of the model's input (`img_size` = (h, w)) of a region
    rectified to `size` = (h, w) with `coeffs`, as [(x, y)] in pixels of the source image — the stretch of the resize undone, then the
    coefficient map, in float64."""
    a = [float(c) for c in coeffs]
    out = []
    for x, y in points:
        X, Y = x * size[1] / img_size[1], y * size[0] / img_size[0]
        den = a[6] * X + a[7] * Y + 1.0
        out.append(((a[0] * X + a[1] * Y + a[2]) / den, (a[3] * X + a[4] * Y + a[5]) / den))
    return out


def region_descs(regions, sizes=None, n_images=None):
    """[(image_index, (h, w), coeffs)] of `regions`: each (image_index, quad) — sized by `sizes[i]` or `region_size` — or
    (image_index, coeffs8, (h, w)) verbatim.  Everything the library would refuse is a ValueError here."""
    regions = list(regions)
    if len(regions) == 0:
        raise ValueError('no regions')
    if sizes is not None and len(sizes) != len(regions):
        raise ValueError(f'{len(sizes)} sizes for {len(regions)} regions')
    out = []
    for i, region in enumerate(regions):
        try:
            if len(region) == 3:
                index, coeffs, (h, w) = region
                if sizes is not None and sizes[i] is not None:
                    h, w = sizes[i]
                h, w = int(h), int(w)
                coeffs = check_coeffs(coeffs, h, w)
            else:
                index, quad = region
                h, w = sizes[i] if sizes is not None and sizes[i] is not None else region_size(quad)
                h, w = int(h), int(w)
                if h < 1 or w < 1:
                    raise ValueError(f'size {h} x {w}: each side must be at least 1')
                coeffs = quad_coeffs(quad, h, w)
        except ValueError as e:
            raise ValueError(f'region {i}: {e}') from None
        index = int(index)
        if n_images is not None and not 0 <= index < n_images:
            raise ValueError(f'region {i}: image index {index} is outside 0 .. {n_images - 1}')
        if h > MAX_SIDE or w > MAX_SIDE:
            raise ValueError(f'region {i}: size {h} x {w}, each side must be at most {MAX_SIDE}')
        out.append((index, (h, w), coeffs))
    return out


def _native_regions(keep, described):
    images = (_native.ImageDesc * len(keep))()
    for d, im in zip(images, keep):
        d.data = im.data_ptr()
        d.height, d.width, d.row_stride = im.shape[0], im.shape[1], im.stride(0)
    regions = (_native.RegionDesc * len(described))()
    for d, (index, (h, w), coeffs) in zip(regions, described):
        d.image, d.height, d.width = index, h, w
        d.coef[:] = coeffs
    return images, regions


def _slot(h, w):
    return (3 * h * w + 255) & ~255


def rectify_batch(images: Sequence[Tensor], regions, sizes=None) -> list:
    """images: CUDA uint8 tensors [H_i, W_i, 3], the scenes; regions: (image_index, quad) each (see `region_descs`).  Returns the uint8
    [h_i, w_i, 3] crops PIL's Image.transform((w, h), PERSPECTIVE, quad_coeffs(quad, h, w), BICUBIC) cuts out of them, all in one launch
    (parseq_rectify; views of one buffer).  The crops on their own are the kernel tests' view of the map — `rectify_resize_batch` never
    hands them out."""
    keep = _checked(images)
    dev = keep[0].device
    described = region_descs(regions, sizes, len(keep))
    image_descs, region_array = _native_regions(keep, described)
    lib = _native.lib()
    n = len(described)
    offsets, total = [], 0
    for _, (h, w), _ in described:
        offsets.append(total)
        total += _slot(h, w)
    flat = torch.empty((total,), dtype=torch.uint8, device=dev)
    outs = [flat[o:o + 3 * h * w].view(h, w, 3) for o, (_, (h, w), _) in zip(offsets, described)]
    pointers = (_native.C.c_void_p * n)(*[flat.data_ptr() + o for o in offsets])
    need = lib.parseq_rectify_workspace_bytes(region_array, n, len(keep))
    if need == 0:
        _native.check(-1)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    with _native.guard(dev):
        _native.check(lib.parseq_rectify(image_descs, len(keep), region_array, n, pointers, _native.ptr(ws), need, _native.stream_ptr(dev)))
    torch.cuda.current_stream(dev).synchronize()          # the three host arrays are read by asynchronous copies
    return outs


def rectify_resize_batch(images: Sequence[Tensor], regions, size=(32, 128), sizes=None) -> Tensor:
    """`resize_batch(rectify_batch(images, regions, sizes), size)` without the crops ever leaving the library's workspace: uint8
    [N, 3, size[0], size[1]], one row per region, the model's input."""
    keep = _checked(images)
    dev = keep[0].device
    described = region_descs(regions, sizes, len(keep))
    image_descs, region_array = _native_regions(keep, described)
    lib = _native.lib()
    n = len(described)
    out = torch.empty((n, 3, size[0], size[1]), dtype=torch.uint8, device=dev)
    need = lib.parseq_rectify_workspace_bytes(region_array, n, len(keep))
    if need == 0:
        _native.check(-1)
    ws = torch.empty((need,), dtype=torch.uint8, device=dev)
    with _native.guard(dev):
        _native.check(lib.parseq_rectify_resize_bicubic(image_descs, len(keep), region_array, n, size[0], size[1], _native.ptr(out), _native.ptr(ws), need,
                                                        _native.stream_ptr(dev)))
    torch.cuda.current_stream(dev).synchronize()
    return out
