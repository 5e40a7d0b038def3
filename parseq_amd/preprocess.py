"""Input step on the device.

The reference's evaluation transform (strhub/data/module.py:69-82) is img.rotate(rotation, expand=True) when `rotation` is non-zero
-> Resize(img_size, BICUBIC) -> ToTensor -> Normalize(0.5, 0.5) on PIL images.  `resize_batch` is the first two steps (Pillow's
nearest-neighbour rotation and its 8-bit bicubic resampling, both bit-exact) as ONE HIP kernel over a ragged batch of uint8 HWC
images that already live in device memory; its uint8 [N, 3, H, W] result goes straight into `model(images)`, whose patch-embed
loader applies ToTensor + Normalize (images_dtype = PARSEQ_U8).  `rotation_map` is the host half of the rotation: Pillow's inverse
map as six 16.16 fixed-point integers, from the same float64 expressions Pillow evaluates, so the device does integer work only.
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
