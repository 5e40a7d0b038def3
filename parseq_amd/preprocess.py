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

`mesh_rectify_resize_batch` is the same step for a detector of curved text: polygons of 2N points, straightened
strip by strip as Pillow's Image.transform(MESH, BICUBIC) straightens them.  `polygon_size`, `polygon_mesh` and `mesh_to_source` are its
host geometry.
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


def _checked(images: Sequence[Tensor], what: str):
    """`images` as the library reads them (uint8 [H, W, 3] on the device, pixels packed), for the public function `what`."""
    if len(images) == 0:
        raise ValueError('empty batch')
    keep = []
    for i, im in enumerate(images):
        if not im.is_cuda:
            raise RuntimeError(f'{what} runs on the GPU (no CPU fallback); move the decoded images to the device first')
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


def _workspace(need: int, dev) -> Tensor:
    """The workspace a *_workspace_bytes function asked for; 0 means the library refused the descriptors: its message is raised."""
    if need == 0:
        _native.check(-1)
    return torch.empty((need,), dtype=torch.uint8, device=dev)


def _image_descs(keep):
    images = (_native.ImageDesc * len(keep))()
    for d, im in zip(images, keep):
        d.data = im.data_ptr()
        d.height, d.width, d.row_stride = im.shape[0], im.shape[1], im.stride(0)
    return images


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
    keep = _checked(images, 'rotate_batch')
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
    keep = _checked(images, 'resize_batch')
    dev = keep[0].device
    n = len(keep)
    angles = _angles(rotation, n)
    lib = _native.lib()
    if all(a % 360.0 == 0 for a in angles):              # nothing turns: the resize alone, as before there was a rotation
        descs, query, call = _image_descs(keep), lib.parseq_resize_workspace_bytes, lib.parseq_resize_bicubic
    else:
        descs, query, call = _rotated_descs(keep, angles)[0], lib.parseq_rotate_resize_workspace_bytes, lib.parseq_rotate_resize_bicubic
    out = torch.empty((n, 3, size[0], size[1]), dtype=torch.uint8, device=dev)
    ws = torch.empty((query(n),), dtype=torch.uint8, device=dev)
    with _native.guard(dev):
        _native.check(call(descs, n, size[0], size[1], _native.ptr(out), _native.ptr(ws), _native.stream_ptr(dev)))
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


def _described(regions, sizes, n_images, verbatim, from_shape, default_size):
    """[(image_index, (h, w), map)] of `regions`, quadrilaterals or polygons alike: each is (image_index, shape) — sized by `sizes[i]` or
    `default_size(shape)`, its map `from_shape(shape, h, w)` — or (image_index, map, (h, w)) verbatim, its map `verbatim(map, h, w)`."""
    regions = list(regions)
    if len(regions) == 0:
        raise ValueError('no regions')
    if sizes is not None and len(sizes) != len(regions):
        raise ValueError(f'{len(sizes)} sizes for {len(regions)} regions')
    out = []
    for i, region in enumerate(regions):
        given = sizes[i] if sizes is not None else None
        try:
            if len(region) == 3:
                index, described, (h, w) = region
                h, w = (int(v) for v in (given if given is not None else (h, w)))
                described = verbatim(described, h, w)
            else:
                index, shape = region
                h, w = (int(v) for v in (given if given is not None else default_size(shape)))
                if h < 1 or w < 1:
                    raise ValueError(f'size {h} x {w}: each side must be at least 1')
                described = from_shape(shape, h, w)
        except ValueError as e:
            raise ValueError(f'region {i}: {e}') from None
        index = int(index)
        if n_images is not None and not 0 <= index < n_images:
            raise ValueError(f'region {i}: image index {index} is outside 0 .. {n_images - 1}')
        if h > MAX_SIDE or w > MAX_SIDE:
            raise ValueError(f'region {i}: size {h} x {w}, each side must be at most {MAX_SIDE}')
        out.append((index, (h, w), described))
    return out


def region_descs(regions, sizes=None, n_images=None):
    """[(image_index, (h, w), coeffs)] of `regions`: each (image_index, quad) — sized by `sizes[i]` or `region_size` — or
    (image_index, coeffs8, (h, w)) verbatim.  Everything the library would refuse is a ValueError here."""
    return _described(regions, sizes, n_images, check_coeffs, quad_coeffs, region_size)


def _native_regions(keep, described):
    images = _image_descs(keep)
    regions = (_native.RegionDesc * len(described))()
    for d, (index, (h, w), coeffs) in zip(regions, described):
        d.image, d.height, d.width = index, h, w
        d.coef[:] = coeffs
    return images, regions


def _region_call(keep, described, arrays, query, call, size=None):
    """One library call over the regions `described` of the scenes `keep`.  `arrays`: the descriptor arrays (images, regions and, for
    polygons, strips); `query`: the call's *_workspace_bytes function; `call`: the library function.
    With `size` the regions are resized into one uint8 [N, 3, size[0], size[1]] tensor, which is returned; without, they are
    returned themselves: uint8 [h_i, w_i, 3] views of one buffer, each on a 256-byte boundary."""
    dev = keep[0].device
    n, n_images = len(described), len(keep)
    images, *others = arrays
    counted = [v for a in others for v in (a, len(a))]            # regions, n[, strips, n_strips]
    if size is None:
        offsets, total = [], 0
        for _, (h, w), _ in described:
            offsets.append(total)
            total += (3 * h * w + 255) & ~255
        flat = torch.empty((total,), dtype=torch.uint8, device=dev)
        result = [flat[o:o + 3 * h * w].view(h, w, 3) for o, (_, (h, w), _) in zip(offsets, described)]
        target = ((_native.C.c_void_p * n)(*[flat.data_ptr() + o for o in offsets]),)
    else:
        result = torch.empty((n, 3, size[0], size[1]), dtype=torch.uint8, device=dev)
        target = (size[0], size[1], _native.ptr(result))
    need = query(*counted, n_images)
    ws = _workspace(need, dev)
    with _native.guard(dev):
        _native.check(call(images, n_images, *counted, *target, _native.ptr(ws), need, _native.stream_ptr(dev)))
    torch.cuda.current_stream(dev).synchronize()          # the host arrays are read by asynchronous copies
    return result


def rectify_batch(images: Sequence[Tensor], regions, sizes=None) -> list:
    """images: CUDA uint8 tensors [H_i, W_i, 3], the scenes; regions: (image_index, quad) each (see `region_descs`).  Returns the uint8
    [h_i, w_i, 3] crops PIL's Image.transform((w, h), PERSPECTIVE, quad_coeffs(quad, h, w), BICUBIC) cuts out of them, all in one launch
    (parseq_rectify; views of one buffer).  The crops on their own are the kernel tests' view of the map — `rectify_resize_batch` never
    hands them out."""
    keep = _checked(images, 'rectify_batch')
    described = region_descs(regions, sizes, len(keep))
    lib = _native.lib()
    return _region_call(keep, described, _native_regions(keep, described), lib.parseq_rectify_workspace_bytes, lib.parseq_rectify)


def rectify_resize_batch(images: Sequence[Tensor], regions, size=(32, 128), sizes=None) -> Tensor:
    """`resize_batch(rectify_batch(images, regions, sizes), size)` without the crops ever leaving the library's workspace: uint8
    [N, 3, size[0], size[1]], one row per region, the model's input."""
    keep = _checked(images, 'rectify_resize_batch')
    described = region_descs(regions, sizes, len(keep))
    lib = _native.lib()
    return _region_call(keep, described, _native_regions(keep, described), lib.parseq_rectify_workspace_bytes, lib.parseq_rectify_resize_bicubic, size)


# ---- polygon regions of a scene --------------------------------------------------------------------------------
# A polygon is 2N points (x, y), N >= 2, clockwise from the TEXT's own top-left as above: top[0 .. N-1] left to right, then
# bottom[N-1 .. 0] right to left — what a detector of curved text returns.  It is N - 1 quadrilaterals side by side, each painted into its
# own strip of output columns through Pillow's bilinear QUAD map: Image.transform(size, Image.MESH, ...).  The rungs top[i] - bottom[i]
# are shared by neighbouring strips, so the map is continuous across the seams.  A 4-point polygon is a one-strip mesh: a BILINEAR map
# of the quadrilateral, not section 22's projective one — the two differ on a trapezoid by design.
MESH_MAX_STRIPS = _native.MESH_MAX_STRIPS          # PARSEQ_MESH_MAX_STRIPS


def _polygon_sides(polygon):
    """(top, bottom), both left to right, as float pairs; ValueError for an odd number of points, fewer than four, or a value not finite."""
    pts = [(float(x), float(y)) for x, y in polygon]
    if len(pts) < 4 or len(pts) % 2:
        raise ValueError(f'a polygon has an even number of points, at least 4 (N along the top, N back along the bottom), got {len(pts)}')
    if not all(math.isfinite(v) for p in pts for v in p):
        raise ValueError(f'polygon {pts} is not finite')
    n = len(pts) // 2
    return pts[:n], pts[:n - 1:-1]


def _dist(p, q):
    return math.hypot(q[0] - p[0], q[1] - p[1])


def polygon_size(polygon, max_side: int = REGION_MAX_SIDE):
    """(h, w) of the rectified crop of `polygon`: w the longer of its top and bottom polylines, h its longest rung |top[i] - bottom[i]|,
    rounded half up, each clamped to 1 .. max_side (the rule of `region_size`)."""
    top, bottom = _polygon_sides(polygon)
    along = max(sum(_dist(side[i], side[i + 1]) for i in range(len(side) - 1)) for side in (top, bottom))
    w = math.floor(along + 0.5)
    h = math.floor(max(_dist(t, b) for t, b in zip(top, bottom)) + 0.5)
    return min(max(h, 1), max_side), min(max(w, 1), max_side)


def quad_strip_coeffs(x0: int, x1: int, h: int, nw, sw, se, ne):
    """What Pillow's Image.__transformer derives for QUAD from the box (x0, 0, x1, h) and the corners NW, SW, SE, NE, in its own
    expression order (the stored bytes depend on the last bit of these numbers)."""
    x0s, y0s = nw
    As = 1.0 / (x1 - x0)
    At = 1.0 / h
    return (x0s, (ne[0] - x0s) * As, (sw[0] - x0s) * At, (se[0] - sw[0] - ne[0] + x0s) * As * At,
            y0s, (ne[1] - y0s) * As, (sw[1] - y0s) * At, (se[1] - sw[1] - ne[1] + y0s) * As * At)


def polygon_mesh(polygon, h: int, w: int):
    """The strips [(x0, x1, coef8)] of `polygon` in an output of h x w.  Segment i weighs the mean length of top[i] -> top[i+1] and
    bottom[i] -> bottom[i+1]; the cuts are cut[0] = 0, cut[N-1] = w and floor(cum_i / total * w + 0.5) in between; a segment whose cuts
    coincide yields no strip, so the strips tile [0, w) exactly, each at least one column wide.  Strip i is Pillow's box
    (cut[i], 0, cut[i+1], h) with the quad NW = top[i], SW = bottom[i], SE = bottom[i+1], NE = top[i+1].  ValueError for what has no such
    mesh: a total weight of 0, a strip whose quad is not clockwise (mirrored or folded text), more than MESH_MAX_STRIPS strips."""
    top, bottom = _polygon_sides(polygon)
    h, w = int(h), int(w)
    if h < 1 or w < 1:
        raise ValueError(f'size {h} x {w}: each side must be at least 1')
    n = len(top)
    weights = [0.5 * (_dist(top[i], top[i + 1]) + _dist(bottom[i], bottom[i + 1])) for i in range(n - 1)]
    total = 0.0
    for v in weights:
        total += v
    if not total > 0.0:
        raise ValueError(f'polygon {top + bottom[::-1]} has no length: every segment weighs 0')
    cuts, cum = [0], 0.0
    for v in weights[:-1]:
        cum += v
        cuts.append(math.floor(cum / total * w + 0.5))
    cuts.append(w)
    strips = []
    for i in range(n - 1):
        if cuts[i + 1] <= cuts[i]:
            continue
        quad = (top[i], top[i + 1], bottom[i + 1], bottom[i])
        area2 = sum(quad[k][0] * quad[(k + 1) % 4][1] - quad[(k + 1) % 4][0] * quad[k][1] for k in range(4))
        if not area2 > 0.0:
            raise ValueError(f'segment {i} of the polygon, {quad}, is not clockwise from the top-left (the text is mirrored or folded there)')
        strips.append((cuts[i], cuts[i + 1], quad_strip_coeffs(cuts[i], cuts[i + 1], h, top[i], bottom[i], bottom[i + 1], top[i + 1])))
    if len(strips) > MESH_MAX_STRIPS:
        raise ValueError(f'{len(strips)} strips, at most {MESH_MAX_STRIPS}')
    return strips


def check_strips(strips, h: int, w: int):
    """The strips as [(int, int, 8 floats)], or ValueError: none or more than MESH_MAX_STRIPS, a coefficient that is not finite, strips
    that do not tile [0, w) in order without gap or overlap."""
    if h < 1 or w < 1:
        raise ValueError(f'region of {h} x {w}: each side must be at least 1')
    out = []
    for x0, x1, coef in strips:
        coef = tuple(map(float, coef))
        if len(coef) != 8:
            raise ValueError(f'{len(coef)} coefficients, a bilinear map has 8')
        if not all(map(math.isfinite, coef)):
            raise ValueError(f'coefficients {coef} are not all finite')
        out.append((int(x0), int(x1), coef))
    if not 1 <= len(out) <= MESH_MAX_STRIPS:
        raise ValueError(f'{len(out)} strips, a region has 1 .. {MESH_MAX_STRIPS}')
    at = 0
    for x0, x1, _ in out:
        if x0 != at or x1 <= x0:
            raise ValueError(f'strip of columns {x0} .. {x1} where {at} begins: the strips must tile 0 .. {w} in order without gap or overlap')
        at = x1
    if at != w:
        raise ValueError(f'the strips end at column {at}: they must tile 0 .. {w}')
    return out


def mesh_to_source(strips, size, img_size, points):
    """The way back from the model's input to the scene, as `map_to_source`: `points` (x, y) in pixels of the model's input (`img_size` =
    (h, w)) of a region rectified to `size` = (h, w) with `strips`, as [(x, y)] in pixels of the source image — the stretch of the resize
    undone, the strip chosen by X (the last one also owns X = w, and what lies beyond either end continues the outermost strip), then its
    bilinear map at (X - x0, Y), without the half-pixel shift, in float64."""
    strips = list(strips)
    out = []
    for x, y in points:
        X, Y = x * size[1] / img_size[1], y * size[0] / img_size[0]
        x0, _, a = next((s for s in strips[:-1] if X < s[1]), strips[-1])
        u = X - x0
        out.append((a[0] + a[1] * u + a[2] * Y + a[3] * u * Y, a[4] + a[5] * u + a[6] * Y + a[7] * u * Y))
    return out


def polygon_descs(regions, sizes=None, n_images=None):
    """[(image_index, (h, w), strips)] of `regions`: each (image_index, polygon) — sized by `sizes[i]` or `polygon_size` — or
    (image_index, strips, (h, w)) verbatim.  Everything the library would refuse is a ValueError here, naming the region."""
    return _described(regions, sizes, n_images, check_strips, polygon_mesh, polygon_size)


def _native_mesh(keep, described):
    images = _image_descs(keep)
    regions = (_native.MeshRegionDesc * len(described))()
    strips = (_native.MeshStrip * sum(len(s) for _, _, s in described))()
    at = 0
    for d, (index, (h, w), region_strips) in zip(regions, described):
        d.image, d.height, d.width, d.first_strip, d.n_strips = index, h, w, at, len(region_strips)
        for x0, x1, coef in region_strips:
            strips[at].x0, strips[at].x1 = x0, x1
            strips[at].coef[:] = coef
            at += 1
    return images, regions, strips


def mesh_rectify_batch(images: Sequence[Tensor], regions, sizes=None) -> list:
    """images: CUDA uint8 tensors [H_i, W_i, 3], the scenes; regions: (image_index, polygon) each (see `polygon_descs`).  Returns the uint8
    [h_i, w_i, 3] crops PIL's Image.transform((w, h), MESH, the boxes and quads of polygon_mesh(polygon, h, w), BICUBIC) cuts out of them, all
    in one launch (parseq_mesh_rectify; views of one buffer), as `rectify_batch` does for quadrilaterals."""
    keep = _checked(images, 'mesh_rectify_batch')
    described = polygon_descs(regions, sizes, len(keep))
    lib = _native.lib()
    return _region_call(keep, described, _native_mesh(keep, described), lib.parseq_mesh_rectify_workspace_bytes, lib.parseq_mesh_rectify)


def mesh_rectify_resize_batch(images: Sequence[Tensor], regions, size=(32, 128), sizes=None) -> Tensor:
    """`resize_batch(mesh_rectify_batch(images, regions, sizes), size)` without the crops ever leaving the library's workspace: uint8
    [N, 3, size[0], size[1]], one row per region, the model's input."""
    keep = _checked(images, 'mesh_rectify_resize_batch')
    described = polygon_descs(regions, sizes, len(keep))
    lib = _native.lib()
    return _region_call(keep, described, _native_mesh(keep, described), lib.parseq_mesh_rectify_workspace_bytes, lib.parseq_mesh_rectify_resize_bicubic,
                        size)


# ---- turned views of a crop -------------------------------------------------------------------------------------
# A reader that does not know which way up a crop is reads it in a few quarter turns and keeps the reading the model trusts most
# (`model.orient`).  The views are made here: Pillow-exact quarter turns fused into the resize, every source uploaded once.
ORIENTATION_MODES = ('flip', 'auto', 'all')


def orientation_angles(sizes, mode: str, tall: float = 1.5):
    """The angles (degrees counter clockwise, as `resize_batch(rotation=)` takes them) of the views of crops of `sizes` [(h, w)]: one
    tuple per crop, the upright guess first.  'flip': (0, 180); 'all': (0, 90, 180, 270); 'auto': (90, 270) for a crop with h > tall * w
    — vertical text — and (0, 180) otherwise, so every crop has two views."""
    if mode not in ORIENTATION_MODES:
        raise ValueError(f'orientation mode must be one of {ORIENTATION_MODES}, got {mode!r}')
    if not (isinstance(tall, numbers.Real) and math.isfinite(tall) and tall > 0):
        raise ValueError(f'tall must be a positive number, got {tall!r}')
    if mode == 'flip':
        return [(0, 180) for _ in sizes]
    if mode == 'all':
        return [(0, 90, 180, 270) for _ in sizes]
    return [(90, 270) if h > tall * w else (0, 180) for h, w in sizes]


def orientation_views(images: Sequence[Tensor], mode: str = 'flip', size=(32, 128), tall: float = 1.5, rotation=0):
    """images: CUDA uint8 tensors [H_i, W_i, 3].  Returns (views uint8 [B, K, 3, size[0], size[1]], angles): view k of crop b is
    `resize_batch([images[b]], size, rotation=rotation + angles[b][k])`.  One parseq_rotate_resize_bicubic launch over B * K descriptors;
    the K descriptors of a crop point at the one copy of its pixels.  `rotation` (degrees, one value; test.py --rotation) turns every crop
    before its views are taken: each view is ONE Pillow rotation by the sum of the two angles, and 'auto' judges the turned crop's shape."""
    keep = _checked(images, 'orientation_views')
    dev = keep[0].device
    angles = orientation_angles([rotation_map(im.shape[0], im.shape[1], rotation)[1:3] for im in keep], mode, tall)
    K = len(angles[0])
    n = len(keep) * K
    descs, _ = _rotated_descs([im for im in keep for _ in range(K)], [rotation + a for per_crop in angles for a in per_crop])
    lib = _native.lib()
    out = torch.empty((len(keep), K, 3, size[0], size[1]), dtype=torch.uint8, device=dev)
    ws = torch.empty((lib.parseq_rotate_resize_workspace_bytes(n),), dtype=torch.uint8, device=dev)
    with _native.guard(dev):
        _native.check(lib.parseq_rotate_resize_bicubic(descs, n, size[0], size[1], _native.ptr(out), _native.ptr(ws), _native.stream_ptr(dev)))
    torch.cuda.current_stream(dev).synchronize()          # the descriptor array is host memory read by an asynchronous copy
    return out, angles


def rotated_size(angle, size):
    """(h, w) of an image of `size` = (h, w) turned by a multiple of 90 degrees."""
    return (size[1], size[0]) if angle % 180 == 90 else (size[0], size[1])


def unrotate_points(angle, size, points):
    """The way back from a turned image to its source: `points` (x, y) in pixels of the image Image.rotate(angle, expand=True) makes of a
    source of `size` = (h, w), angle a multiple of 90 degrees, as [(x, y)] in pixels of the source.  A pixel's area maps onto the area of
    the pixel it was copied from: (x' + 0.5, y' + 0.5) goes to the centre of the source pixel of (x', y')."""
    h, w = size
    angle = angle % 360
    if angle not in (0, 90, 180, 270):
        raise ValueError(f'unrotate_points: {angle} degrees is not a multiple of 90')
    if angle == 0:
        return [(x, y) for x, y in points]
    if angle == 90:
        return [(w - y, x) for x, y in points]
    if angle == 180:
        return [(w - x, h - y) for x, y in points]
    return [(y, h - x) for x, y in points]


def shift_quad(quad, k: int):
    """View k of a quadrilateral: its corner list shifted cyclically by k, so that corner k becomes the text's top-left.  The rectified
    crop of shift k is the crop of shift 0 turned by 90 k degrees counter clockwise (shift 1: what was the top-right corner is now the
    top-left), and `region_size` swaps height and width under an odd shift."""
    quad = list(quad)
    if len(quad) != 4:
        raise ValueError(f'a quadrilateral has 4 points, got {len(quad)}')
    k %= 4
    return quad[k:] + quad[:k]


def orientation_regions(regions, mode: str = 'flip', tall: float = 1.5):
    """The views of quadrilateral regions [(image_index, quad)] for `rectify_resize_batch`: (regions of all views, crop-major; the shifts of
    every region).  The shifts are the angles of `orientation_angles` on the `region_size` of each quad, divided by 90."""
    regions = [(index, list(quad)) for index, quad in regions]
    angles = orientation_angles([region_size(quad) for _, quad in regions], mode, tall)
    shifts = [tuple(a // 90 for a in per_region) for per_region in angles]
    return [(index, shift_quad(quad, k)) for (index, quad), per_region in zip(regions, shifts) for k in per_region], shifts


# ---- long text lines -------------------------------------------------------------------------------------------
# A line wider than the model's input is read as overlapping windows of the width the model was made for; `model.read_lines` reads them as
# one batch and stitches the characters by position on the device.  The plan is made here, on the host, in float64 and integers.
LINE_MAX_WINDOWS = _native.LINE_MAX_WINDOWS          # PARSEQ_LINE_MAX_WINDOWS


def line_windows(h: int, w: int, img_size=(32, 128), overlap: float = 0.25, aspect: float = 1.0):
    """[(x0, ww)] — the windows of a line of `h` x `w` pixels, left to right: window k is the columns x0 .. x0 + ww - 1.  The width
    ww = max(1, floor(h img_w / img_h aspect + 1/2)) is what the resize maps onto the model's input without distortion (`aspect` stretches
    it); a line no wider than that is one window (0, w), the crop as `resize_batch` reads it.  Otherwise neighbours share
    ov = floor(ww overlap + 1/2) columns: the stride is s = max(1, ww - ov), there are ceil((w - ww) / s) + 1 windows, and the last one is
    right-aligned.  ValueError: sizes below 1, `overlap` outside [0, 0.75], `aspect` outside [0.25, 4], more than LINE_MAX_WINDOWS windows."""
    h, w, img_h, img_w = int(h), int(w), int(img_size[0]), int(img_size[1])
    if h < 1 or w < 1 or img_h < 1 or img_w < 1:
        raise ValueError(f'line_windows: a line of {h} x {w} for an input of {img_h} x {img_w}: every side must be at least 1')
    if not 0.0 <= overlap <= 0.75:
        raise ValueError(f'line_windows: overlap must be in [0, 0.75], got {overlap!r}')
    if not 0.25 <= aspect <= 4.0:
        raise ValueError(f'line_windows: aspect must be in [0.25, 4], got {aspect!r}')
    ww = max(1, math.floor(h * img_w / img_h * aspect + 0.5))
    if w <= ww:
        return [(0, w)]
    ov = math.floor(ww * overlap + 0.5)
    s = max(1, ww - ov)
    K = -(-(w - ww) // s) + 1
    if K > LINE_MAX_WINDOWS:
        raise ValueError(f'line_windows: a line of {h} x {w} gives {K} windows of {ww} columns, the limit is {LINE_MAX_WINDOWS}; raise `aspect` or cut the line')
    return [(min(k * s, w - ww), ww) for k in range(K)]


def line_plan(sizes, img_size=(32, 128), overlap: float = 0.25, aspect: float = 1.0):
    """The window table of the lines of `sizes` = [(h, w)]: (win, line_first) as lists — win[row] = (x0, ww, h) for every window of every
    line in order, line_first[l] the first row of line l, with one entry more for the end."""
    win, first = [], [0]
    for h, w in sizes:
        win += [(x0, ww, int(h)) for x0, ww in line_windows(h, w, img_size, overlap, aspect)]
        first.append(len(win))
    return win, first


def line_views(images: Sequence[Tensor], win, line_first):
    """The windows of `line_plan` as views of the uploaded lines: image l's columns x0 .. x0 + ww - 1 per row of `win`.  No copy."""
    return [images[l][:, x0:x0 + ww] for l in range(len(images)) for x0, ww, _ in win[line_first[l]:line_first[l + 1]]]
