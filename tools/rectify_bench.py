"""What rectifying a detector's quadrilaterals costs on the host and on the device (profiles/rectify.md).

One seeded 1080 x 1920 scene, decoded once and (for the device path) uploaded once, with 64 and with 256 seeded quadrilaterals of
text-like size (heights 16 .. 64, aspect 2 .. 8, turned by up to 20 degrees, corners perturbed):
  host    the pipeline stage 1 replaces: PIL `transform(PERSPECTIVE, BICUBIC)` per region, upload of every crop, `resize_batch`
  device  `rectify_resize_batch` on the scene in device memory
and the library call alone (HIP events around parseq_rectify_resize_bicubic with descriptors and workspace prepared).  Every figure is
the median of `--passes` passes after a warm-up pass, the variants alternating inside a pass; host clocks end in a synchronisation.
`--kernels-only N` runs the device path N times and nothing else: the run a kernel trace is taken of.
    python tools/rectify_bench.py [--out rectify.json]
"""
import argparse
import json
import math
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parseq_amd import _native  # noqa: E402
from parseq_amd.preprocess import _native_regions, rectify_resize_batch, region_descs, resize_batch  # noqa: E402

DEV = 'cuda'
SIZE = (32, 128)
SCENE = (1080, 1920)


def make_scene():
    rng = np.random.default_rng(1080)
    h, w = SCENE
    y, x = np.mgrid[0:h, 0:w]
    base = (40 + 8 * ((x // 16 + 3 * (y // 8)) % 24))[..., None] + np.array([0, 20, 40])
    return np.clip(base + rng.integers(-12, 13, (h, w, 3)), 0, 255).astype(np.uint8)


def make_quads(n):
    rng = np.random.default_rng(n)
    quads = []
    for _ in range(n):
        hh = rng.uniform(16, 64) / 2
        hw = hh * rng.uniform(2, 8)
        cx, cy, t = rng.uniform(0, SCENE[1]), rng.uniform(0, SCENE[0]), math.radians(rng.uniform(-20, 20))
        c, s = math.cos(t), math.sin(t)
        rect = ((-hw, -hh), (hw, -hh), (hw, hh), (-hw, hh))
        quads.append(tuple((cx + c * x - s * y + rng.uniform(-0.1, 0.1) * hh, cy + s * x + c * y + rng.uniform(-0.1, 0.1) * hh) for x, y in rect))
    return quads


def host_path(pil, described):
    crops = [torch.from_numpy(np.asarray(pil.transform((w, h), Image.PERSPECTIVE, coeffs, Image.BICUBIC)).copy()).to(DEV) for _, (h, w), coeffs in described]
    return resize_batch(crops, SIZE)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def call_ms(scene, described, repeats=20):
    """The library call alone: `repeats` calls between two events, descriptors, workspace and output prepared."""
    lib = _native.lib()
    n = len(described)
    images, regions = _native_regions([scene], described)
    need = lib.parseq_rectify_workspace_bytes(regions, n, 1)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    out = torch.empty((n, 3) + SIZE, dtype=torch.uint8, device=DEV)
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = _native.stream_ptr(out)
    for _ in range(2):
        start.record()
        for _ in range(repeats):
            _native.check(lib.parseq_rectify_resize_bicubic(images, 1, regions, n, SIZE[0], SIZE[1], _native.ptr(out), _native.ptr(ws), need, stream))
        end.record()
        torch.cuda.synchronize()
    return start.elapsed_time(end) / repeats


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--regions', type=int, nargs='+', default=[64, 256])
    parser.add_argument('--passes', type=int, default=15)
    parser.add_argument('--kernels-only', type=int, default=0, metavar='N')
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    host_scene = make_scene()
    pil = Image.fromarray(host_scene, 'RGB')
    scene = torch.from_numpy(host_scene).to(DEV)
    cases = {n: region_descs([(0, q) for q in make_quads(n)], n_images=1) for n in args.regions}
    forms = {n: [(i, coeffs, size) for i, size, coeffs in described] for n, described in cases.items()}
    if args.kernels_only:
        for _ in range(args.kernels_only):
            for n in args.regions:
                rectify_resize_batch([scene], forms[n], SIZE)
        torch.cuda.synchronize()
        return
    variants = {}
    for n in args.regions:
        variants[f'host: PIL transform + upload per region + resize_batch, {n} regions'] = lambda n=n: host_path(pil, cases[n])
        variants[f'device: rectify_resize_batch, {n} regions'] = lambda n=n: rectify_resize_batch([scene], forms[n], SIZE)
    times = {k: [] for k in variants}
    for p in range(args.passes + 1):
        for name, fn in variants.items():
            ms, _ = clock(fn)
            if p:
                times[name].append(ms)
    for n in args.regions:          # both paths give the same bytes
        assert torch.equal(host_path(pil, cases[n]), rectify_resize_batch([scene], forms[n], SIZE)), n
    pixels = {n: sum(h * w for _, (h, w), _ in cases[n]) for n in args.regions}
    result = {'scene': SCENE, 'passes': args.passes, 'device': torch.cuda.get_device_name(0), 'rectified_pixels': pixels,
              'ms': {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for k, v in times.items()},
              'library_call_ms': {f'parseq_rectify_resize_bicubic, {n} regions': call_ms(scene, cases[n]) for n in args.regions}}
    for k, v in result['ms'].items():
        print(f'| {k} | {v["median"]:.3f} | {v["min"]:.3f} | {v["max"]:.3f} |')
    for k, v in result['library_call_ms'].items():
        print(f'| {k} | {v * 1e3:.1f} us |')
    print('rectified pixels', pixels)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
