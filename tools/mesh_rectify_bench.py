"""What rectifying a curved-text detector's polygons costs on the host and on the device (profiles/mesh_rectify.md).

The seeded 1080 x 1920 scene of tools/rectify_bench.py, decoded once and (for the device path) uploaded once, with 64 and with 256 seeded
14-point polygons of text-like size (heights 16 .. 64, aspect 2 .. 8, turned by up to 20 degrees, bowed by up to half their height,
points perturbed):
  host       the pipeline the device path replaces: PIL `transform(MESH, BICUBIC)` per region, upload of every crop, `resize_batch`
  device     `mesh_rectify_resize_batch` on the scene in device memory
  yardstick  `rectify_resize_batch` (section 22, unchanged) on the quadrilaterals through the polygons' four end points, at the polygons'
             sizes: the same rectified pixels through the perspective map, so the difference is the strip lookup and the other map
and the two library calls alone (HIP events around parseq_mesh_rectify_resize_bicubic and parseq_rectify_resize_bicubic with descriptors
and workspace prepared).  Every figure is the median of `--passes` passes after a warm-up pass, the variants alternating inside a pass;
host clocks end in a synchronisation.  `--kernels-only N` runs the two device paths N times and nothing else: the run a kernel trace is
taken of.
    python tools/mesh_rectify_bench.py [--out mesh_rectify.json]
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from parseq_amd import _native  # noqa: E402
from parseq_amd.preprocess import (_native_mesh, _native_regions, mesh_rectify_resize_batch, polygon_descs, rectify_resize_batch, region_descs,  # noqa: E402
                                   resize_batch)
from rectify_bench import DEV, SCENE, SIZE, clock, make_scene  # noqa: E402

POINTS = 7          # a side: 14-point polygons


def make_polygons(n):
    rng = np.random.default_rng(1400 + n)
    polygons = []
    for _ in range(n):
        hh = rng.uniform(16, 64) / 2
        hw = hh * rng.uniform(2, 8)
        cx, cy, t = rng.uniform(0, SCENE[1]), rng.uniform(0, SCENE[0]), math.radians(rng.uniform(-20, 20))
        bow = rng.uniform(-1.0, 1.0) * hh
        c, s = math.cos(t), math.sin(t)
        us = [-1.0 + 2.0 * i / (POINTS - 1) for i in range(POINTS)]
        local = [(u * hw, -hh - bow * (1.0 - u * u)) for u in us] + [(u * hw, hh - bow * (1.0 - u * u)) for u in reversed(us)]
        polygons.append(tuple((cx + c * x - s * y + rng.uniform(-0.05, 0.05) * hh, cy + s * x + c * y + rng.uniform(-0.05, 0.05) * hh) for x, y in local))
    return polygons


def host_path(pil, polygons, described):
    crops = []
    for polygon, (_, (h, w), strips) in zip(polygons, described):
        top, bottom = polygon[:POINTS], polygon[POINTS:][::-1]
        seg = 0
        data = []
        for x0, x1, _ in strips:          # every segment has a strip here: the polygons are far wider than they have segments
            data.append(((x0, 0, x1, h), top[seg] + bottom[seg] + bottom[seg + 1] + top[seg + 1]))
            seg += 1
        crops.append(torch.from_numpy(np.asarray(pil.transform((w, h), Image.MESH, data, Image.BICUBIC)).copy()).to(DEV))
    return resize_batch(crops, SIZE)


def call_ms(call, repeats=20):
    """A library call alone: `repeats` calls between two events."""
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    for _ in range(2):
        start.record()
        for _ in range(repeats):
            _native.check(call())
        end.record()
        torch.cuda.synchronize()
    return start.elapsed_time(end) / repeats


def library_calls(scene, mesh, quads):
    """(mesh call, perspective call) as closures over prepared descriptors, workspaces and outputs (kept alive by the closures)."""
    lib = _native.lib()
    n = len(mesh)
    out = torch.empty((n, 3) + SIZE, dtype=torch.uint8, device=DEV)
    stream = _native.stream_ptr(out)
    images, regions, strips = _native_mesh([scene], mesh)
    need = lib.parseq_mesh_rectify_workspace_bytes(regions, n, strips, len(strips), 1)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    q_images, q_regions = _native_regions([scene], quads)
    q_need = lib.parseq_rectify_workspace_bytes(q_regions, n, 1)
    q_ws = torch.empty(q_need, dtype=torch.uint8, device=DEV)
    return (lambda: lib.parseq_mesh_rectify_resize_bicubic(images, 1, regions, n, strips, len(strips), SIZE[0], SIZE[1], _native.ptr(out), _native.ptr(ws), need, stream),
            lambda: lib.parseq_rectify_resize_bicubic(q_images, 1, q_regions, n, SIZE[0], SIZE[1], _native.ptr(out), _native.ptr(q_ws), q_need, stream))


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
    polygons = {n: make_polygons(n) for n in args.regions}
    mesh = {n: polygon_descs([(0, p) for p in polygons[n]], n_images=1) for n in args.regions}
    assert all(len(strips) == POINTS - 1 for n in args.regions for _, _, strips in mesh[n])
    quads = {n: region_descs([(0, (p[0], p[POINTS - 1], p[POINTS], p[-1])) for p in polygons[n]], sizes=[size for _, size, _ in mesh[n]], n_images=1)
             for n in args.regions}
    mesh_forms = {n: [(i, strips, size) for i, size, strips in mesh[n]] for n in args.regions}
    quad_forms = {n: [(i, coeffs, size) for i, size, coeffs in quads[n]] for n in args.regions}
    if args.kernels_only:
        for _ in range(args.kernels_only):
            for n in args.regions:
                mesh_rectify_resize_batch([scene], mesh_forms[n], SIZE)
                rectify_resize_batch([scene], quad_forms[n], SIZE)
        torch.cuda.synchronize()
        return
    variants = {}
    for n in args.regions:
        variants[f'host: PIL transform(MESH) + upload per region + resize_batch, {n} regions'] = lambda n=n: host_path(pil, polygons[n], mesh[n])
        variants[f'device: mesh_rectify_resize_batch, {n} regions'] = lambda n=n: mesh_rectify_resize_batch([scene], mesh_forms[n], SIZE)
        variants[f'yardstick: rectify_resize_batch on quadrilaterals of the same sizes, {n} regions'] = lambda n=n: rectify_resize_batch([scene], quad_forms[n], SIZE)
    times = {k: [] for k in variants}
    for p in range(args.passes + 1):
        for name, fn in variants.items():
            ms, _ = clock(fn)
            if p:
                times[name].append(ms)
    for n in args.regions:          # both paths give the same bytes
        assert torch.equal(host_path(pil, polygons[n], mesh[n]), mesh_rectify_resize_batch([scene], mesh_forms[n], SIZE)), n
    pixels = {n: sum(h * w for _, (h, w), _ in mesh[n]) for n in args.regions}
    library = {}
    for n in args.regions:
        mesh_call, quad_call = library_calls(scene, mesh[n], quads[n])
        library[f'parseq_mesh_rectify_resize_bicubic, {n} regions'] = call_ms(mesh_call)
        library[f'parseq_rectify_resize_bicubic, {n} regions'] = call_ms(quad_call)
    sizes = {n: [min(size for _, size, _ in mesh[n]), max(size for _, size, _ in mesh[n])] for n in args.regions}
    result = {'scene': SCENE, 'passes': args.passes, 'device': torch.cuda.get_device_name(0), 'rectified_pixels': pixels, 'sizes_min_max': sizes,
              'ms': {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for k, v in times.items()}, 'library_call_ms': library}
    for k, v in result['ms'].items():
        print(f'| {k} | {v["median"]:.3f} | {v["min"]:.3f} | {v["max"]:.3f} |')
    for k, v in library.items():
        print(f'| {k} | {v * 1e3:.1f} us |')
    print('rectified pixels', pixels, 'sizes', sizes)
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
