"""What `--rotation` costs on the host and on the device (profiles/rotate_resize.md).

One batch of 512 seeded crops of about 32 x 100, decoded once (PIL images in memory), then for each rotation:
  host    the evaluation loop before the rotation moved: PIL `rotate(expand=True)` per crop, upload, `resize_batch`
  device  the loop now: upload the crops as they are, `resize_batch(..., rotation=)`
and, with the crops already in device memory, `resize_batch` alone (unrotated / rotated) and the kernel alone (HIP events around
the C entry point with the descriptors prepared).  Every figure is the median of `--passes` passes after a warm-up pass, the
variants alternating inside a pass; host clocks end in a stream synchronisation.
    python tools/rotate_resize_bench.py [--out rotate_resize.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch
from PIL import Image

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from parseq_amd import _native  # noqa: E402
from parseq_amd.preprocess import _rotated_descs, resize_batch  # noqa: E402

DEV = 'cuda'
SIZE = (32, 128)


def make_crops(n):
    rng = np.random.default_rng(512)
    return [Image.fromarray(rng.integers(0, 256, (int(rng.integers(24, 41)), int(rng.integers(70, 131)), 3), dtype=np.uint8), 'RGB') for _ in range(n)]


def upload(pil):
    return torch.from_numpy(np.asarray(pil).copy()).to(DEV)


def host_path(crops, rotation):
    return resize_batch([upload(c.rotate(rotation, expand=True) if rotation else c) for c in crops], SIZE)


def device_path(crops, rotation):
    return resize_batch([upload(c) for c in crops], SIZE, rotation=rotation)


def clock(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def kernel_ms(on_device, rotation, repeats=20):
    """The launch alone: `repeats` calls of the entry point between two events, descriptors and buffers prepared."""
    lib = _native.lib()
    n = len(on_device)
    out = torch.empty((n, 3) + SIZE, dtype=torch.uint8, device=DEV)
    if rotation is None:
        descs = (_native.ImageDesc * n)()
        for d, im in zip(descs, on_device):
            d.data, d.height, d.width, d.row_stride = im.data_ptr(), im.shape[0], im.shape[1], im.stride(0)
        ws = torch.empty(lib.parseq_resize_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        call = lib.parseq_resize_bicubic
    else:
        descs, _ = _rotated_descs(on_device, [rotation] * n)
        ws = torch.empty(lib.parseq_rotate_resize_workspace_bytes(n), dtype=torch.uint8, device=DEV)
        call = lib.parseq_rotate_resize_bicubic
    start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    stream = _native.stream_ptr(out)
    for timed in (False, True):
        start.record()
        for _ in range(repeats):
            _native.check(call(descs, n, SIZE[0], SIZE[1], _native.ptr(out), _native.ptr(ws), stream))
        end.record()
        torch.cuda.synchronize()
    return start.elapsed_time(end) / repeats


def main():
    parser = argparse.ArgumentParser()
    parser.add_argument('--crops', type=int, default=512)
    parser.add_argument('--passes', type=int, default=7)
    parser.add_argument('--out', default=None)
    args = parser.parse_args()
    assert torch.cuda.is_available(), 'needs the GPU'
    crops = make_crops(args.crops)
    on_device = [upload(c) for c in crops]
    variants = {}
    for rotation in (90, 15):
        variants[f'host rotate + upload + resize_batch, rotation {rotation}'] = lambda r=rotation: host_path(crops, r)
        variants[f'upload + resize_batch(rotation={rotation})'] = lambda r=rotation: device_path(crops, r)
    variants['upload + resize_batch, unrotated'] = lambda: device_path(crops, 0)
    for rotation in (0, 90, 15):
        variants[f'resize_batch(rotation={rotation}), crops on the device'] = lambda r=rotation: resize_batch(on_device, SIZE, rotation=r)
    times = {k: [] for k in variants}
    for p in range(args.passes + 1):
        for name, fn in variants.items():
            ms, _ = clock(fn)
            if p:
                times[name].append(ms)
    for rotation in (90, 15):          # both paths give the same bytes
        assert torch.equal(host_path(crops, rotation), device_path(crops, rotation)), rotation
    result = {'crops': args.crops, 'passes': args.passes, 'device': torch.cuda.get_device_name(0),
              'ms': {k: {'median': statistics.median(v), 'min': min(v), 'max': max(v)} for k, v in times.items()},
              'kernel_ms': {'resize_bicubic_kernel': kernel_ms(on_device, None), 'rotate_resize_bicubic_kernel, mode none': kernel_ms(on_device, 0),
                            'rotate_resize_bicubic_kernel, 90': kernel_ms(on_device, 90), 'rotate_resize_bicubic_kernel, 15': kernel_ms(on_device, 15)}}
    for k, v in result['ms'].items():
        print(f'| {k} | {v["median"]:.3f} | {v["min"]:.3f} | {v["max"]:.3f} |')
    for k, v in result['kernel_ms'].items():
        print(f'| {k} | {v * 1e3:.1f} us |')
    if args.out:
        with open(args.out, 'w') as fh:
            json.dump(result, fh, indent=1)


if __name__ == '__main__':
    main()
