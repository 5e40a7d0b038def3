"""The rotation of the reference's evaluation transform, `img.rotate(rotation, expand=True)` (strhub/data/module.py:72-73), on the
device and fused into the bicubic resize.

Fixtures: Pillow's own `Image.rotate(angle, expand=True)` outputs on seeded inputs, and `.resize(..., BICUBIC)` of them for one
ragged batch (tools/make_rotate_golden.py -> tests/golden/rotate_pillow.npz).  Everything is compared with `np.array_equal`: the
map is integer arithmetic, there is no tolerance.
CPU: tests/rotate_reference.py and parseq_amd.preprocess.rotation_map == Pillow (stored outputs; live Pillow when importable); the
     size bound; the library's refusals (host code).
GPU: parseq_op_rotate and parseq_rotate_resize_bicubic through the C ABI == the same outputs; test.py's evaluate_dataset with
     --rotation == the same call on files PIL rotated beforehand.
"""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest
import torch

from oracle.resize_oracle import resize_bicubic_u8
from rotate_reference import ANGLES, BATCH, SIZES, TARGETS, affine_map, apply_map, make_input, rotate_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'rotate_pillow.npz'))


@pytest.mark.parametrize('h,w', SIZES)
def test_reference_and_rotation_map_match_pillow_fixtures(h, w):
    from parseq_amd.preprocess import rotation_map
    img = make_input(h, w)
    for angle in ANGLES:
        want = GOLD[f'{h}x{w}_{angle}']
        assert np.array_equal(rotate_u8(img, angle), want), angle
        mode, nh, nw, ints = rotation_map(h, w, angle)
        assert (mode, nh, nw, tuple(ints)) == affine_map(h, w, angle) and (nh, nw) == want.shape[:2], angle
        assert np.array_equal(apply_map(img, mode, nh, nw, ints), want), angle


def test_reference_and_rotation_map_match_live_pillow():
    Image = pytest.importorskip('PIL.Image')
    from parseq_amd.preprocess import rotation_map
    for h, w in SIZES:
        img = make_input(h, w)
        for angle in ANGLES:
            want = np.asarray(Image.fromarray(img, 'RGB').rotate(angle, expand=True))
            assert np.array_equal(rotate_u8(img, angle), want), (h, w, angle)
            assert np.array_equal(apply_map(img, *rotation_map(h, w, angle)), want), (h, w, angle)


def test_long_thin_image_matches_live_pillow():
    """The 32-bit map at a long side: 3000 x 17 turned by 33 degrees (Pillow's own fixed point holds to 32767, ours is cut at 16384)."""
    Image = pytest.importorskip('PIL.Image')
    from parseq_amd.preprocess import rotation_map
    img = np.random.default_rng(3).integers(0, 256, (17, 3000, 3), dtype=np.uint8)
    want = np.asarray(Image.fromarray(img, 'RGB').rotate(33, expand=True))
    mode, nh, nw, ints = rotation_map(17, 3000, 33)
    assert (nh, nw) == want.shape[:2] and all(-2 ** 31 <= v < 2 ** 31 for v in ints)
    assert np.array_equal(apply_map(img, mode, nh, nw, ints), want)
    assert np.array_equal(apply_map(img.transpose(1, 0, 2).copy(), *rotation_map(3000, 17, 33)),
                          np.asarray(Image.fromarray(img.transpose(1, 0, 2).copy(), 'RGB').rotate(33, expand=True)))


def test_sides_above_the_bound_are_refused():
    from parseq_amd.preprocess import MAX_SIDE, rotation_map
    assert MAX_SIDE == 16384
    assert rotation_map(MAX_SIDE, 3, 90)[1:3] == (3, MAX_SIDE) and rotation_map(3, MAX_SIDE, 0)[0] == 0
    for h, w, angle in ((MAX_SIDE + 1, 3, 0), (3, MAX_SIDE + 1, 90), (MAX_SIDE + 1, 3, 33), (0, 3, 0)):
        with pytest.raises(ValueError, match=str(MAX_SIDE)):
            rotation_map(h, w, angle)
    with pytest.raises(ValueError, match='rotated by'):      # the source fits, its expanded canvas does not
        rotation_map(MAX_SIDE, MAX_SIDE, 45)
    assert rotation_map(MAX_SIDE, 1, 45)[0] == 4


def test_library_refuses_bad_descriptors():
    """parseq_op_rotate / parseq_rotate_resize_bicubic check the descriptor on the host before anything is launched."""
    from parseq_amd import _native
    lib = _native.lib()

    def desc(h, w, mode, nh, nw):
        d = _native.RotatedImageDesc()
        d.data, d.height, d.width, d.row_stride, d.mode, d.rot_height, d.rot_width = 4096, h, w, 3 * w, mode, nh, nw
        return d
    out = C.c_void_p(4096)           # never written: every call below is refused
    for d, word in ((desc(4, 6, 5, 4, 6), b'mode'), (desc(4, 6, 1, 4, 6), b'turns'), (desc(4, 6, 0, 6, 4), b'turns'), (desc(4, 6, 4, 0, 7), b'rotated size'),
                    (desc(4, 6, 4, 16385, 7), b'16384'), (desc(16385, 6, 0, 16385, 6), b'16384'), (desc(0, 6, 0, 0, 6), b'bad descriptor')):
        assert lib.parseq_op_rotate(d, out, None) == -1 and word in lib.parseq_last_error(), word
        assert lib.parseq_rotate_resize_bicubic(d, 1, 32, 128, out, out, None) == -1 and word in lib.parseq_last_error(), word
    assert lib.parseq_rotate_resize_workspace_bytes(3) == 3 * C.sizeof(_native.RotatedImageDesc) and lib.parseq_rotate_resize_workspace_bytes(0) == 0


def test_rotation_refuses_cpu():
    from parseq_amd.preprocess import resize_batch, rotate_batch
    for rotation in (90, 15.5, [30]):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            resize_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], (32, 128), rotation=rotation)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        rotate_batch([torch.zeros(8, 8, 3, dtype=torch.uint8)], 90)


@pytest.mark.gpu
@pytest.mark.parametrize('h,w', SIZES)
def test_rotate_kernel_matches_pillow(h, w):
    """parseq_op_rotate (through rotate_batch) for every angle of the fixtures."""
    from parseq_amd.preprocess import rotate_batch
    img = torch.from_numpy(make_input(h, w)).cuda()
    outs = rotate_batch([img] * len(ANGLES), ANGLES)
    for angle, out in zip(ANGLES, outs):
        want = GOLD[f'{h}x{w}_{angle}']
        assert tuple(out.shape) == want.shape and np.array_equal(out.cpu().numpy(), want), angle


@pytest.mark.gpu
@pytest.mark.parametrize('target', TARGETS)
def test_rotate_resize_kernel_matches_pillow_ragged_batch(target):
    """One launch over every size with a map of its own per image: two unrotated images, each exact turn, seven affine maps."""
    from parseq_amd.preprocess import resize_batch, rotation_map
    modes = [rotation_map(h, w, angle)[0] for (h, w), angle in BATCH]
    assert modes.count(0) == 2 and {1, 2, 3} <= set(modes) and modes.count(4) >= 5 and {s for s, _ in BATCH} == set(SIZES)
    imgs = [torch.from_numpy(make_input(h, w)).cuda() for (h, w), _ in BATCH]
    out = resize_batch(imgs, target, rotation=[angle for _, angle in BATCH]).cpu().numpy()
    assert out.shape == (len(BATCH), 3) + tuple(target)
    for i, ((h, w), angle) in enumerate(BATCH):
        want = GOLD[f'batch{i}_{target[0]}x{target[1]}'].transpose(2, 0, 1)
        assert np.array_equal(out[i], want), (h, w, angle, int(np.abs(out[i].astype(int) - want.astype(int)).max()))


@pytest.mark.gpu
def test_rotation_of_a_strided_view():
    """A crop cut out of a larger image (row stride 900 bytes > 3 * 240) under an affine map and under a quarter turn."""
    from parseq_amd.preprocess import resize_batch, rotate_batch
    big = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (64, 300, 3), dtype=np.uint8)).cuda()
    view = big[8:50, 20:260]
    assert view.stride(0) == 900
    host = view.cpu().numpy().copy()
    for angle in (30, 90):
        want = rotate_u8(host, angle)
        assert np.array_equal(rotate_batch([view], angle)[0].cpu().numpy(), want), angle
        for target in TARGETS:
            got = resize_batch([view], target, rotation=angle).cpu().numpy()[0].transpose(1, 2, 0)
            assert np.array_equal(got, resize_bicubic_u8(want, *target)), (angle, target)


@pytest.mark.gpu
def test_no_rotation_is_the_plain_resize():
    """rotation=0 is byte-identical to no rotation argument, and so is the unrotated mode of the rotating kernel (the other images of
    its batch turn); an oversized source is refused before any launch."""
    from parseq_amd.preprocess import resize_batch
    imgs = [torch.from_numpy(make_input(h, w)).cuda() for h, w in SIZES]
    plain = resize_batch(imgs, (32, 128))
    assert torch.equal(resize_batch(imgs, (32, 128), rotation=0), plain)
    assert torch.equal(resize_batch(imgs, (32, 128), rotation=[0.0] * len(imgs)), plain)
    mixed = resize_batch(imgs + imgs[:1], (32, 128), rotation=[0] * len(imgs) + [90])
    assert torch.equal(mixed[:-1], plain)
    assert torch.equal(resize_batch(imgs, (32, 128), rotation=360), plain)
    with pytest.raises(ValueError, match='16384'):
        resize_batch([torch.zeros(1, 16385, 3, dtype=torch.uint8, device='cuda')], (32, 128), rotation=45)
    with pytest.raises(ValueError, match='rotations for'):
        resize_batch(imgs, (32, 128), rotation=[90])


@pytest.mark.gpu
@pytest.mark.parametrize('target', [(32, 128), (16, 64)])
def test_skipped_passes_through_both_resize_kernels(target):
    """A pass whose size does not change is skipped: canvases with the target's height, its width, or both, through the plain kernel and
    through the rotating one — as its unrotated mode and as a turn whose CANVAS has the side (the last image of the batch turns)."""
    from parseq_amd.preprocess import resize_batch, rotation_map
    cases = [((32, 128), 0), ((32, 77), 0), ((50, 128), 0), ((16, 64), 0), ((16, 40), 0), ((9, 64), 0),
             ((128, 32), 90), ((77, 32), 90), ((128, 50), 270), ((32, 128), 180)]
    assert [rotation_map(h, w, a)[1:3] for (h, w), a in cases[6:]] == [(32, 128), (32, 77), (50, 128), (32, 128)]
    rng = np.random.default_rng(54)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for (h, w), _ in cases]
    canvases = [rotate_u8(img, angle) for img, (_, angle) in zip(imgs, cases)]
    want = np.stack([resize_bicubic_u8(canvas, *target).transpose(2, 0, 1) for canvas in canvases])
    skipped = {(c.shape[0] == target[0], c.shape[1] == target[1]) for c in canvases}
    assert skipped == {(True, True), (True, False), (False, True), (False, False)}
    plain = resize_batch([torch.from_numpy(c).cuda() for c in canvases], target).cpu().numpy()
    turned = resize_batch([torch.from_numpy(i).cuda() for i in imgs], target, rotation=[a for _, a in cases]).cpu().numpy()
    for i, case in enumerate(cases):
        assert np.array_equal(plain[i], want[i]), ('plain', case)
        assert np.array_equal(turned[i], want[i]), ('rotating', case)


@pytest.mark.gpu
def test_region_of_the_target_size_skips_both_passes_behind_a_rectification():
    """An integer axis-aligned 32 x 128 box rectified and resized to (32, 128): the map is the identity shifted, both resize passes are
    skipped, the result is the slice; the same box as a 4-point polygon comes out of the resize as it came out of the mesh."""
    from parseq_amd.preprocess import mesh_rectify_batch, mesh_rectify_resize_batch, rectify_resize_batch
    scene = torch.from_numpy(np.random.default_rng(55).integers(0, 256, (60, 200, 3), dtype=np.uint8)).cuda()
    left, top = 7, 5
    box = [(left, top), (left + 128, top), (left + 128, top + 32), (left, top + 32)]
    got = rectify_resize_batch([scene], [(0, box)], (32, 128))
    assert np.array_equal(got[0].cpu().numpy(), scene[top:top + 32, left:left + 128].permute(2, 0, 1).cpu().numpy())
    crop = mesh_rectify_batch([scene], [(0, box)], sizes=[(32, 128)])[0]
    got = mesh_rectify_resize_batch([scene], [(0, box)], (32, 128), sizes=[(32, 128)])
    assert tuple(crop.shape) == (32, 128, 3) and np.array_equal(got[0].cpu().numpy(), crop.permute(2, 0, 1).cpu().numpy())


@pytest.mark.gpu
@pytest.mark.parametrize('rotation', [90, 15])
def test_evaluate_dataset_rotates_on_the_device(rotation, tmp_path):
    """test.py --rotation: the same Result as the unrotated evaluation of files PIL rotated beforehand."""
    Image = pytest.importorskip('PIL.Image')
    from gpu_util import make_model
    spec = importlib.util.spec_from_file_location('parseq_test_cli', os.path.join(ROOT, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    model = make_model('parseq', 'bf16x3')
    rng = np.random.default_rng(21)
    for name in ('plain', 'turned'):
        (tmp_path / name / 'set').mkdir(parents=True)
    lines = []
    for i, (h, w) in enumerate([(32, 100), (27, 141), (48, 63), (31, 90)]):
        img = Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8), 'RGB')
        img.save(tmp_path / 'plain' / 'set' / f'{i}.png')
        img.rotate(rotation, expand=True).save(tmp_path / 'turned' / 'set' / f'{i}.png')
        lines.append(f'{i}.png {"ab12"[:i + 1]}')
    for name in ('plain', 'turned'):
        (tmp_path / name / 'set' / 'gt.txt').write_text('\n'.join(lines) + '\n', encoding='utf-8')
    got = cli.evaluate_dataset(model, str(tmp_path / 'plain'), 'set', batch_size=3, rotation=rotation)
    want = cli.evaluate_dataset(model, str(tmp_path / 'turned'), 'set', batch_size=3, rotation=0)
    print(rotation, got, want)
    assert got.num_samples == 4 and got == want
