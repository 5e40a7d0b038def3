"""The RandAugment operators of the reference's training transform (strhub/data/augment.py, aa_overrides.py) on the device, and
fused into the bicubic resize.

Fixtures: Pillow's own outputs for every operator on seeded inputs (tools/make_augment_golden.py -> tests/golden/augment_pillow.npz).
Everything is compared with `np.array_equal` on uint8: there is no tolerance anywhere.
CPU: tests/augment_reference.py == Pillow (stored outputs; live Pillow when importable, with the degenerate and the long images);
     the host halves of parseq_amd.augment == the reference's; the policy; the library's refusals (host code).
GPU: parseq_op_augment and parseq_augment_resize_bicubic through the C ABI == the same outputs.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from augment_reference import (BATCH, BICUBIC, BILINEAR, CHAINS, GEOMETRIC, SIZES, apply_chain, apply_op, case_key, make_input, rotate_matrix,
                               single_cases, table)
from augment_reference import affine_coeffs as reference_coeffs
from oracle.resize_oracle import resize_bicubic_u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'augment_pillow.npz'))
CASES = single_cases()


def _pillow_op():
    """tools/make_augment_golden.py's pillow_op: the Pillow call of every operator."""
    import importlib.util
    spec = importlib.util.spec_from_file_location('make_augment_golden', os.path.join(ROOT, 'tools', 'make_augment_golden.py'))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod.pillow_op


def test_cases_cover_every_operator_and_extreme():
    assert {name for name, _ in CASES} == set(__import__('augment_reference').OPS) and len(GOLD.files) == 1 + len(SIZES) * len(CASES)
    for want in (('Posterize', (0,)), ('Posterize', (8,)), ('Solarize', (0,)), ('Solarize', (256,)), ('Color', (0.1,)), ('Contrast', (0.1,)),
                 ('Brightness', (0.1,)), ('Rotate', (-15.0, BILINEAR)), ('Rotate', (15.0, BICUBIC)), ('ShearX', (-0.45, BICUBIC))):
        assert want in CASES, want


@pytest.mark.parametrize('h,w', SIZES)
def test_reference_matches_pillow_fixtures(h, w):
    img = make_input(h, w)
    for name, args in CASES:
        want = GOLD[case_key(h, w, name, args)]
        got = apply_op(img, name, *args)
        assert got.shape == want.shape and np.array_equal(got, want), (name, args)


def test_reference_matches_live_pillow():
    Image = pytest.importorskip('PIL.Image')
    pillow_op = _pillow_op()
    rng = np.random.default_rng(5)
    two = np.where(rng.integers(0, 2, (12, 14, 3)) > 0, 200, 30).astype(np.uint8)            # every channel uses exactly two grey levels
    assert all(len(np.unique(two[..., c])) == 2 for c in range(3))
    images = [make_input(h, w) for h, w in SIZES] + [np.full((9, 11, 3), 77, np.uint8), two]
    for img in images:
        pil = Image.fromarray(img, 'RGB')
        for name, args in CASES:
            want = np.asarray(pillow_op(pil, name, *args))
            got = apply_op(img, name, *args)
            assert got.shape == want.shape and np.array_equal(got, want), (img.shape, name, args)


def test_long_thin_image_matches_live_pillow():
    """A 3000 x 17 crop, both ways up, sheared by 0.45 and rotated by 15 degrees, both filters."""
    Image = pytest.importorskip('PIL.Image')
    pillow_op = _pillow_op()
    wide = np.random.default_rng(3).integers(0, 256, (17, 3000, 3), dtype=np.uint8)
    for img in (wide, wide.transpose(1, 0, 2).copy()):
        for name, arg in (('ShearX', 0.45), ('Rotate', 15.0)):
            for r in (BILINEAR, BICUBIC):
                want = np.asarray(pillow_op(Image.fromarray(img, 'RGB'), name, arg, r))
                assert np.array_equal(apply_op(img, name, arg, r), want), (img.shape, name, r)


def test_host_halves_match_the_reference():
    from parseq_amd import augment
    for name, args in CASES:
        if name in augment.TABLE_OPS:
            assert np.array_equal(augment.lut_for(name, *args), table(name, *args)), (name, args)
    for f in (0.1, 0.55, 1.0, 1.45, 1.9):
        assert np.array_equal(augment.lut_for('Brightness', f), table('Brightness', f)), f
    for h, w in SIZES:
        for name, args in CASES:
            if name not in GEOMETRIC:
                continue
            want = GOLD[case_key(h, w, name, args)]
            if name == 'Rotate':
                turn, nh, nw, coef = augment.rotate_expand_map(h, w, args[0])
                assert turn is None and (nh, nw) == want.shape[:2] and (nh, nw, coef) == rotate_matrix(h, w, args[0]), (h, w, args)
            else:
                coef = augment.affine_coeffs(name, h, w, args[0])
                assert coef == tuple(float(c) for c in reference_coeffs(name, h, w, args[0])) and want.shape[:2] == (h, w), (h, w, name, args)
    assert augment.rotate_expand_map(3, 7, 90)[:3] == (1, 7, 3) and augment.rotate_expand_map(3, 7, 180)[:3] == (2, 3, 7)
    assert augment.rotate_expand_map(3, 7, 270)[:3] == (3, 7, 3) and augment.rotate_expand_map(3, 7, 360)[:3] == (0, 3, 7)
    for bad in (lambda: augment.lut_for('Posterize', 9), lambda: augment.lut_for('Solarize', 257), lambda: augment.lut_for('SolarizeAdd', -1),
                lambda: augment.lut_for('Brightness', 0.05), lambda: augment.lut_for('Color', 1.0), lambda: augment.rotate_expand_map(16385, 3, 15),
                lambda: augment.affine_coeffs('Rotate', 3, 3, 1.0)):
        with pytest.raises(ValueError):
            bad()


def test_policy():
    from parseq_amd.augment import RandAugment
    assert RandAugment.missing == ('GaussianBlur', 'PoissonNoise') and len(RandAugment.ops) == 14 and len(set(RandAugment.ops)) == 14
    sizes = [(32, 100)] * 1334                      # 1334 x 3 = 4002 draws of "apply or not"
    chains = RandAugment(seed=11).sample(sizes)
    assert chains == RandAugment(seed=11).sample(sizes) and chains != RandAugment(seed=12).sample(sizes)
    allowed = {'Rotate': {15.0, -15.0}, 'ShearX': {0.45, -0.45}, 'ShearY': {0.1, -0.1}, 'TranslateXRel': {0.05, -0.05},
               'TranslateYRel': {0.15, -0.15}, 'Posterize': {2}, 'Solarize': {128}, 'SolarizeAdd': {55}, 'Color': {1.45, 0.55},
               'Contrast': {1.45, 0.55}, 'Brightness': {1.45, 0.55}}
    applied, resamples, seen = 0, set(), set()
    for chain in chains:
        names = [op[0] for op in chain]
        assert len(chain) <= 3 and len(set(names)) == len(names) and set(names) <= set(RandAugment.ops)
        applied += len(chain)
        seen |= set(names)
        for op in chain:
            if op[0] in allowed:
                assert op[1] in allowed[op[0]], op
            else:
                assert len(op) == 1, op
            if op[0] in GEOMETRIC:
                assert len(op) == 3 and op[2] in (BILINEAR, BICUBIC), op
                resamples.add(op[2])
            elif op[0] in allowed:
                assert len(op) == 2, op
    rate = applied / (3 * len(chains))
    print('application rate', rate)
    assert abs(rate - 0.5) <= 0.03                  # sigma = sqrt(0.25 / 4002) = 0.0079: the bound is 3.8 sigma
    assert resamples == {BILINEAR, BICUBIC} and seen == set(RandAugment.ops)
    assert all(len(c) <= 1 for c in RandAugment(num_layers=1, seed=0).sample(sizes[:50]))
    assert RandAugment(magnitude=10, seed=0)._args('Posterize') == (0,) and RandAugment(magnitude=10, seed=0)._args('Solarize') == (0,)
    assert RandAugment(magnitude=10, seed=0)._args('SolarizeAdd') == (110,) and RandAugment(magnitude=10, seed=0)._args('Contrast')[0] in (0.1, 1.9)


def test_library_refuses_bad_descriptors():
    """parseq_op_augment / parseq_augment_resize_bicubic check every descriptor on the host before anything is launched."""
    from parseq_amd import _native
    lib = _native.lib()

    def desc(h=4, w=6, ops=((2, 0, 4, 6),)):
        d = (_native.AugmentDesc * 1)()
        d[0].data, d[0].height, d[0].width, d[0].row_stride, d[0].num_ops = 4096, h, w, 3 * w, len(ops)
        for slot, (op, mode, oh, ow) in zip(d[0].ops, ops[:3]):
            slot.op, slot.mode, slot.out_height, slot.out_width = op, mode, oh, ow
        return d
    ptr = C.c_void_p(4096)           # never read or written: every call below is refused
    big = 1 << 40

    def low_factor():
        d = desc(ops=((4, 0, 4, 6),))
        d[0].ops[0].arg.factor = 0.05
        return d

    def nan_coefficient():
        d = desc(ops=((6, 3, 4, 6),))
        d[0].ops[0].arg.coef[:] = [1, 0, float('nan'), 0, 1, 0]
        return d
    cases = [(desc(ops=((9, 0, 4, 6),)), b'unknown operator'), (desc(ops=((2, 0, 4, 6),) * 4), b'at most 3'), (low_factor(), b'out of range'),
             (nan_coefficient(), b'out of range'), (desc(ops=((6, 1, 4, 6),)), b'out of range'), (desc(ops=((7, 4, 4, 6),)), b'out of range'),
             (desc(h=16385, ops=()), b'16384'), (desc(ops=((6, 2, 16385, 6),)), b'16384'), (desc(ops=((2, 0, 5, 6),)), b'keeps the size'),
             (desc(ops=((7, 1, 4, 6),)), b'turn'), (desc(h=0, ops=()), b'bad descriptor')]
    for d, word in cases:
        assert lib.parseq_op_augment(d, ptr, ptr, big, None) == -1 and word in lib.parseq_last_error(), word
        assert lib.parseq_augment_resize_bicubic(d, 1, 32, 128, ptr, ptr, big, None) == -1 and word in lib.parseq_last_error(), word
        assert lib.parseq_augment_workspace_bytes(d, 1) == 0 and word in lib.parseq_last_error(), word
    good = desc(ops=((2, 0, 4, 6), (7, 1, 6, 4)))
    need = lib.parseq_augment_workspace_bytes(good, 1)
    assert need >= C.sizeof(_native.AugmentDesc) + 2 * 4 * 6 * 3
    for call in (lambda n: lib.parseq_op_augment(good, ptr, ptr, n, None), lambda n: lib.parseq_augment_resize_bicubic(good, 1, 32, 128, ptr, ptr, n, None)):
        assert call(need - 1) == -1 and b'workspace' in lib.parseq_last_error()
    assert lib.parseq_op_augment(good, ptr, None, big, None) == -1 and b'null' in lib.parseq_last_error()


def test_augment_refuses_cpu_and_bad_chains():
    from parseq_amd.augment import apply_batch, augment_resize_batch
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        apply_batch([img], [[('Invert',)]])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        augment_resize_batch([img], [[]])


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize('h,w', SIZES)
def test_operator_kernels_match_pillow(h, w):
    """parseq_op_augment (through apply_batch), one operator per chain, every case of the fixtures."""
    from parseq_amd.augment import apply_batch
    img = torch.from_numpy(make_input(h, w)).cuda()
    outs = apply_batch([img] * len(CASES), [[(name,) + args] for name, args in CASES])
    for (name, args), out in zip(CASES, outs):
        want = GOLD[case_key(h, w, name, args)]
        got = out.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (name, args, int(np.abs(got.astype(int) - want.astype(int)).max()))


@pytest.mark.gpu
@pytest.mark.parametrize('index', range(len(CHAINS)))
def test_chains_match_the_composed_reference(index):
    """Three operators (statistics, table, geometric; Rotate first, in the middle, last) at every size, and a strided view as the source."""
    from parseq_amd.augment import apply_batch
    chain = CHAINS[index]
    assert len(chain) == 3
    hosts = [make_input(h, w) for h, w in SIZES]
    big = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (64, 300, 3), dtype=np.uint8)).cuda()
    view = big[8:50, 20:260]
    assert view.stride(0) == 900
    hosts.append(view.cpu().numpy().copy())
    outs = apply_batch([torch.from_numpy(a).cuda() for a in hosts[:-1]] + [view], [chain] * len(hosts))
    for host, out in zip(hosts, outs):
        want = apply_chain(host, chain)
        got = out.cpu().numpy()
        assert got.shape == want.shape and np.array_equal(got, want), (host.shape, chain)


@pytest.mark.gpu
def test_quarter_turns_and_large_images():
    """Rotate by multiples of 90 degrees (Pillow's transposes), and an image of more than one tile (200 x 300 = 15 tiles) under every kind of
    operator: the statistics of a tiled image are the whole image's."""
    from parseq_amd.augment import apply_batch
    small, large = make_input(17, 40), np.random.default_rng(4).integers(0, 256, (200, 300, 3), dtype=np.uint8)
    chains = [[('Rotate', a, BICUBIC)] for a in (0, 90, 180, 270, 360, -90)]
    for out, chain in zip(apply_batch([torch.from_numpy(small).cuda()] * len(chains), chains), chains):
        assert np.array_equal(out.cpu().numpy(), apply_chain(small, chain)), chain
    chains = [[('AutoContrast',), ('Rotate', 90, BILINEAR), ('Equalize',)], [('Contrast', 0.55), ('Color', 1.45), ('ShearX', 0.45, BILINEAR)],
              [('Rotate', 15.0, BICUBIC), ('Solarize', 128)]]
    for out, chain in zip(apply_batch([torch.from_numpy(large).cuda()] * len(chains), chains), chains):
        assert np.array_equal(out.cpu().numpy(), apply_chain(large, chain)), chain


@pytest.mark.gpu
def test_augment_resize_ragged_batch():
    """One call over 7 images (a 1 x 1 image, an empty chain, chains of one, two and three) == the resize oracle of the composed
    reference; the same call twice gives the same bytes."""
    from parseq_amd.augment import augment_resize_batch
    assert len(BATCH) == 7 and BATCH[0][0] == (1, 1) and [] in [c for _, c in BATCH] and {len(c) for _, c in BATCH} == {0, 1, 2, 3}
    hosts = [make_input(h, w) for (h, w), _ in BATCH]
    imgs = [torch.from_numpy(a).cuda() for a in hosts]
    chains = [c for _, c in BATCH]
    for target in ((32, 128), (16, 64)):
        out = augment_resize_batch(imgs, chains, target)
        again = augment_resize_batch(imgs, chains, target)
        assert out.shape == (7, 3) + target and torch.equal(out, again)
        got = out.cpu().numpy()
        for i, (host, chain) in enumerate(zip(hosts, chains)):
            want = resize_bicubic_u8(apply_chain(host, chain), *target).transpose(2, 0, 1)
            assert np.array_equal(got[i], want), (i, host.shape, chain, target)


@pytest.mark.gpu
def test_empty_chains_are_the_plain_resize():
    from parseq_amd.augment import apply_batch, augment_resize_batch
    from parseq_amd.preprocess import resize_batch
    imgs = [torch.from_numpy(make_input(h, w)).cuda() for h, w in SIZES]
    assert torch.equal(augment_resize_batch(imgs, [[]] * len(imgs)), resize_batch(imgs, (32, 128)))
    assert torch.equal(augment_resize_batch(imgs, [[('Rotate', 360, BILINEAR)]] * len(imgs), (16, 64)), resize_batch(imgs, (16, 64)))
    for img, out in zip(imgs, apply_batch(imgs, [[]] * len(imgs))):
        assert torch.equal(img, out)
    with pytest.raises(ValueError, match='at most 3'):
        apply_batch(imgs[:1], [[('Invert',)] * 4])
    with pytest.raises(ValueError, match='chains for'):
        augment_resize_batch(imgs, [[]])
