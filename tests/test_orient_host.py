"""Host tests of orientation-robust reading: the numpy restatement of the choice against torch, the pure host
functions of parseq_amd/preprocess.py (the angles of a mode, the way back from a turned image, the views of a quadrilateral) and the
refusals of the flags and of `orient` that need no device."""
import argparse
import math

import numpy as np
import pytest
import torch

import orient_reference as R
import rotate_reference as RR
from parseq_amd.model import check_orient
from parseq_amd.preprocess import (orientation_angles, orientation_regions, quad_coeffs, map_to_source, region_size, rotated_size, shift_quad,
                                   unrotate_points)
from parseq_amd.search_flags import add_orientation_flags, orientation_prior, resolve_orientation


# ---- the reference itself ----------------------------------------------------------------------------------------------------------------
def _torch_rows(seed, rows=12, L=26, C=95, eos=0):
    g = torch.Generator().manual_seed(seed)
    x = 4.0 * torch.randn(rows, L, C, generator=g)
    for r in range(0, rows, 2):
        x[r, (7 * r) % L, eos] += 30.0
    p, ids = x.softmax(-1).max(-1)
    lengths = torch.tensor([(row == eos).nonzero()[0, 0].item() if (row == eos).any() else L for row in ids])
    return p, lengths


def test_sum_key_is_the_log_of_the_confidence_product():
    p, lengths = _torch_rows(3)
    k = R.keys(p.numpy(), lengths.numpy(), 3, 'sum')
    for r in range(p.shape[0]):
        n = min(int(lengths[r]) + 1, p.shape[1])
        want = math.log(float(p[r, :n].double().prod()))
        assert abs(k[r // 3, r % 3] - want) <= 1e-12 * abs(want)      # fp64 both ways: n roundings of 1.1e-16 each
    m = R.keys(p.numpy(), lengths.numpy(), 3, 'mean')
    n = np.minimum(lengths.numpy() + 1, p.shape[1]).reshape(-1, 3)
    np.testing.assert_allclose(m * n, k, rtol=1e-14)
    assert np.array_equal(R.winners(k), k.argmax(1))
    pr = [0.0, 40.0, 0.0]
    assert R.select(p.numpy(), lengths.numpy(), 3, 'sum', pr)[1].tolist() == [1] * 4
    np.testing.assert_array_equal(R.keys(p.numpy(), lengths.numpy(), 3, 'sum', pr) - k, np.array([pr] * 4))


def test_reference_ties_nan_and_all_lost():
    k = np.array([[-1.0, -1.0, -2.0], [-np.inf, -np.inf, -np.inf], [-3.0, -0.5, -0.5]])
    assert R.winners(k).tolist() == [0, 0, 1]
    p = np.full((4, 3), 0.5, dtype=np.float32)
    p[1, 0] = np.nan
    p[2, 2] = np.nan          # past n: not read
    keys, view = R.select(p, np.array([3, 3, 1, 0]), 2, 'sum')
    assert keys[0, 1] == -np.inf and view.tolist() == [0, 1]
    np.testing.assert_allclose(keys[1], [2 * math.log(0.5), math.log(0.5)], rtol=1e-15)
    assert R.top_two_gap(keys)[0] == np.inf and R.top_two_gap(np.zeros((2, 1))).tolist() == [np.inf, np.inf]


# ---- orientation_angles ----------------------------------------------------------------------------------------------------------------
def test_orientation_angles():
    sizes = [(32, 100), (100, 32), (30, 20), (31, 20), (3, 2)]
    assert orientation_angles(sizes, 'flip') == [(0, 180)] * 5
    assert orientation_angles(sizes, 'all') == [(0, 90, 180, 270)] * 5
    assert orientation_angles(sizes, 'auto') == [(0, 180), (90, 270), (0, 180), (90, 270), (0, 180)]      # h == tall * w is not tall
    assert orientation_angles([(30, 20)], 'auto', tall=1.0) == [(90, 270)] and orientation_angles([(100, 32)], 'auto', tall=4) == [(0, 180)]
    assert orientation_angles([], 'all') == []
    with pytest.raises(ValueError, match='mode'):
        orientation_angles(sizes, 'upright')
    with pytest.raises(ValueError, match='tall'):
        orientation_angles(sizes, 'auto', tall=0)


# ---- unrotate_points -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('angle', [0, 90, 180, 270, -90, 450])
def test_unrotate_points_follows_the_pixel_map(angle):
    h, w = 3, 5
    src = np.arange(h * w * 3, dtype=np.uint8).reshape(h, w, 3)
    turned = RR.rotate_u8(src, angle)
    assert turned.shape[:2] == rotated_size(angle, (h, w))
    for y in range(turned.shape[0]):
        for x in range(turned.shape[1]):
            (sx, sy), = unrotate_points(angle, (h, w), [(x + 0.5, y + 0.5)])
            assert (sx - 0.5, sy - 0.5) == (int(sx), int(sy)), 'a pixel centre goes to a pixel centre'
            assert np.array_equal(src[int(sy), int(sx)], turned[y, x])
    corners = unrotate_points(angle, (h, w), [(0, 0), (turned.shape[1], turned.shape[0])])
    assert sorted(corners) in ([(0, 0), (w, h)], [(0, h), (w, 0)])
    with pytest.raises(ValueError, match='multiple of 90'):
        unrotate_points(45, (h, w), [(0, 0)])


# ---- quadrilaterals ----------------------------------------------------------------------------------------------------------------------
def test_quad_views_shift_the_corners_and_swap_the_size():
    quad = [(10.0, 20.0), (110.0, 25.0), (108.0, 55.0), (9.0, 50.0)]
    h, w = region_size(quad)
    assert (h, w) == (30, 100)
    for k in range(4):
        q = shift_quad(quad, k)
        assert q == quad[k:] + quad[:k] and q[0] == quad[k]
        assert region_size(q) == ((h, w) if k % 2 == 0 else (w, h))
    assert shift_quad(quad, 5) == shift_quad(quad, 1)
    with pytest.raises(ValueError, match='4 points'):
        shift_quad(quad[:3], 1)
    # shift k is the crop of shift 0 turned by 90 k degrees counter clockwise: the point that unrotate_points leads back from the turned crop
    # to the upright one lies at the same place of the scene through either map (an affine quad, so both maps are exact)
    para = [(10.0, 20.0), (110.0, 30.0), (105.0, 60.0), (5.0, 50.0)]
    h, w = region_size(para)
    c0 = quad_coeffs(para, h, w)
    for k in range(4):
        qk = shift_quad(para, k)
        hk, wk = region_size(qk)
        assert (hk, wk) == rotated_size(90 * k, (h, w))
        ck = quad_coeffs(qk, hk, wk)
        for pt in [(0.0, 0.0), (1.5, 2.25), (wk, hk), (wk / 3, hk / 2)]:
            (sx, sy), = map_to_source(ck, (hk, wk), (hk, wk), [pt])
            (ux, uy), = unrotate_points(90 * k, (h, w), [pt])
            (tx, ty), = map_to_source(c0, (h, w), (h, w), [(ux, uy)])
            assert abs(sx - tx) < 1e-9 and abs(sy - ty) < 1e-9, (k, pt)


def test_orientation_regions():
    wide, tall = [(0, 0), (40, 0), (40, 10), (0, 10)], [(0, 0), (10, 0), (10, 40), (0, 40)]
    regions, shifts = orientation_regions([(0, wide), (1, tall)], 'auto')
    assert shifts == [(0, 2), (1, 3)]
    assert regions == [(0, wide), (0, shift_quad(wide, 2)), (1, shift_quad(tall, 1)), (1, shift_quad(tall, 3))]
    assert [region_size(q) for _, q in regions] == [(10, 40)] * 4      # every view of 'auto' lies on its side
    regions, shifts = orientation_regions([(0, wide)], 'all')
    assert shifts == [(0, 1, 2, 3)] and [q[0] for _, q in regions] == wide
    assert orientation_regions([(3, tall)], 'flip')[1] == [(0, 2)]


# ---- refusals ------------------------------------------------------------------------------------------------------------------------------
def _parse(argv, polygons=False):
    parser = argparse.ArgumentParser()
    add_orientation_flags(parser)
    if polygons:
        parser.add_argument('--polygons', nargs='+', default=None)
    args = parser.parse_args(argv)
    return resolve_orientation(parser, args)


def test_flag_rules(capsys):
    assert _parse([]) is None and _parse([], polygons=True) is None
    assert _parse(['--auto-rotate', 'flip']) == ('flip', 0.0)
    assert _parse(['--auto-rotate', 'all', '--upright-bias', '0.25'], polygons=True) == ('all', 0.25)
    for argv, polygons, message in ((['--upright-bias', '1'], False, '--upright-bias needs --auto-rotate'),
                                    (['--auto-rotate', 'sideways'], False, 'invalid choice'),
                                    (['--auto-rotate', 'flip', '--upright-bias', 'nan'], False, 'must be finite'),
                                    (['--auto-rotate', 'auto', '--polygons', 'a.txt'], True, '--polygons')):
        with pytest.raises(SystemExit):
            _parse(argv, polygons)
        assert message in capsys.readouterr().err
    assert orientation_prior(0.0, 4) is None and orientation_prior(0.5, 3) == [0.5, 0.0, 0.0]


def test_read_and_test_parsers_take_the_flags(capsys):
    import read as read_cli
    parser = read_cli.build_parser()
    args, _ = parser.parse_known_args(['pretrained=parseq', '--images', 'a.png', '--auto-rotate', 'flip', '--polygons', 'a.txt'])
    with pytest.raises(SystemExit):
        resolve_orientation(parser, args)
    assert 'polygon' in capsys.readouterr().err
    args, _ = parser.parse_known_args(['pretrained=parseq', '--images', 'a.png'])
    assert resolve_orientation(parser, args) is None
    assert read_cli.turned_name('a.png', 0) == 'a.png' and read_cli.turned_name('a.png#2', 270) == 'a.png#2@270' and read_cli.turned_name('a', 360) == 'a'
    assert read_cli.unturned_box((1.0, 2.0, 3.0, 5.0), 0, (10, 20)) == (1.0, 2.0, 3.0, 5.0)
    assert read_cli.unturned_box((1.0, 2.0, 3.0, 5.0), 180, (10, 20)) == (17.0, 5.0, 19.0, 8.0)
    assert read_cli.unturned_box((1.0, 2.0, 3.0, 5.0), 90, (10, 20)) == (15.0, 1.0, 18.0, 3.0)


def test_test_cli_refuses_auto_rotate_with_a_search_flag(capsys):
    import importlib.util
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location('parseq_test_cli_orient_host', os.path.join(root, 'test.py'))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    for argv, message in ((['pretrained=parseq', '--auto-rotate', 'flip', '--beam', '3'], 'not with a search flag'),
                          (['pretrained=parseq', '--upright-bias', '0.5'], '--upright-bias needs --auto-rotate')):
        with pytest.raises(SystemExit):
            cli.main(argv)
        assert message in capsys.readouterr().err


def test_check_orient():
    assert check_orient((4, 2, 3, 32, 128), 'mean', None) == (4, 2, None)
    assert check_orient((1, 8, 3, 32, 128), 'sum', torch.tensor([0.5] + [0.0] * 7)) == (1, 8, [0.5] + [0.0] * 7)
    assert check_orient((1, 2, 3, 32, 128), 'sum', [0.0, float('-inf')])[2] == [0.0, float('-inf')]
    for shape, criterion, prior, message in (((4, 3, 32, 128), 'mean', None, 'views must be'), ((4, 0, 3, 32, 128), 'mean', None, 'views per crop'),
                                             ((4, 9, 3, 32, 128), 'mean', None, 'views per crop'), ((0, 2, 3, 32, 128), 'mean', None, 'empty'),
                                             ((4, 2, 3, 32, 128), 'max', None, 'criterion'), ((4, 2, 3, 32, 128), 'mean', [0.0], 'prior'),
                                             ((4, 2, 3, 32, 128), 'mean', [0.0, float('nan')], 'prior'), ((4, 2, 3, 32, 128), 'mean', [float('inf'), 0.0], 'prior')):
        with pytest.raises(ValueError, match=message):
            check_orient(shape, criterion, prior)
