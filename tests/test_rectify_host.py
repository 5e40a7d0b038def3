"""Host tests of the rectification of quadrilateral regions: the NumPy restatement (tests/rectify_reference.py)
against Pillow — stored bytes (tests/golden/rectify_pillow.npz, tools/make_rectify_golden.py) and live Pillow —, the host geometry of
parseq_amd.preprocess (region_size, quad_coeffs, map_to_source), the library's refusals (host code: nothing is launched), and read.py's
region files.  Every image comparison is `np.array_equal` on uint8: there is no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import rectify_reference as R
from rectify_reference import CASES, MANY, MANY_SOURCE, SOURCES, make_input, many_regions, transform_perspective

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'rectify_pillow.npz'))


def _pillow(img, h, w, coeffs):
    from PIL import Image
    return np.asarray(Image.fromarray(img, 'RGB').transform((w, h), Image.PERSPECTIVE, tuple(float(c) for c in coeffs), Image.BICUBIC))


def test_cases_cover_what_the_kernel_can_get_wrong():
    assert {SOURCES[s] for _, s, _, _ in CASES} == {(1, 1), (1, 2), (2, 3), (5, 7), (37, 53)}
    assert {(1, 1), (1, 9), (9, 1), (17, 33), (40, 70)} <= {size for _, _, size, _ in CASES}
    names = {name for name, *_ in CASES}
    assert {'inside', 'over_left', 'over_right', 'over_top', 'over_bottom', 'outside', 'foreshortened', 'rotated_rectangle'} <= names
    assert sum(s == 4 for _, s, _, _ in CASES) >= 3 and MANY + 1 > 256
    by_name = {name: (SOURCES[s], size, quad) for name, s, size, quad in CASES}

    def filled(name):
        """Share of the output pixels whose source position is outside the source."""
        (sh, sw), (h, w), _ = by_name[name]
        y, x = np.mgrid[0:h, 0:w]
        sx, sy = R.apply_coeffs(GOLD[f'{name}_coef'], x + 0.5, y + 0.5)
        return 1.0 - float(((sx >= 0) & (sx < sw) & (sy >= 0) & (sy < sh)).mean())
    fills = {name: filled(name) for name in names}
    assert fills['outside'] == 1.0 and fills['inside'] == 0.0
    for name in ('over_left', 'over_right', 'over_top', 'over_bottom'):
        assert 0.1 < fills[name] < 0.9, (name, fills[name])
    dens = R.denominators(GOLD['foreshortened_coef'], *by_name['foreshortened'][1])
    assert max(dens) / min(dens) >= 3.0, dens                              # strongly foreshortened: the denominator varies by 3 x
    assert tuple(GOLD['rotated_rectangle_coef'][6:]) == (0.0, 0.0)         # the closed form
    assert R.region_size(by_name['rotated_rectangle'][2]) == (13, 26)
    # the clip is exercised at both ends somewhere
    assert any((GOLD[f'{n}_out'] == 255).any() for n in names) and any(((GOLD[f'{n}_out'] == 0).any(axis=-1) & ~(GOLD[f'{n}_out'] == 0).all(axis=-1)).any()
                                                                         for n in names)


@pytest.mark.parametrize('name,source,size,quad', CASES, ids=[c[0] for c in CASES])
def test_reference_matches_pillow(name, source, size, quad):
    """The restatement == the stored bytes == live Pillow, with the stored coefficients; the coefficients are what quad_coeffs gives today
    to the solver's accuracy."""
    img = make_input(*SOURCES[source])
    coeffs = GOLD[f'{name}_coef']
    want = GOLD[f'{name}_out']
    got = transform_perspective(img, *size, coeffs)
    assert got.shape == want.shape == size + (3,) and np.array_equal(got, want)
    assert np.array_equal(_pillow(img, *size, coeffs), want)
    np.testing.assert_allclose(R.quad_coeffs(quad, *size), coeffs, rtol=1e-9, atol=1e-12)


def test_reference_matches_pillow_on_many_small_regions():
    img = make_input(*SOURCES[MANY_SOURCE])
    coefs, flat = GOLD['many_coef'], GOLD['many_out']
    assert coefs.shape == (MANY, 8)
    at = 0
    for ((h, w), _), coeffs in zip(many_regions(), coefs):
        want = flat[at:at + 3 * h * w].reshape(h, w, 3)
        at += 3 * h * w
        assert np.array_equal(transform_perspective(img, h, w, coeffs), want) and np.array_equal(_pillow(img, h, w, coeffs), want)
    assert at == flat.size


def test_reference_matches_live_pillow_on_random_quads():
    """60 seeded quads on sources of many sizes, outputs from 1 x 1, quads hanging outside: beyond what the fixtures store."""
    rng = np.random.default_rng(61)
    total = 0
    for k in range(60):
        sh, sw = int(rng.integers(1, 70)), int(rng.integers(1, 90))
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        cx, cy, hw, hh = rng.uniform(0, sw), rng.uniform(0, sh), rng.uniform(0.5, sw), rng.uniform(0.5, sh)
        rect = ((cx - hw, cy - hh), (cx + hw, cy - hh), (cx + hw, cy + hh), (cx - hw, cy + hh))
        quad = [(x + rng.uniform(-0.35, 0.35) * hw, y + rng.uniform(-0.35, 0.35) * hh) for x, y in rect]
        h, w = (1, 1) if k % 10 == 0 else R.region_size(quad, 80)
        coeffs = R.quad_coeffs(quad, h, w)
        want = _pillow(img, h, w, coeffs)
        assert np.array_equal(transform_perspective(img, h, w, coeffs), want), (k, (sh, sw), (h, w), quad)
        total += want.size
    assert total > 50000


# ---- the host geometry of the product ---------------------------------------------------------------------------------------------
def _quads():
    return [quad for _, _, _, quad in CASES] + [quad for _, quad in many_regions()[:40]]


def test_quad_coeffs_maps_the_output_corners_onto_the_quad():
    from parseq_amd.preprocess import quad_coeffs, region_size
    for quad in _quads():
        for h, w in (region_size(quad), (32, 128), (7, 3)):
            a = quad_coeffs(quad, h, w)
            assert len(a) == 8 and all(isinstance(c, float) for c in a)
            np.testing.assert_allclose(a, R.quad_coeffs(quad, h, w), rtol=1e-9, atol=1e-12)
            scale = max(abs(v) for p in quad for v in p)
            for (X, Y), (x, y) in zip(R.corners(h, w), quad):
                gx, gy = R.apply_coeffs(a, X, Y)
                assert abs(gx - x) <= 1e-9 * scale and abs(gy - y) <= 1e-9 * scale, (quad, (h, w))


def test_parallelogram_takes_the_closed_form_exactly():
    from parseq_amd.preprocess import quad_coeffs, region_size
    quad = dict((c[0], c[3]) for c in CASES)['rotated_rectangle']
    a = quad_coeffs(quad, 13, 26)
    assert a == (24.0 / 26, -5.0 / 13, 12.5, 10.0 / 26, 12.0 / 13, 3.25, 0.0, 0.0)
    # corners that are binary fractions, sides that are powers of two: the map is exact at every corner
    quad = ((3.5, 1.25), (19.5, 5.25), (17.5, 13.25), (1.5, 9.25))
    a = quad_coeffs(quad, 8, 16)
    assert [R.apply_coeffs(a, X, Y) for X, Y in R.corners(8, 16)] == [tuple(p) for p in quad]
    for left, top, right, bottom in ((0, 0, 53, 37), (4, 2, 9, 3), (7, 5, 8, 6), (10, 0, 11, 37)):
        box = ((left, top), (right, top), (right, bottom), (left, bottom))
        h, w = region_size(box)
        assert (h, w) == (bottom - top, right - left)
        assert quad_coeffs(box, h, w) == (1.0, 0.0, float(left), 0.0, 1.0, float(top), 0.0, 0.0)
        img = make_input(37, 53)
        assert np.array_equal(transform_perspective(img, h, w, quad_coeffs(box, h, w)), img[top:bottom, left:right])


def test_quad_coeffs_refuses_what_has_no_rectification():
    from parseq_amd.preprocess import check_coeffs, quad_coeffs
    good = ((10.0, 5.0), (40.0, 6.0), (41.0, 20.0), (9.0, 19.0))
    quad_coeffs(good, 14, 30)
    bow_tie = (good[0], good[1], good[3], good[2])
    flipped = (good[1], good[0], good[3], good[2])                         # mirrored: counter clockwise
    upside = (good[3], good[2], good[1], good[0])                          # mirrored the other way
    near_horizon = ((10.0, 5.0), (40.0, 5.0), (26.0, 6.0), (24.0, 6.0))    # the far edge 15 x shorter, the horizon just beyond it: legal
    quad_coeffs(near_horizon, 14, 30)
    # BR pulled inside the triangle of the other three: not convex, i.e. the horizon (the zero line of the denominator) crosses the output
    dart = ((10.0, 5.0), (40.0, 6.0), (14.0, 8.0), (9.0, 19.0))
    for bad in (bow_tie, flipped, upside, dart, ((1.0, 1.0),) * 4, ((0.0, 0.0), (1.0, 0.0), (2.0, 0.0), (3.0, 0.0)),
                (good[0], good[1], good[2], (float('nan'), 1.0)), (good[0], good[1], (float('inf'), 3.0), good[3]), good[:3]):
        with pytest.raises(ValueError):
            quad_coeffs(bad, 14, 30)
    # ... and a vanishing line that crosses the output: the denominator 1 - X / 20 is 0 at X = 20 < 30
    for coeffs in ((1, 0, 0, 0, 1, 0, -1 / 20, 0), (1, 0, 0, 0, 1, 0, 0, -1 / 14), (1, 0, 0, 0, 1, 0, -1 / 30, 0), (1, 0, float('nan'), 0, 1, 0, 0, 0),
                   (1, 0, 0, 0, float('inf'), 0, 0, 0), (1, 0, 0, 0, 1, 0, 0)):
        with pytest.raises(ValueError):
            check_coeffs(coeffs, 14, 30)
    assert check_coeffs((1, 0, 0, 0, 1, 0, -1 / 31, 0), 14, 30)[6] == -1 / 31


def test_region_size_rounds_and_clamps():
    from parseq_amd.preprocess import region_size
    assert region_size(((0, 0), (10.4, 0), (10.4, 3.5), (0, 3.5))) == (4, 10)           # 3.5 rounds up, 10.4 down
    assert region_size(((0, 0), (10.5, 0), (10.5, 3.49), (0, 3.49))) == (3, 11)
    assert region_size(((0, 0), (3, 4), (3, 4), (0, 0))) == (1, 5)                      # hypot; a side of length 0 is clamped to 1
    assert region_size(((0, 0), (10, 0), (30, 7), (0, 2))) == (21, 30)                  # the longer of two opposite edges: hypot(20, 7), hypot(30, 5)
    assert region_size(((0, 0), (0.2, 0), (0.2, 0.3), (0, 0.3))) == (1, 1)
    assert region_size(((0, 0), (5000, 0), (5000, 20), (0, 20))) == (20, 1024)
    assert region_size(((0, 0), (5000, 0), (5000, 20), (0, 20)), max_side=64) == (20, 64)
    for quad in _quads():
        assert region_size(quad) == R.region_size(quad)
    assert all(isinstance(v, int) for v in region_size(((0, 0), (10.4, 0), (10.4, 3.5), (0, 3.5))))


def test_map_to_source_sends_the_model_input_back_to_the_quad():
    from parseq_amd.preprocess import map_to_source, quad_coeffs, region_size
    H, W = 32, 128
    for quad in _quads():
        h, w = region_size(quad)
        a = quad_coeffs(quad, h, w)
        back = map_to_source(a, (h, w), (H, W), [(0, 0), (W, 0), (W, H), (0, H)])
        scale = max(abs(v) for p in quad for v in p)
        np.testing.assert_allclose(back, quad, rtol=0, atol=1e-9 * scale)
        pts = [(17.5, 3.25), (64.0, 16.0), (127.0, 31.0)]
        np.testing.assert_allclose(map_to_source(a, (h, w), (H, W), pts), R.map_to_source(a, (h, w), (H, W), pts), rtol=1e-12, atol=0)
    # an axis-aligned box: the plain stretch of read.py's scale_box, moved to the box's corner
    assert map_to_source((1, 0, 40, 0, 1, 20, 0, 0), (64, 256), (H, W), [(8.0, 4.0), (64.0, 32.0)]) == [(56.0, 28.0), (168.0, 84.0)]


def test_region_descs_accepts_both_forms_and_names_the_region():
    from parseq_amd.preprocess import region_descs
    quad = CASES[7][3]
    descs = region_descs([(0, quad), (1, (1, 0, 3, 0, 1, 2, 0, 0), (5, 9)), (0, quad)], sizes=[None, None, (8, 40)], n_images=2)
    assert [d[1] for d in descs] == [R.region_size(quad), (5, 9), (8, 40)] and descs[1][2] == (1.0, 0.0, 3.0, 0.0, 1.0, 2.0, 0.0, 0.0)
    for bad, word in (([(2, quad)], 'image index'), ([(-1, quad)], 'image index'), ([(0, quad), (0, (quad[0], quad[1], quad[3], quad[2]))], 'region 1'),
                      ([(0, (1, 0, 0, 0, 1, 0, 0, 0), (0, 4))], 'at least 1'), ([], 'no regions'), ([(0, quad, (3, 3), 1)], 'region 0')):
        with pytest.raises(ValueError, match=word):
            region_descs(bad, n_images=2)
    with pytest.raises(ValueError, match='sizes for'):
        region_descs([(0, quad)], sizes=[(3, 3), (4, 4)], n_images=1)
    with pytest.raises(ValueError, match='at least 1'):
        region_descs([(0, quad)], sizes=[(0, 3)], n_images=1)


# ---- the library's refusals: host code, nothing is launched --------------------------------------------------------------------------
def test_library_refuses_bad_regions_before_any_device_work():
    from parseq_amd import _native
    lib = _native.lib()
    ptr = C.c_void_p(4096)           # never read or written: every call below is refused
    big = 1 << 40

    def image(h=37, w=53, stride=None):
        d = (_native.ImageDesc * 1)()
        d[0].data, d[0].height, d[0].width, d[0].row_stride = 4096, h, w, 3 * w if stride is None else stride
        return d

    def region(index=0, h=5, w=9, coef=(1, 0, 0, 0, 1, 0, 0, 0)):
        d = (_native.RegionDesc * 1)()
        d[0].image, d[0].height, d[0].width = index, h, w
        d[0].coef[:] = coef
        return d
    outs = (C.c_void_p * 1)(4096)
    cases = [(image(), region(index=1), b'image index'), (image(), region(index=-1), b'image index'), (image(), region(h=0), b'each side'),
             (image(), region(w=0), b'each side'), (image(), region(w=16385), b'16384'), (image(), region(coef=(1, 0, float('nan'), 0, 1, 0, 0, 0)), b'not finite'),
             (image(), region(coef=(1, 0, 0, 0, float('inf'), 0, 0, 0)), b'not finite'), (image(), region(coef=(1, 0, 0, 0, 1, 0, -1 / 9, 0)), b'denominator'),
             (image(), region(coef=(1, 0, 0, 0, 1, 0, 0, -1 / 4)), b'denominator'), (image(), region(coef=(1, 0, 0, 0, 1, 0, -1, -1)), b'denominator'),
             (image(h=0), region(), b'bad descriptor'), (image(stride=100), region(), b'bad descriptor'),
             (image(h=16384, w=16384, stride=1 << 17), region(), b'31 bits'), (image(h=3, w=5, stride=1 << 30), region(), b'31 bits')]
    for images, regions, word in cases:
        assert lib.parseq_rectify(images, 1, regions, 1, outs, ptr, big, None) == -1 and word in lib.parseq_last_error(), word
        assert lib.parseq_rectify_resize_bicubic(images, 1, regions, 1, 32, 128, ptr, ptr, big, None) == -1 and word in lib.parseq_last_error(), word
    assert lib.parseq_rectify_workspace_bytes(region(h=0), 1, 1) == 0 and b'each side' in lib.parseq_last_error()
    assert lib.parseq_rectify_workspace_bytes(region(), 0, 1) == 0 and lib.parseq_rectify_workspace_bytes(region(), 1, 0) == 0
    need = lib.parseq_rectify_workspace_bytes(region(), 1, 1)
    assert need >= C.sizeof(_native.RegionDesc) + C.sizeof(_native.ImageDesc) + 5 * 9 * 3 and need % 256 == 0
    # a denominator that is positive at the corners is accepted as far as the workspace check
    edge = region(coef=(1, 0, 0, 0, 1, 0, -1 / 9.5, 0))
    for images, regions in ((image(), region()), (image(), edge), (image(h=16383, w=16384, stride=1 << 17), region())):
        assert lib.parseq_rectify(images, 1, regions, 1, outs, ptr, need - 1, None) == -1 and b'workspace' in lib.parseq_last_error()
        assert lib.parseq_rectify_resize_bicubic(images, 1, regions, 1, 32, 128, ptr, ptr, need - 1, None) == -1 and b'workspace' in lib.parseq_last_error()
    assert lib.parseq_rectify(image(), 1, region(), 1, None, ptr, big, None) == -1 and b'null' in lib.parseq_last_error()
    assert lib.parseq_rectify(image(), 1, region(), 1, outs, None, big, None) == -1 and b'null' in lib.parseq_last_error()
    assert lib.parseq_rectify_resize_bicubic(image(), 1, region(), 1, 0, 128, ptr, ptr, big, None) == -1 and b'bad shape' in lib.parseq_last_error()
    assert C.sizeof(_native.RegionDesc) == 80 and _native.RegionDesc.coef.offset == 16


def test_rectify_refuses_cpu_tensors_and_bad_regions():
    import torch
    from parseq_amd.preprocess import rectify_batch, rectify_resize_batch
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    box = ((0, 0), (4, 0), (4, 4), (0, 4))
    for call in (rectify_batch, rectify_resize_batch):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call([img], [(0, box)])


# ---- read.py --regions ------------------------------------------------------------------------------------------------------------
def test_region_file_parser(tmp_path):
    pytest.importorskip('PIL.Image')
    import read as read_cli
    f = tmp_path / 'gt_img_1.txt'
    f.write_bytes('\ufeff377,117,463,117,465,130,378,130,Genaxis Theatre\r\n\n  \n10.5, 20.25, 30, 21, 31, 40.75, 9, 39\n1,2,3,4,5,6,7,8,a,b,,c\n'.encode('utf-8'))
    assert read_cli.load_regions(str(f)) == [((377.0, 117.0), (463.0, 117.0), (465.0, 130.0), (378.0, 130.0)),
                                              ((10.5, 20.25), (30.0, 21.0), (31.0, 40.75), (9.0, 39.0)),
                                              ((1.0, 2.0), (3.0, 4.0), (5.0, 6.0), (7.0, 8.0))]
    for text, line in (('1,2,3,4,5,6,7,8\n1,2,3,4,5,6,7\n', 2), ('1,2,3,4,five,6,7,8\n', 1), ('\n\n1 2 3 4 5 6 7 8\n', 3), ('1,2,3,4,5,6,7,nan\n', 1)):
        g = tmp_path / 'bad.txt'
        g.write_text(text, encoding='utf-8')
        with pytest.raises(ValueError, match=rf'bad\.txt.*line {line}\b'):
            read_cli.load_regions(str(g))
    empty = tmp_path / 'empty.txt'
    empty.write_text('\n', encoding='utf-8')
    assert read_cli.load_regions(str(empty)) == []


def test_read_cli_regions_need_one_file_per_image(monkeypatch, capsys):
    pytest.importorskip('PIL.Image')
    import read as read_cli

    def no_model(*a, **kw):
        raise AssertionError('the model must not be loaded after an argument error')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', no_model)
    with pytest.raises(SystemExit) as e:
        read_cli.main(['pretrained=parseq', '--images', 'a.png', 'b.png', '--regions', 'a.txt'])
    assert e.value.code == 2 and '--regions' in capsys.readouterr().err


def test_product_modules_import_nothing_from_the_oracle_or_the_tests():
    import re
    pat = re.compile(r'^\s*(from|import)\s+(oracle|tests|rectify_reference|augment_reference|gpu_util)\b', re.M)
    for path in (os.path.join(ROOT, 'read.py'), os.path.join(ROOT, 'parseq_amd', 'preprocess.py'), os.path.join(ROOT, 'parseq_amd', '_native.py')):
        text = open(path).read()
        assert not pat.search(text) and 'sys.path' not in text, path
