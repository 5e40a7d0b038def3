"""Host tests of the rectification of polygon regions: the NumPy restatement (tests/mesh_reference.py) against
Pillow — stored bytes (tests/golden/mesh_pillow.npz, tools/make_mesh_golden.py) and live Pillow —, the host geometry of
parseq_amd.preprocess (polygon_size, polygon_mesh, mesh_to_source, polygon_descs), the refusals in Python and in the library (host code:
nothing is launched), and read.py's polygon files.  Every image comparison is `np.array_equal` on uint8: there is no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import mesh_reference as M
from mesh_reference import CASES, MANY, MANY_SOURCE, SOURCES, make_input, many_regions, transform_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'mesh_pillow.npz'))


def _pillow(img, h, w, quads):
    from PIL import Image
    data = [(box, tuple(v for p in quad for v in p)) for box, quad in quads]
    return np.asarray(Image.fromarray(img, 'RGB').transform((w, h), Image.MESH, data, Image.BICUBIC))


def _pillow_quad_data(box, quad):
    """The eight numbers Image.__transformer hands to the C transform for QUAD: its own code, run on a stand-in that records them."""
    from PIL import Image

    class Core:
        def transform(self, box, im, method, data, resample, fill):
            self.data = tuple(data)

    class Spy:
        im = Core()

        def load(self):
            pass
    spy = Spy()
    Image.Image._Image__transformer(spy, box, Image.new('RGB', (2, 2)), Image.Transform.QUAD, tuple(v for p in quad for v in p), Image.BICUBIC, True)
    return spy.im.data


def _strips(name):
    return M.strips_from_array(GOLD[f'{name}_strips'])


def test_cases_cover_what_the_kernel_can_get_wrong():
    by_name = {name: (SOURCES[s], size, polygon) for name, s, size, polygon in CASES}
    assert {SOURCES[s] for _, s, _, _ in CASES} == {(1, 1), (2, 3), (5, 7), (37, 53)}
    assert {len(p) for _, _, _, p in CASES} >= {4, 6, 10, 14}
    counts = {name: len(_strips(name)) for name in by_name}
    assert counts['quad'] == 1 and counts['arc6'] == 2 and counts['arc10'] == 4 and counts['arc14'] == 6
    assert counts['sixty_four_strips'] == 64 == M.MAX_STRIPS and len(by_name['sixty_four_strips'][2]) == 130
    assert counts['vanishing'] == 2 and len(by_name['vanishing'][2]) == 8             # three segments, one without a column
    assert by_name['one_wide'][1] == (9, 1) and len(by_name['one_wide'][2]) == 12 and counts['one_wide'] == 1
    assert by_name['one_high'][1][0] == 1 and counts['one_high'] > 1
    h, w = by_name['several_tiles'][1]
    assert h > 32 and w > 64 and all(x1 % 16 for _, x1, _ in _strips('several_tiles')[:-1])      # several tiles a side, the cuts inside tiles
    assert sum(x1 <= 16 for _, x1, _ in _strips('three_in_a_tile')) >= 3
    assert [x1 for _, x1, _ in _strips('cut_on_a_tile_edge')] == [16, 32]
    assert MANY + 1 > 256 and len(GOLD['many_counts']) == MANY

    def filled(name):
        return float((GOLD[f'{name}_out'] == 0).all(axis=-1).mean())
    assert filled('outside') == 1.0
    for name in ('over_left', 'over_right', 'over_top', 'over_bottom'):
        assert 0.1 < filled(name) - filled('arc10') < 0.9, name


@pytest.mark.parametrize('name,source,size,polygon', CASES, ids=[c[0] for c in CASES])
def test_reference_matches_pillow(name, source, size, polygon):
    """The restatement == the stored bytes == live Pillow, with the stored strips; the strips are what polygon_mesh gives today."""
    img = make_input(*SOURCES[source])
    strips = _strips(name)
    want = GOLD[f'{name}_out']
    got = transform_mesh(img, *size, strips)
    assert got.shape == want.shape == size + (3,) and np.array_equal(got, want)
    assert np.array_equal(_pillow(img, *size, M.polygon_quads(polygon, *size)), want)
    assert M.polygon_mesh(polygon, *size) == strips


def test_reference_matches_pillow_on_many_small_regions():
    img = make_input(*SOURCES[MANY_SOURCE])
    rows, counts, flat = GOLD['many_strips'], GOLD['many_counts'], GOLD['many_out']
    at = k = 0
    for ((h, w), polygon), c in zip(many_regions(), counts):
        strips = M.strips_from_array(rows[k:k + c])
        k += c
        want = flat[at:at + 3 * h * w].reshape(h, w, 3)
        at += 3 * h * w
        assert np.array_equal(transform_mesh(img, h, w, strips), want) and np.array_equal(_pillow(img, h, w, M.polygon_quads(polygon, h, w)), want)
    assert at == flat.size and k == len(rows)


def _random_polygon(rng, sh, sw):
    n = int(rng.integers(2, 8))
    cx, cy, hw, hh = rng.uniform(0, sw), rng.uniform(0, sh), rng.uniform(0.5, sw), rng.uniform(0.5, sh)
    xs = np.sort(rng.uniform(cx - hw, cx + hw, n))
    top = [(float(x), float(cy - hh + rng.uniform(-0.3, 0.3) * hh)) for x in xs]
    bottom = [(float(x + rng.uniform(-0.2, 0.2)), float(cy + hh + rng.uniform(-0.3, 0.3) * hh)) for x in xs]
    return tuple(top) + tuple(bottom[::-1])


def test_reference_matches_live_pillow_on_random_polygons():
    """60 seeded polygons of 2 to 7 points a side on sources of many sizes, outputs from 1 x 1, polygons hanging outside, strips of no width
    dropped: beyond what the fixtures store."""
    rng = np.random.default_rng(62)
    total = 0
    for k in range(60):
        sh, sw = int(rng.integers(1, 41)), int(rng.integers(1, 61))
        img = rng.integers(0, 256, (sh, sw, 3), dtype=np.uint8)
        polygon = _random_polygon(rng, sh, sw)
        h, w = (1, 1) if k % 10 == 0 else M.polygon_size(polygon, 70)
        want = _pillow(img, h, w, M.polygon_quads(polygon, h, w))
        assert np.array_equal(transform_mesh(img, h, w, M.polygon_mesh(polygon, h, w)), want), (k, (sh, sw), (h, w), polygon)
        total += want.size
    assert total > 50000


# ---- the host geometry of the product ---------------------------------------------------------------------------------------------
def _polygons():
    return [(size, polygon) for _, _, size, polygon in CASES] + many_regions()[:40]


def test_polygon_mesh_tiles_the_output_and_derives_pillows_coefficients():
    from parseq_amd.preprocess import polygon_mesh
    for (h, w), polygon in _polygons():
        strips = polygon_mesh(polygon, h, w)
        assert strips == M.polygon_mesh(polygon, h, w)
        assert strips[0][0] == 0 and strips[-1][1] == w and all(a[1] == b[0] for a, b in zip(strips, strips[1:])) and all(x1 > x0 for x0, x1, _ in strips)
        assert all(isinstance(x0, int) and isinstance(x1, int) and len(a) == 8 and all(isinstance(c, float) for c in a) for x0, x1, a in strips)
        quads = M.polygon_quads(polygon, h, w)
        assert len(quads) == len(strips)
        for (x0, x1, a), (box, quad) in zip(strips, quads):
            assert box == (x0, 0, x1, h) and a == _pillow_quad_data(box, quad)          # bit for bit: Pillow's own expression, evaluated by Pillow


def test_polygon_size_rounds_and_clamps():
    from parseq_amd.preprocess import polygon_size, region_size
    assert polygon_size(((0, 0), (10.4, 0), (10.4, 3.5), (0, 3.5))) == (4, 10)           # 3.5 rounds up, 10.4 down
    assert polygon_size(((0, 0), (10.5, 0), (10.5, 3.49), (0, 3.49))) == (3, 11)
    assert polygon_size(((0, 0), (3, 4), (6, 0), (6, 2), (3, 6), (0, 2))) == (2, 10)     # the polyline's length, not the chord
    assert polygon_size(((0, 0), (3, 4), (6, 0), (6, 1), (3, 9), (0, 1))) == (5, 17)     # the longer side (two of hypot(3, 8)), the longest rung
    assert polygon_size(((0, 0), (0.2, 0), (0.2, 0.3), (0, 0.3))) == (1, 1)
    assert polygon_size(((0, 0), (2500, 0), (5000, 0), (5000, 20), (2500, 20), (0, 20))) == (20, 1024)
    assert polygon_size(((0, 0), (2500, 0), (5000, 0), (5000, 20), (2500, 20), (0, 20)), max_side=64) == (20, 64)
    for _, polygon in _polygons():
        assert polygon_size(polygon) == M.polygon_size(polygon)
    box = ((1.0, 2.0), (30.5, 2.0), (30.5, 11.0), (1.0, 11.0))
    assert polygon_size(box) == region_size(box)                                         # a quadrilateral is sized as section 22 sizes it
    assert all(isinstance(v, int) for v in polygon_size(box))


def test_mesh_to_source_sends_strip_corners_onto_the_polygon_and_is_continuous():
    from parseq_amd.preprocess import mesh_to_source, polygon_mesh
    H, W = 32, 128
    for (h, w), polygon in _polygons():
        strips = polygon_mesh(polygon, h, w)
        top, bottom = M.sides(polygon)
        cuts = M.polygon_cuts(polygon, w)
        scale = max(1.0, max(abs(v) for p in polygon for v in p))
        for x0, x1, _ in strips:
            i = max(k for k in range(len(cuts) - 1) if cuts[k] == x0 and cuts[k + 1] == x1)
            # just inside the strip's left edge and at its right edge from the left: NW, SW and — by continuity — NE, SE
            eps = 1e-9
            back = mesh_to_source(strips, (h, w), (H, W), [((x0 + eps) * W / w, 0), ((x0 + eps) * W / w, H), ((x1 - eps) * W / w, 0), ((x1 - eps) * W / w, H)])
            np.testing.assert_allclose(back, [top[i], bottom[i], top[i + 1], bottom[i + 1]], rtol=0, atol=1e-6 * scale)
        for a, b in zip(strips, strips[1:]):                                             # across a seam: both strips give the rung
            if cuts.count(a[1]) > 1:
                continue                                                                 # a segment of no width lies between the two
            for Y in (0.0, 0.37 * h, float(h)):
                left, right = M.apply_strip(a[2], a[1] - a[0], Y), M.apply_strip(b[2], 0.0, Y)
                np.testing.assert_allclose(left, right, rtol=0, atol=1e-9 * scale)
        pts = [(0.0, 0.0), (17.5, 3.25), (64.0, 16.0), (127.0, 31.0), (W, H), (-3.0, 5.0), (W + 2.0, 5.0)]
        assert mesh_to_source(strips, (h, w), (H, W), pts) == M.mesh_to_source(strips, (h, w), (H, W), pts)
        # the last strip owns X = w
        x0, x1, a = strips[-1]
        assert mesh_to_source(strips, (h, w), (H, W), [(W, H)]) == [M.apply_strip(a, float(w) - x0, float(h))]
    # an axis-aligned box: the plain stretch, moved to the box's corner
    box = ((40.0, 20.0), (296.0, 20.0), (296.0, 84.0), (40.0, 84.0))
    assert mesh_to_source(polygon_mesh(box, 64, 256), (64, 256), (H, W), [(8.0, 4.0), (64.0, 32.0)]) == [(56.0, 28.0), (168.0, 84.0)]


GOOD = ((5.0, 8.0), (24.0, 5.0), (45.0, 9.0), (44.0, 24.0), (24.0, 20.0), (6.0, 23.0))


def test_python_refuses_what_has_no_mesh():
    from parseq_amd.preprocess import MESH_MAX_STRIPS, check_strips, polygon_descs, polygon_mesh, polygon_size
    assert MESH_MAX_STRIPS == 64
    assert len(polygon_mesh(GOOD, 16, 40)) == 2
    nan, inf = float('nan'), float('inf')
    mirrored = GOOD[2::-1] + GOOD[:2:-1]                                                 # right to left: every strip counter clockwise
    folded = (GOOD[0], GOOD[2], GOOD[1]) + GOOD[3:]                                      # the top edge doubles back
    many = tuple((float(i), 0.0) for i in range(66)) + tuple((float(i), 5.0) for i in range(65, -1, -1))      # 65 strips at w = 130
    for bad, word in ((GOOD[:5], 'even number'), (GOOD[:3], 'even number'), (GOOD[:2], 'even number'), ((), 'even number'),
                      (GOOD[:2] + ((nan, 1.0),) + GOOD[3:], 'not finite'), (GOOD[:4] + ((3.0, inf),) + GOOD[5:], 'not finite'),
                      (((1.0, 1.0),) * 6, 'no length'), (mirrored, 'not clockwise'), (folded, 'not clockwise'), (many, 'at most 64')):
        with pytest.raises(ValueError, match=word):
            polygon_mesh(bad, 16, 130)
        if word in ('even number', 'not finite'):
            with pytest.raises(ValueError, match=word):
                polygon_size(bad)
    assert len(polygon_mesh(many[1:-1], 16, 130)) == 64
    for size in ((0, 9), (9, 0)):
        with pytest.raises(ValueError, match='at least 1'):
            polygon_mesh(GOOD, *size)
    # a segment of no width is dropped before the clockwise test: its quad may have no area
    assert len(polygon_mesh(dict((c[0], c[3]) for c in CASES)['vanishing'], 17, 33)) == 2
    one = (1.0, 0.5, 0.0, 0.0, 2.0, 0.0, 0.5, 0.0)
    assert check_strips([(0, 4, one), (4, 9, one)], 5, 9) == [(0, 4, one), (4, 9, one)]
    for bad, word in (([], '1 .. 64'), ([(i, i + 1, one) for i in range(65)], '1 .. 64'), ([(0, 4, one), (5, 9, one)], 'tile'), ([(0, 5, one), (4, 9, one)], 'tile'),
                      ([(1, 9, one)], 'tile'), ([(0, 8, one)], 'tile'), ([(0, 10, one)], 'tile'), ([(0, 4, one), (4, 4, one), (4, 9, one)], 'tile'),
                      ([(4, 9, one), (0, 4, one)], 'tile'), ([(0, 9, one[:7])], '8'), ([(0, 9, one[:3] + (nan,) + one[4:])], 'not all finite'),
                      ([(0, 9, (inf,) + one[1:])], 'not all finite')):
        with pytest.raises(ValueError, match=word):
            check_strips(bad, 5, 65 if len(bad) == 65 else 9)


def test_polygon_descs_accepts_both_forms_and_names_the_region():
    from parseq_amd.preprocess import polygon_descs, polygon_mesh
    one = (1.0, 0.5, 0.0, 0.0, 2.0, 0.0, 0.5, 0.0)
    descs = polygon_descs([(0, GOOD), (1, [(0, 4, one), (4, 9, one)], (5, 9)), (0, GOOD)], sizes=[None, None, (8, 40)], n_images=2)
    assert [d[0] for d in descs] == [0, 1, 0] and [d[1] for d in descs] == [M.polygon_size(GOOD), (5, 9), (8, 40)]
    assert descs[0][2] == polygon_mesh(GOOD, *M.polygon_size(GOOD)) and descs[1][2] == [(0, 4, one), (4, 9, one)] and descs[2][2] == polygon_mesh(GOOD, 8, 40)
    mirrored = GOOD[2::-1] + GOOD[:2:-1]
    for bad, word in (([(2, GOOD)], 'region 0: image index'), ([(-1, GOOD)], 'image index'), ([(0, GOOD), (0, mirrored)], 'region 1: .*not clockwise'),
                      ([(0, GOOD), (0, GOOD[:5])], 'region 1: .*even number'), ([(0, [(0, 4, one)], (5, 9))], 'region 0: .*tile'),
                      ([(0, [(0, 4, one)], (0, 4))], 'region 0: .*at least 1'), ([], 'no regions'), ([(0, GOOD, (3, 3), 1)], 'region 0'),
                      ([(0, [(0, 16385, one)], (5, 16385))], 'region 0: .*at most 16384')):
        with pytest.raises(ValueError, match=word):
            polygon_descs(bad, n_images=2)
    with pytest.raises(ValueError, match='sizes for'):
        polygon_descs([(0, GOOD)], sizes=[(3, 3), (4, 4)], n_images=1)
    with pytest.raises(ValueError, match='region 0: .*at least 1'):
        polygon_descs([(0, GOOD)], sizes=[(0, 3)], n_images=1)
    with pytest.raises(ValueError, match='region 0: .*at most 16384'):
        polygon_descs([(0, GOOD)], sizes=[(16385, 3)], n_images=1)


# ---- the library's refusals: host code, nothing is launched --------------------------------------------------------------------------
def test_library_refuses_bad_meshes_before_any_device_work():
    from parseq_amd import _native
    lib = _native.lib()
    ptr = C.c_void_p(4096)           # never read or written: every call below is refused
    big = 1 << 40
    one = (1.0, 0.5, 0.0, 0.0, 2.0, 0.0, 0.5, 0.0)

    def image(h=37, w=53, stride=None):
        d = (_native.ImageDesc * 1)()
        d[0].data, d[0].height, d[0].width, d[0].row_stride = 4096, h, w, 3 * w if stride is None else stride
        return d

    def region(index=0, h=5, w=9, first=0, n=2):
        d = (_native.MeshRegionDesc * 1)()
        d[0].image, d[0].height, d[0].width, d[0].first_strip, d[0].n_strips = index, h, w, first, n
        return d

    def strips(*items):
        items = items or ((0, 4, one), (4, 9, one))
        d = (_native.MeshStrip * len(items))()
        for s, (x0, x1, coef) in zip(d, items):
            s.x0, s.x1 = x0, x1
            s.coef[:] = coef
        return d
    outs = (C.c_void_p * 1)(4096)
    nan, inf = float('nan'), float('inf')
    column = [(i, i + 1, one) for i in range(65)]
    cases = [(image(), region(index=1), strips(), b'image index'), (image(), region(index=-1), strips(), b'image index'),
             (image(), region(h=0), strips(), b'each side'), (image(), region(w=0), strips(), b'each side'), (image(), region(w=16385), strips(), b'16384'),
             (image(), region(), strips((0, 4, one[:2] + (nan,) + one[3:]), (4, 9, one)), b'not finite'),
             (image(), region(), strips((0, 4, one), (4, 9, one[:7] + (inf,))), b'not finite'),
             (image(), region(n=0), strips(), b'1 .. 64'), (image(), region(n=-1), strips(), b'1 .. 64'), (image(), region(w=65, n=65), strips(*column), b'1 .. 64'),
             (image(), region(first=1), strips(), b'outside the strips array'), (image(), region(first=-1), strips(), b'outside the strips array'),
             (image(), region(n=3), strips(), b'outside the strips array'), (image(), region(first=1 << 30), strips(), b'outside the strips array'),
             (image(), region(), strips((0, 4, one), (5, 9, one)), b'must tile'), (image(), region(), strips((0, 5, one), (4, 9, one)), b'must tile'),
             (image(), region(), strips((1, 4, one), (4, 9, one)), b'must tile'), (image(), region(), strips((0, 4, one), (4, 8, one)), b'must tile'),
             (image(), region(), strips((0, 4, one), (4, 10, one)), b'must tile'), (image(), region(), strips((4, 9, one), (0, 4, one)), b'must tile'),
             (image(), region(n=3), strips((0, 4, one), (4, 4, one), (4, 9, one)), b'must tile'),
             (image(h=0), region(), strips(), b'bad descriptor'), (image(stride=100), region(), strips(), b'bad descriptor'),
             (image(h=16384, w=16384, stride=1 << 17), region(), strips(), b'31 bits'), (image(h=3, w=5, stride=1 << 30), region(), strips(), b'31 bits')]
    for images, regions, table, word in cases:
        assert lib.parseq_mesh_rectify(images, 1, regions, 1, table, len(table), outs, ptr, big, None) == -1 and word in lib.parseq_last_error(), word
        assert lib.parseq_mesh_rectify_resize_bicubic(images, 1, regions, 1, table, len(table), 32, 128, ptr, ptr, big, None) == -1, word
        assert word in lib.parseq_last_error(), word
    assert lib.parseq_mesh_rectify_workspace_bytes(region(h=0), 1, strips(), 2, 1) == 0 and b'each side' in lib.parseq_last_error()
    for n_regions, n_strips, n_images in ((0, 2, 1), (1, 0, 1), (1, 2, 0)):
        assert lib.parseq_mesh_rectify_workspace_bytes(region(), n_regions, strips(), n_strips, n_images) == 0
    assert lib.parseq_mesh_rectify_workspace_bytes(None, 1, strips(), 2, 1) == 0 and lib.parseq_mesh_rectify_workspace_bytes(region(), 1, None, 2, 1) == 0
    need = lib.parseq_mesh_rectify_workspace_bytes(region(), 1, strips(), 2, 1)
    assert need >= C.sizeof(_native.MeshRegionDesc) + 2 * C.sizeof(_native.MeshStrip) + C.sizeof(_native.ImageDesc) + 5 * 9 * 3 and need % 256 == 0
    # a full region of 64 strips and a table longer than the region's run are accepted as far as the workspace check
    for regions, table in ((region(), strips()), (region(w=64, n=64), strips(*column[:64])), (region(first=1), strips((0, 9, one), (0, 4, one), (4, 9, one)))):
        assert lib.parseq_mesh_rectify(image(), 1, regions, 1, table, len(table), outs, ptr, 255, None) == -1 and b'workspace' in lib.parseq_last_error()
        assert lib.parseq_mesh_rectify_resize_bicubic(image(), 1, regions, 1, table, len(table), 32, 128, ptr, ptr, 255, None) == -1
        assert b'workspace' in lib.parseq_last_error()
    assert lib.parseq_mesh_rectify(image(), 1, region(), 1, strips(), 2, outs, ptr, need - 1, None) == -1 and b'workspace' in lib.parseq_last_error()
    assert lib.parseq_mesh_rectify(image(), 1, region(), 1, strips(), 2, None, ptr, big, None) == -1 and b'null' in lib.parseq_last_error()
    assert lib.parseq_mesh_rectify(image(), 1, region(), 1, strips(), 2, outs, None, big, None) == -1 and b'null' in lib.parseq_last_error()
    assert lib.parseq_mesh_rectify(image(), 1, region(), 1, None, 2, outs, ptr, big, None) == -1 and b'null' in lib.parseq_last_error()
    assert lib.parseq_mesh_rectify(None, 1, region(), 1, strips(), 2, outs, ptr, big, None) == -1 and b'null' in lib.parseq_last_error()
    assert lib.parseq_mesh_rectify_resize_bicubic(image(), 1, region(), 1, strips(), 2, 0, 128, ptr, ptr, big, None) == -1 and b'bad shape' in lib.parseq_last_error()
    assert lib.parseq_mesh_rectify_resize_bicubic(image(), 1, region(), 1, strips(), 2, 32, 128, None, ptr, big, None) == -1 and b'null' in lib.parseq_last_error()
    assert C.sizeof(_native.MeshStrip) == 72 and _native.MeshStrip.coef.offset == 8 and C.sizeof(_native.MeshRegionDesc) == 20
    assert C.sizeof(_native.RegionDesc) == 80          # parseq_region_desc keeps its layout


def test_mesh_rectify_refuses_cpu_tensors():
    import torch
    from parseq_amd.preprocess import mesh_rectify_batch, mesh_rectify_resize_batch
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    box = ((0, 0), (4, 0), (4, 4), (0, 4))
    for call in (mesh_rectify_batch, mesh_rectify_resize_batch):
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call([img], [(0, box)])


# ---- read.py --polygons -----------------------------------------------------------------------------------------------------------
def test_polygon_file_parser(tmp_path):
    pytest.importorskip('PIL.Image')
    import read as read_cli
    f = tmp_path / 'poly_gt_img1.txt'
    f.write_bytes(('\ufeff377,117,420,110,463,117,465,130,421,124,378,130,Genaxis Theatre\r\n\n  \n'      # six points and a text with a blank
                   '10.5, 20.25, 30, 21, 31, 40.75, 9, 39\n'                                                 # four points, blanks, no text
                   '1,2,3,4,5,6,7,8,1984\n'                                                                  # a numeric transcription: the ninth number
                   '1,2,3,4,5,6,7,8,9,10,11,12,a,b,,c\n'                                                     # six points, a text with commas
                   '1,2,3,4,5,6,7,8,nan\n1,2,3,4,5,6,7,8,,9,9\n').encode('utf-8'))                           # what is not finite / empty ends the run
    quad = ((1.0, 2.0), (3.0, 4.0), (5.0, 6.0), (7.0, 8.0))
    assert read_cli.load_polygons(str(f)) == [((377.0, 117.0), (420.0, 110.0), (463.0, 117.0), (465.0, 130.0), (421.0, 124.0), (378.0, 130.0)),
                                               ((10.5, 20.25), (30.0, 21.0), (31.0, 40.75), (9.0, 39.0)), quad,
                                               quad + ((9.0, 10.0), (11.0, 12.0)), quad, quad]
    for text, line in (('1,2,3,4,5,6,7,8\n1,2,3,4,5,6,7\n', 2), ('1,2,3,4,five,6,7,8\n', 1), ('\n\n1 2 3 4 5 6 7 8\n', 3), ('1,2,3,4,5,6,7,nan\n', 1),
                       ('1,2,3,4,5,6,7,8,9,10,text\n', 1), ('1,2,3,4,5,6,7,8,9,10,11\n', 1), ('1,2,3,4,5,6,###\n', 1), ('###\n', 1)):
        g = tmp_path / 'bad.txt'
        g.write_text(text, encoding='utf-8')
        with pytest.raises(ValueError, match=rf'bad\.txt.*line {line}\b'):
            read_cli.load_polygons(str(g))
    empty = tmp_path / 'empty.txt'
    empty.write_text('\n', encoding='utf-8')
    assert read_cli.load_polygons(str(empty)) == []
    # --regions keeps its habit: the first eight fields, whatever follows
    assert read_cli.load_regions(str(f))[3] == quad


def test_read_cli_polygons_exclude_regions_and_need_one_file_per_image(monkeypatch, capsys):
    pytest.importorskip('PIL.Image')
    import read as read_cli

    def no_model(*a, **kw):
        raise AssertionError('the model must not be loaded after an argument error')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', no_model)
    with pytest.raises(SystemExit) as e:
        read_cli.main(['pretrained=parseq', '--images', 'a.png', '--regions', 'a.txt', '--polygons', 'a.txt'])
    err = capsys.readouterr().err
    assert e.value.code == 2 and '--polygons' in err and '--regions' in err
    with pytest.raises(SystemExit) as e:
        read_cli.main(['pretrained=parseq', '--images', 'a.png', 'b.png', '--polygons', 'a.txt'])
    assert e.value.code == 2 and '--polygons takes one file per image' in capsys.readouterr().err


def test_product_modules_import_nothing_from_the_tests():
    import re
    pat = re.compile(r'^\s*(from|import)\s+(oracle|tests|mesh_reference|rectify_reference|augment_reference|gpu_util)\b', re.M)
    for path in (os.path.join(ROOT, 'read.py'), os.path.join(ROOT, 'parseq_amd', 'preprocess.py'), os.path.join(ROOT, 'parseq_amd', '_native.py')):
        text = open(path).read()
        assert not pat.search(text) and 'sys.path' not in text, path
