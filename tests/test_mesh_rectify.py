"""Rectification of polygon text regions on the device: parseq_mesh_rectify and parseq_mesh_rectify_resize_bicubic
through parseq_amd.preprocess, against Pillow's own outputs (tests/golden/mesh_pillow.npz, tools/make_mesh_golden.py; restated and checked
on the CPU in tests/test_mesh_rectify_host.py).  Everything is compared with `np.array_equal` / `torch.equal` on uint8 or bit for bit on
floats: there is no tolerance anywhere.  Every case is tiny: the shapes are the smallest at which the kernel can still go wrong."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import mesh_reference as M
from mesh_reference import CASES, MANY, MANY_SOURCE, RESIZED, SOURCES, TARGET, make_input, many_regions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = np.load(os.path.join(ROOT, 'tests', 'golden', 'mesh_pillow.npz'))


def _sources():
    return [torch.from_numpy(make_input(h, w)).cuda() for h, w in SOURCES]


def _case_regions(cases=CASES, index_of=lambda s: s):
    """Fixture cases as (image_index, strips, (h, w)): the stored strips verbatim."""
    return [(index_of(s), M.strips_from_array(GOLD[f'{name}_strips']), size) for name, s, size, _ in cases]


def _many():
    rows, at, out = GOLD['many_strips'], 0, []
    for c, (size, _) in zip(GOLD['many_counts'].tolist(), many_regions()):
        out.append((0, M.strips_from_array(rows[at:at + c]), size))
        at += c
    return out


def _many_want():
    flat, at, out = GOLD['many_out'], 0, []
    for (h, w), _ in many_regions():
        out.append(flat[at:at + 3 * h * w].reshape(h, w, 3))
        at += 3 * h * w
    return out


# ---- 1. the fixtures, byte for byte ----------------------------------------------------------------------------------------------
def test_every_case_in_one_call_matches_pillow():
    """Twenty regions over four sources in ONE call: sources from 1 x 1, outputs from 1 x 1 to several tiles a side, 1 to 64 strips, cuts
    inside tiles and on a tile's edge, a tile of five strips, polygons inside, over each edge and outside."""
    from parseq_amd.preprocess import mesh_rectify_batch
    outs = mesh_rectify_batch(_sources(), _case_regions())
    assert len(outs) == len(CASES)
    for (name, _, size, _), out in zip(CASES, outs):
        want = GOLD[f'{name}_out']
        got = out.cpu().numpy()
        assert got.shape == want.shape == size + (3,), name
        assert np.array_equal(got, want), (name, int((got != want).sum()), int(np.abs(got.astype(int) - want.astype(int)).max()))


def test_a_view_of_a_wider_tensor_as_the_source():
    from parseq_amd.preprocess import mesh_rectify_batch
    h, w = SOURCES[3]
    wide = torch.full((h + 8, w + 27, 3), 201, dtype=torch.uint8, device='cuda')
    wide[4:4 + h, 10:10 + w] = torch.from_numpy(make_input(h, w)).cuda()
    view = wide[4:4 + h, 10:10 + w]
    assert view.stride(0) == 3 * (w + 27) > 3 * w and view.stride(1) == 3
    cases = [c for c in CASES if c[1] == 3]
    outs = mesh_rectify_batch([view], _case_regions(cases, lambda s: 0))
    for (name, *_), out in zip(cases, outs):
        assert np.array_equal(out.cpu().numpy(), GOLD[f'{name}_out']), name


def test_more_regions_than_a_workgroup_has_work_items():
    """300 regions, 301 entries in the tile table, 555 strips: the plan's scan runs twice and the bisection is deep."""
    from parseq_amd.preprocess import mesh_rectify_batch
    assert MANY + 1 > 256
    outs = mesh_rectify_batch([_sources()[MANY_SOURCE]], _many())
    for i, (out, want) in enumerate(zip(outs, _many_want())):
        assert np.array_equal(out.cpu().numpy(), want), (i, want.shape)


# ---- 2. fused with the resize -------------------------------------------------------------------------------------------------------
def test_mesh_rectify_resize_is_the_resize_of_the_rectified_and_matches_pillow():
    from parseq_amd.preprocess import mesh_rectify_batch, mesh_rectify_resize_batch, resize_batch
    src, regions = _sources(), _case_regions()
    fused = mesh_rectify_resize_batch(src, regions, TARGET)
    assert fused.shape == (len(CASES), 3) + TARGET and fused.dtype == torch.uint8
    assert torch.equal(fused, resize_batch(mesh_rectify_batch(src, regions), TARGET))
    got = fused.cpu().numpy()
    assert set(RESIZED) <= {c[0] for c in CASES}
    for i, (name, *_) in enumerate(CASES):
        if name in RESIZED:
            assert np.array_equal(got[i], GOLD[f'{name}_resized']), name
    for target in ((16, 64), (9, 31)):
        assert torch.equal(mesh_rectify_resize_batch(src, regions, target), resize_batch(mesh_rectify_batch(src, regions), target)), target
    many = _many()
    one = [src[MANY_SOURCE]]
    assert torch.equal(mesh_rectify_resize_batch(one, many, TARGET), resize_batch(mesh_rectify_batch(one, many), TARGET))


def test_polygons_and_sizes_give_what_their_strips_give():
    """The (image_index, polygon) form with `sizes`, and with polygon_size, is the strip form of the same mesh."""
    from parseq_amd.preprocess import mesh_rectify_batch, polygon_mesh, polygon_size
    src = _sources()
    polygons = [(s, polygon) for _, s, _, polygon in CASES]
    sizes = [size for _, _, size, _ in CASES]
    got = mesh_rectify_batch(src, polygons, sizes=sizes)
    want = mesh_rectify_batch(src, [(s, polygon_mesh(polygon, *size), size) for (s, polygon), size in zip(polygons, sizes)])
    stored = mesh_rectify_batch(src, _case_regions())
    for (name, *_), a, b, c in zip(CASES, got, want, stored):
        assert torch.equal(a, b) and torch.equal(a, c), name
    for out, (s, polygon) in zip(mesh_rectify_batch(src, polygons), polygons):
        assert tuple(out.shape[:2]) == polygon_size(polygon)


# ---- 3. the same bytes every run, on any stream ------------------------------------------------------------------------------------------
def test_two_runs_and_a_side_stream_give_the_same_bytes():
    from parseq_amd.preprocess import mesh_rectify_batch, mesh_rectify_resize_batch
    src, regions = _sources(), _case_regions()
    first, fused = mesh_rectify_batch(src, regions), mesh_rectify_resize_batch(src, regions, TARGET)
    for a, b in zip(first, mesh_rectify_batch(src, regions)):
        assert torch.equal(a, b)
    assert torch.equal(fused, mesh_rectify_resize_batch(src, regions, TARGET))
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        again, fused_again = mesh_rectify_batch(src, regions), mesh_rectify_resize_batch(src, regions, TARGET)
    side.synchronize()
    for a, b in zip(first, again):
        assert torch.equal(a, b)
    assert torch.equal(fused, fused_again)


# ---- 4. refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_untouched():
    from parseq_amd import _native
    from parseq_amd.preprocess import mesh_rectify_batch, mesh_rectify_resize_batch
    lib = _native.lib()
    src = _sources()[3]
    good = ((2.0, 3.0), (16.0, 1.0), (30.0, 4.0), (31.0, 15.0), (16.0, 12.0), (1.0, 14.0))
    identity = (0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0)          # one strip at x0 = 0: the source's own top-left corner
    nan = float('nan')
    for call in (mesh_rectify_batch, mesh_rectify_resize_batch):
        for regions, kw in (([(1, good)], {}), ([(-1, good)], {}), ([(0, good[2::-1] + good[:2:-1])], {}), ([(0, good[:5])], {}),
                            ([(0, good)], {'sizes': [(0, 9)]}), ([(0, [(0, 9, identity)], (5, 0))], {}), ([(0, [(0, 9, identity[:2] + (nan,) + identity[3:])], (5, 9))], {}),
                            ([(0, [(0, 4, identity), (5, 9, identity)], (5, 9))], {}), ([(0, [(i, i + 1, identity) for i in range(65)], (5, 65))], {})):
            with pytest.raises(ValueError):
                call([src], regions, **kw)
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            call([src.cpu()], [(0, good)])
        with pytest.raises(ValueError, match='uint8'):
            call([src.float()], [(0, good)])

    # the raw binding: status -1 and not one byte written
    images = (_native.ImageDesc * 1)()
    images[0].data, images[0].height, images[0].width, images[0].row_stride = src.data_ptr(), src.shape[0], src.shape[1], src.stride(0)

    def region(index=0, h=5, w=9, first=0, n=2):
        d = (_native.MeshRegionDesc * 1)()
        d[0].image, d[0].height, d[0].width, d[0].first_strip, d[0].n_strips = index, h, w, first, n
        return d

    def strips(*items):
        d = (_native.MeshStrip * len(items))()
        for s, (x0, x1, coef) in zip(d, items):
            s.x0, s.x1 = x0, x1
            s.coef[:] = coef
        return d
    shifted = (4.0,) + identity[1:]                               # the second strip starts at source column 4: together the identity
    table = strips((0, 4, identity), (4, 9, shifted))
    need = lib.parseq_mesh_rectify_workspace_bytes(region(), 1, table, 2, 1)
    assert need > 0
    crop = torch.full((5, 9, 3), 0xA5, dtype=torch.uint8, device='cuda')
    batch = torch.full((1, 3) + TARGET, 0xA5, dtype=torch.uint8, device='cuda')
    ws = torch.full((need,), 0xA5, dtype=torch.uint8, device='cuda')
    outs = (C.c_void_p * 1)(crop.data_ptr())
    stream = _native.stream_ptr(src)
    for regions, tab, bytes_, word in ((region(index=1), table, need, b'image index'), (region(h=0), table, need, b'each side'), (region(n=0), table, need, b'1 .. 64'),
                                       (region(first=1), table, need, b'outside the strips array'), (region(), strips((0, 4, identity), (5, 9, shifted)), need, b'must tile'),
                                       (region(), strips((0, 4, identity), (4, 9, (nan,) + identity[1:])), need, b'not finite'), (region(), table, need - 1, b'workspace')):
        assert lib.parseq_mesh_rectify(images, 1, regions, 1, tab, 2, outs, _native.ptr(ws), bytes_, stream) == -1 and word in lib.parseq_last_error(), word
        assert lib.parseq_mesh_rectify_resize_bicubic(images, 1, regions, 1, tab, 2, TARGET[0], TARGET[1], _native.ptr(batch), _native.ptr(ws), bytes_, stream) == -1
        assert word in lib.parseq_last_error(), word
    torch.cuda.synchronize()
    assert bool((crop == 0xA5).all()) and bool((batch == 0xA5).all()) and bool((ws == 0xA5).all())
    # and the same arguments, all valid, do write
    assert lib.parseq_mesh_rectify(images, 1, region(), 1, table, 2, outs, _native.ptr(ws), need, stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(crop, src[:5, :9])


# ---- 5. end to end -------------------------------------------------------------------------------------------------------------------
SCENE_POLYGONS = [M.arc(4, 3.0, 60.0, 8.0, 12.0, 4.5, 1.5), M.arc(3, 50.0, 93.0, 24.0, 13.0, -3.0),
                  M.arc(7, 8.0, 70.0, 22.0, 15.0, 6.0, 2.0)]


def test_scene_to_strings_end_to_end(tmp_path, monkeypatch, capsys):
    """One 40 x 96 scene, three curved polygons: the device path feeds the model the bytes the host pipeline (Pillow MESH transform per
    region, upload, resize_batch) feeds it, so logits, strings and character quads are the same bit for bit."""
    from PIL import Image
    import read as read_cli
    from gpu_util import make_model
    from parseq_amd.preprocess import mesh_rectify_resize_batch, mesh_to_source, polygon_mesh, polygon_size, resize_batch
    scene = make_input(40, 96)
    sizes = [polygon_size(p) for p in SCENE_POLYGONS]
    meshes = [polygon_mesh(p, h, w) for p, (h, w) in zip(SCENE_POLYGONS, sizes)]
    assert [len(mesh) for mesh in meshes] == [3, 2, 6]
    pil = Image.fromarray(scene, 'RGB')
    crops = []
    for p, (h, w) in zip(SCENE_POLYGONS, sizes):
        data = [(box, tuple(v for q in quad for v in q)) for box, quad in M.polygon_quads(p, h, w)]
        crops.append(torch.from_numpy(np.asarray(pil.transform((w, h), Image.MESH, data, Image.BICUBIC)).copy()).cuda())
    m = make_model('parseq-tiny', 'fp32')
    img_size = tuple(m.hparams.img_size)
    with torch.inference_mode():
        host_batch = resize_batch(crops, img_size)
        device_batch = mesh_rectify_resize_batch([torch.from_numpy(scene).cuda()], [(0, p) for p in SCENE_POLYGONS], img_size)
        assert torch.equal(device_batch, host_batch)
        want_logits = m(host_batch).clone()
        assert torch.equal(m(device_batch), want_logits)
        labels, _ = m.tokenizer.read(want_logits)
        located, chars = m.tokenizer.decode_localization(m.localize(host_batch))

    scene_file, polygon_file = tmp_path / 'scene.png', tmp_path / 'scene.txt'
    pil.save(scene_file)
    polygon_file.write_text('\n'.join(','.join(repr(float(v)) for q in p for v in q) + ',###' for p in SCENE_POLYGONS) + '\n', encoding='utf-8')
    names = [f'{scene_file}#{k}' for k in range(3)]
    assert read_cli.read_regions(m, [str(scene_file)], [str(polygon_file)], polygons=True) == [f'{n}: {label}' for n, label in zip(names, labels)]

    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    read_cli.main(['pretrained=parseq-tiny', '--images', str(scene_file), '--polygons', str(polygon_file), '--boxes'])
    printed = capsys.readouterr().out.splitlines()[1:]
    want = []
    for name, label, row, mesh, size in zip(names, located, chars, meshes, sizes):
        want.append(f'{name}: {label}')
        quads = [mesh_to_source(mesh, size, img_size, ((x0, y0), (x1, y0), (x1, y1), (x0, y1))) for _, (x0, y0, x1, y1) in row]
        want.append('    ' + ' '.join(f'{ch}[' + ','.join(f'{v:.1f}' for p in quad for v in p) + ']' for (ch, _), quad in zip(row, quads)))
    assert printed == want and located == labels
    assert sum(len(row) for row in chars) > 0          # the synthetic weights do read something: the quads were compared
