"""GPU tests of orientation-robust reading: the choice among K turned views of a crop.

1. `parseq_op_orient_select` against the numpy restatement (tests/orient_reference.py), which is fed by the existing `parseq_postprocess` on the
   same rows: view, logits, ids, lengths and confidence bitwise, keys to a relative 1e-12 (fp64 `log` of identical fp32 inputs: only last-place
   differences of `log` remain).  Every case asserts that the reference's top-two key gap exceeds 1e-9, so no choice hangs on those last places.
2. the winner's crop through the copy, at aligned, odd and misaligned sizes and addresses, into buffers pre-filled with 0xFF.
3. the rules: ties, priors, NaN and +inf, <eos> first, no <eos>, L = 1, K = 1.
4. `orient` of the models against `forward` on the flattened views, `parseq_postprocess` and the reference choice: bitwise.
5. `orientation_views` against `resize_batch(rotation=)`, bytes.
6. flip symmetry: crops and the same crops turned by 180 degrees read alike.
7. the command lines.
"""
import functools
import os

import numpy as np
import pytest
import torch

import orient_reference as R
from gpu_util import DEV, make_model, native
from oracle.synth import CONFIGS, synth_images
from parseq_amd.model import orient_select
from parseq_amd.preprocess import orientation_views, resize_batch

pytestmark = pytest.mark.gpu

EOS = 0
SHAPES = [(1, 1, 26, 95), (3, 2, 26, 95), (5, 4, 26, 95), (7, 3, 7, 37), (2, 4, 64, 130), (9, 8, 33, 95)]
DTYPES = {torch.uint8: 2, torch.float32: 0, torch.bfloat16: 1}


def _logits(B, K, L, C, seed):
    """4 N(0, 1), seeded, with + 30 on <eos> at a random position of every row, or (one row in four) nowhere."""
    g = torch.Generator().manual_seed(seed)
    x = 4.0 * torch.randn(B * K, L, C, generator=g)
    where = torch.randint(0, L, (B * K,), generator=g)
    skip = torch.randint(0, 4, (B * K,), generator=g) == 0
    for r in range(B * K):
        if not skip[r]:
            x[r, where[r], EOS] += 30.0
    return x


def _postprocess(logits, eos=EOS):
    """(ids, lengths, probs, conf) of the existing parseq_postprocess on device logits [R, L, C]; device tensors."""
    nat, lib = native()
    rows, L, C = logits.shape
    ids = torch.empty(rows, L, dtype=torch.int32, device=DEV)
    lengths = torch.empty(rows, dtype=torch.int32, device=DEV)
    probs = torch.empty(rows, L, dtype=torch.float32, device=DEV)
    conf = torch.empty(rows, dtype=torch.float32, device=DEV)
    with nat.guard(logits):
        nat.check(lib.parseq_postprocess(nat.ptr(logits), rows, L, C, eos, nat.ptr(ids), nat.ptr(lengths), nat.ptr(probs), nat.ptr(conf), nat.stream_ptr(logits)))
    return ids, lengths, probs, conf


def _filled(shape, dtype, skew=0):
    """A device tensor of `shape` whose every byte is 0xFF, starting `skew` bytes past an allocation boundary."""
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    if skew:
        assert dtype == torch.uint8
    raw = torch.full((n + skew,), 255, dtype=torch.uint8, device=DEV)
    return raw[skew:].view(dtype).view(*shape)


def _run_op(logits, K, criterion='mean', prior=None, images=None, eos=EOS, skew_in=0, skew_out=0):
    """parseq_op_orient_select through the C ABI on buffers and a workspace pre-filled with 0xFF; everything back on the host."""
    nat, lib = native()
    x = logits.to(DEV).contiguous()
    rows, L, C = x.shape
    B = rows // K
    out = dict(view=_filled((B,), torch.int32), keys=_filled((B, K), torch.float64), logits=_filled((B, L, C), torch.float32),
               ids=_filled((B, L), torch.int32), lengths=_filled((B,), torch.int32), confidence=_filled((B,), torch.float32))
    img = img_out = None
    code = elems = 0
    if images is not None:
        img = _filled(tuple(images.shape), images.dtype, skew_in)
        img.copy_(images)
        img_out = out['images'] = _filled((B,) + tuple(images.shape[1:]), images.dtype, skew_out)
        code, elems = DTYPES[images.dtype], images[0].numel()
    pr = torch.tensor(prior, dtype=torch.float32, device=DEV) if prior is not None else None
    need = lib.parseq_op_orient_select_workspace_bytes(B, K, L)
    assert need > 0
    ws = _filled((need,), torch.uint8)
    with nat.guard(x):
        nat.check(lib.parseq_op_orient_select(nat.ptr(x), B, K, L, C, eos, nat.ptr(img), code, elems, nat.ORIENT_CRITERIA[criterion], nat.ptr(pr),
                                              nat.ptr(out['view']), nat.ptr(out['keys']), nat.ptr(out['logits']), nat.ptr(out['ids']),
                                              nat.ptr(out['lengths']), nat.ptr(out['confidence']), nat.ptr(img_out), nat.ptr(ws), need, nat.stream_ptr(x)))
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in out.items()}


def _bits(t):
    return t.contiguous().view(torch.uint8) if t.dtype != torch.uint8 else t


def _reference(logits, K, criterion, prior, eos=EOS):
    """The reference choice on what the existing parseq_postprocess says of the rows, and the winner's rows of everything."""
    x = logits.to(DEV).contiguous()
    ids, lengths, probs, conf = (t.cpu() for t in _postprocess(x, eos))
    keys, view = R.select(probs.numpy(), lengths.numpy(), K, criterion, prior)
    rows = torch.arange(len(view)) * K + torch.from_numpy(view)
    return dict(keys=keys, view=view, gap=R.top_two_gap(keys), logits=logits[rows], ids=ids[rows], lengths=lengths[rows], confidence=conf[rows], rows=rows)


def _assert_matches(got, want, K):
    assert got['view'].tolist() == want['view'].tolist()
    for name in ('logits', 'ids', 'lengths', 'confidence'):
        assert torch.equal(_bits(got[name]), _bits(want[name])), name
    gk, wk = got['keys'].numpy(), want['keys']
    print('keys: max relative difference', np.nanmax(np.where(np.isfinite(wk), np.abs(gk - wk) / np.maximum(np.abs(wk), 1e-300), 0.0)))
    assert np.array_equal(np.isfinite(gk), np.isfinite(wk)) and np.array_equal(gk[~np.isfinite(wk)], wk[~np.isfinite(wk)])
    np.testing.assert_allclose(gk[np.isfinite(wk)], wk[np.isfinite(wk)], rtol=1e-12, atol=0)


# -------------------------------------------------------------------------------------------------------------------
# 1. the operator against the reference
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('with_prior', [False, True])
@pytest.mark.parametrize('criterion', ['mean', 'sum'])
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_op_matches_reference(shape, criterion, with_prior):
    B, K, L, C = shape
    # the seeds were checked on the CPU (torch's soft-max for the probabilities): the smallest top-two gap of the reference over all 24 cases
    # is 0.009.  A seed that puts a near-certain <eos> at position 0 of two views of one crop gives two keys of exactly 0 and is no input for this test
    logits = _logits(B, K, L, C, seed=1009 + 7 * B + K)
    prior = [0.25 * ((3 * k) % 5) - 0.5 for k in range(K)] if with_prior else None
    want = _reference(logits, K, criterion, prior)
    print('top-two gaps', want['gap'])
    assert np.all(want['gap'] > 1e-9), 'the condition of the comparison: no choice hangs on the last places of log'
    _assert_matches(_run_op(logits, K, criterion, prior), want, K)


# -------------------------------------------------------------------------------------------------------------------
# 2. crops through the copy
# -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', [('u8', 3 * 32 * 128, 0, 0), ('u8', 105, 0, 0), ('u8', 105, 1, 3), ('u8', 3 * 32 * 128, 4, 8), ('u8', 1, 0, 0), ('f32', 3 * 8 * 10, 0, 0),
                                  ('f32', 7, 0, 0), ('bf16', 33, 0, 0)], ids=lambda c: '-'.join(map(str, c)))
def test_crops_through_the_copy(case):
    kind, elems, skew_in, skew_out = case
    B, K, L, C = 5, 4, 26, 95
    logits = _logits(B, K, L, C, seed=77)
    g = torch.Generator().manual_seed(elems)
    if kind == 'u8':
        images = torch.randint(0, 255, (B * K, elems), dtype=torch.uint8, generator=g)      # never 255: a byte left alone shows
    else:
        images = torch.randn(B * K, elems, generator=g).to(torch.float32 if kind == 'f32' else torch.bfloat16)
    want = _reference(logits, K, 'mean', None)
    assert len(set(want['view'].tolist())) > 1, 'the crops of several views must be asked for'
    got = _run_op(logits, K, 'mean', None, images=images, skew_in=skew_in, skew_out=skew_out)
    _assert_matches(got, want, K)
    assert torch.equal(_bits(got['images']), _bits(images[want['rows']]))


# -------------------------------------------------------------------------------------------------------------------
# 3. the rules
# -------------------------------------------------------------------------------------------------------------------
def test_identical_views_go_to_the_lowest_and_a_prior_flips_it():
    one = _logits(3, 1, 26, 95, seed=5)
    both = one.repeat_interleave(2, dim=0)      # rows b 2 and b 2 + 1 are byte-identical
    for criterion in ('mean', 'sum'):
        got = _run_op(both, 2, criterion)
        assert got['view'].tolist() == [0, 0, 0] and torch.equal(got['keys'][:, 0], got['keys'][:, 1])
        assert torch.equal(got['logits'], one)
        got = _run_op(both, 2, criterion, prior=[0.0, 0.5])
        assert got['view'].tolist() == [1, 1, 1]
        got = _run_op(both, 2, criterion, prior=[0.0, -0.5])
        assert got['view'].tolist() == [0, 0, 0]


@pytest.mark.parametrize('bad', [float('nan'), float('inf')])
def test_a_view_without_a_finite_softmax_loses(bad):
    x = _logits(4, 3, 26, 95, seed=9)
    x[:, :, EOS] -= 60.0                # no <eos> anywhere: every position counts
    for b in range(4):
        x[b * 3 + b % 3, 5, 17] = bad   # one view of every crop, a position inside the reading
    for criterion in ('mean', 'sum'):
        want = _reference(x, 3, criterion, None)
        got = _run_op(x, 3, criterion)
        _assert_matches(got, want, 3)
        for b in range(4):
            assert got['keys'][b, b % 3] == float('-inf') and got['view'][b] != b % 3
    # every view of crop 1 bad: view 0; its rows are copied as they are (NaN confidence, ids 0 at the bad position)
    x[3:6, 5, 17] = bad
    got, want = _run_op(x, 3), _reference(x, 3, 'mean', None)
    _assert_matches(got, want, 3)
    assert got['view'][1] == 0 and torch.all(got['keys'][1] == float('-inf'))


def test_eos_first_no_eos_one_position_one_view():
    L, C = 26, 95
    x = _logits(4, 2, L, C, seed=11)
    x[:, :, EOS] -= 60.0
    x[0, 0, EOS] += 120.0               # crop 0 view 0: <eos> at position 0, n = 1
    x[3, 0, EOS] += 120.0               # crop 1 view 1 likewise; crops 2 and 3: no <eos>, n = L
    for criterion in ('mean', 'sum'):
        want = _reference(x, 2, criterion, None)
        assert want['lengths'].tolist()[2:] == [L, L]
        got = _run_op(x, 2, criterion)
        _assert_matches(got, want, 2)
        p0 = float(torch.softmax(x[0, 0].double(), -1)[EOS])
        assert abs(float(got['keys'][0, 0]) - np.log(p0)) < 1e-6      # n = 1: one term, and the mean is the sum
    assert _run_op(x, 2, 'sum')['view'][0] == 0                       # one near-certain <eos> beats 26 uncertain characters
    one = _logits(6, 3, 1, C, seed=12)                                # L = 1
    for criterion in ('mean', 'sum'):
        _assert_matches(_run_op(one, 3, criterion), _reference(one, 3, criterion, None), 3)
    single = _logits(6, 1, L, C, seed=13)                             # K = 1: the post-processing of every row
    got = _run_op(single, 1, 'mean', prior=[-3.0])
    _assert_matches(got, _reference(single, 1, 'mean', [-3.0]), 1)
    assert got['view'].tolist() == [0] * 6 and torch.equal(got['logits'], single)


def test_op_refusals():
    nat, lib = native()
    assert lib.parseq_op_orient_select_workspace_bytes(4, 0, 26) == 0 and lib.parseq_op_orient_select_workspace_bytes(4, 9, 26) == 0
    assert lib.parseq_op_orient_select_workspace_bytes(4, 2, 65) == 0 and lib.parseq_op_orient_select_workspace_bytes(0, 2, 26) == 0
    x = _logits(2, 2, 26, 95, seed=1).to(DEV)
    with pytest.raises(ValueError, match='criterion'):
        orient_select(x, 2, EOS, criterion='max')
    with pytest.raises(ValueError, match='prior'):
        orient_select(x, 2, EOS, prior=[0.0])
    with pytest.raises(ValueError, match='prior'):
        orient_select(x, 2, EOS, prior=[0.0, float('nan')])
    with pytest.raises(ValueError, match='logits'):
        orient_select(x, 3, EOS)
    ws = torch.empty(1 << 16, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    args = lambda crit, images, images_out, nbytes: (nat.ptr(x), 2, 2, 26, 95, EOS, images, 2, 7, crit, None, nat.ptr(out), nat.ptr(out), nat.ptr(out), nat.ptr(out),
                                                     nat.ptr(out), nat.ptr(out), images_out, nat.ptr(ws), nbytes, nat.stream_ptr(x))
    assert lib.parseq_op_orient_select(*args(2, None, None, 1 << 16)) == -1 and b'criterion' in lib.parseq_last_error()
    assert lib.parseq_op_orient_select(*args(0, nat.ptr(out), None, 1 << 16)) == -1 and b'go together' in lib.parseq_last_error()
    assert lib.parseq_op_orient_select(*args(0, None, None, 16)) == -1 and b'workspace' in lib.parseq_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0      # refused before any device work


# -------------------------------------------------------------------------------------------------------------------
# 4. orient of the models against the existing path
# -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(precision):
    return make_model('parseq', precision)      # AR + one refinement iteration


def _existing_path(m, views, criterion, prior, eos):
    """forward on the flattened views, parseq_postprocess, the reference choice."""
    with torch.inference_mode():
        logits = m(views.flatten(0, 1))
    assert logits.shape[1] == m.model.max_label_length + 1
    want = _reference(logits.cpu(), views.shape[1], criterion, prior, eos)
    want['images'] = views.flatten(0, 1).cpu()[want['rows']]
    return want


def _assert_result(res, want, K):
    got = {k: getattr(res, k).cpu() for k in ('view', 'keys', 'logits', 'ids', 'lengths', 'confidence')}
    _assert_matches(got, want, K)
    assert torch.equal(_bits(res.images.cpu()), _bits(want['images']))


@pytest.mark.small_batch_route      # the library's own routes: 10 and 12 rows take the small-batch encoder, 80 rows the one-launch kernels
@pytest.mark.parametrize('shape', [(5, 2), (3, 4), (40, 2)], ids=lambda s: 'x'.join(map(str, s)))
@pytest.mark.parametrize('precision', ['bf16x3', 'bf16'])
def test_model_orient_matches_the_existing_path(precision, shape):
    B, K = shape
    m = _model(precision)
    cfg = CONFIGS['parseq']
    views = synth_images(B * K, cfg, seed=100 + B).to(DEV).view(B, K, 3, 32, 128)
    for criterion, prior in (('mean', None), ('sum', [0.125 * k for k in range(K)])):
        want = _existing_path(m, views, criterion, prior, m.eos_id)
        with torch.inference_mode():
            res = m.orient(views, criterion=criterion, prior=prior)
        _assert_result(res, want, K)
    assert m.tokenizer.decode_logits(res.logits)[0] == m.tokenizer.decode_logits(want['logits'].to(DEV))[0]


def test_model_orient_u8_views_and_one_view_is_forward():
    m = _model('bf16x3')
    g = torch.Generator().manual_seed(3)
    views = torch.randint(0, 256, (6, 2, 3, 32, 128), dtype=torch.uint8, generator=g).to(DEV)
    want = _existing_path(m, views, 'mean', None, m.eos_id)
    with torch.inference_mode():
        _assert_result(m.orient(views), want, 2)
        one = m.orient(views[:, :1])
        assert torch.equal(one.logits, m(views[:, 0])) and one.view.tolist() == [0] * 6 and torch.equal(one.images, views[:, 0])
        short = m.orient(views, max_length=6)
        assert short.logits.shape == (6, 7, 95) and short.ids.shape == (6, 7)


def test_vitstr_orient_matches_the_existing_path():
    from parseq_amd import create_model
    torch.manual_seed(0)
    m = create_model('vitstr', precision='bf16x3').eval().to(DEV)
    g = torch.Generator().manual_seed(4)
    views = torch.randn(3, 2, 3, *m.hparams.img_size, generator=g).to(DEV)
    want = _existing_path(m, views, 'mean', None, m.eos_id)
    with torch.inference_mode():
        _assert_result(m.orient(views), want, 2)


def test_model_orient_refusals():
    m = _model('bf16x3')
    nat, lib = native()
    z = torch.zeros(2, 2, 3, 32, 128, device=DEV)
    with pytest.raises(ValueError, match='views'):
        m.orient(z[:, 0])
    with pytest.raises(ValueError, match='views per crop'):
        m.orient(torch.zeros(1, 9, 3, 32, 128, device=DEV))
    with pytest.raises(ValueError, match='criterion'):
        m.orient(z, criterion='product')
    with pytest.raises(ValueError, match='prior'):
        m.orient(z, prior=[0.0, 0.0, 0.0])
    with pytest.raises(ValueError, match='prior'):
        m.orient(z, prior=[0.0, float('inf')])
    plan = m.model._plan(8)
    assert lib.parseq_forward_oriented_workspace_bytes(plan, 4096, 8, 26) == 0 and b'views' in lib.parseq_last_error()      # past any plan's max_batch
    assert lib.parseq_forward_oriented_workspace_bytes(plan, 2, 9, 26) == 0 and lib.parseq_forward_oriented_workspace_bytes(plan, 2, 0, 26) == 0
    assert lib.parseq_forward_oriented_workspace_bytes(plan, 2, 2, 27) == 0
    ws = torch.empty(1 << 20, dtype=torch.uint8, device=DEV)
    out = torch.zeros(1 << 12, dtype=torch.float64, device=DEV)
    p = nat.ptr(out)
    status = lib.parseq_forward_oriented(plan, nat.ptr(z), 0, 2, 2, 1, 1, 26, 5, None, p, p, p, p, p, p, None, nat.ptr(ws), 1 << 20, nat.stream_ptr(z))
    assert status == -1 and b'criterion' in lib.parseq_last_error()
    status = lib.parseq_forward_oriented(plan, nat.ptr(z), 0, 2, 9, 1, 1, 26, 0, None, p, p, p, p, p, p, None, nat.ptr(ws), 1 << 20, nat.stream_ptr(z))
    assert status == -1 and b'views' in lib.parseq_last_error()
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0


# -------------------------------------------------------------------------------------------------------------------
# 5. orientation_views
# -------------------------------------------------------------------------------------------------------------------
def _crops(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(DEV) for h, w in sizes]


@pytest.mark.parametrize('mode', ['flip', 'auto', 'all'])
def test_orientation_views_are_resize_batch(mode):
    crops = _crops([(31, 100), (64, 21), (7, 9), (40, 40), (33, 22), (1, 5)], seed=21)      # (64, 21) is tall; (33, 22) is exactly 1.5: not tall
    views, angles = orientation_views(crops, mode)
    K = {'flip': 2, 'auto': 2, 'all': 4}[mode]
    assert views.shape == (6, K, 3, 32, 128) and views.dtype == torch.uint8
    if mode == 'auto':
        assert angles == [(0, 180), (90, 270), (0, 180), (0, 180), (0, 180), (0, 180)]
    for k in range(K):
        assert torch.equal(views[:, k], resize_batch(crops, (32, 128), rotation=[a[k] for a in angles])), (mode, k)
    small, _ = orientation_views(crops[:2], mode, size=(16, 48))
    assert torch.equal(small[:, 1], resize_batch(crops[:2], (16, 48), rotation=[a[1] for a in angles[:2]]))


# -------------------------------------------------------------------------------------------------------------------
# 6. flip symmetry
# -------------------------------------------------------------------------------------------------------------------
FLIP_SIZES = [(31, 100), (24, 90), (40, 133), (16, 64), (33, 97), (48, 150), (20, 77), (37, 120)]
FLIP_SEED = 31          # checked on the CPU with oracle/parseq_oracle.py on Pillow's views of these crops: see the test's docstring
FLIP_MARGIN = 1e-2


def test_flip_symmetry():
    """Eight seeded crops read with 'flip', then the same crops turned by 180 degrees (an exact flip of both axes) read with 'flip': the two
    views of a crop are the same two images in the other order, so wherever the better view leads by more than FLIP_MARGIN the winners are
    complementary and the strings equal.  The lead is taken from `forward` + `parseq_postprocess`, not from `orient`; at most 2 of the 8
    crops may fall under the margin.  (CPU oracle on these crops, FLIP_SEED = 31: the smallest lead is 0.081, none under the margin.)"""
    m = _model('bf16x3')
    crops = _crops(FLIP_SIZES, FLIP_SEED)
    turned = [c.flip(0, 1).contiguous() for c in crops]
    va, _ = orientation_views(crops, 'flip')
    vb, _ = orientation_views(turned, 'flip')
    assert torch.equal(va[:, 0], vb[:, 1]) and torch.equal(va[:, 1], vb[:, 0])
    with torch.inference_mode():
        _, lengths, probs, _ = _postprocess(m(va.flatten(0, 1)).contiguous(), m.eos_id)
        ra, rb = m.orient(va), m.orient(vb)
    keys = R.keys(probs.cpu().numpy(), lengths.cpu().numpy(), 2, 'mean')
    lead = np.abs(keys[:, 0] - keys[:, 1])
    print('leads', lead)
    clear = lead > FLIP_MARGIN
    assert int((~clear).sum()) <= 2
    sa, sb = m.tokenizer.decode_logits(ra.logits)[0], m.tokenizer.decode_logits(rb.logits)[0]
    for b in np.nonzero(clear)[0]:
        assert int(ra.view[b]) + int(rb.view[b]) == 1 and int(ra.view[b]) == int(keys[b].argmax()), b
        assert sa[b] == sb[b], b


# -------------------------------------------------------------------------------------------------------------------
# 7. the command lines
# -------------------------------------------------------------------------------------------------------------------
def _load_script(name, path):
    import importlib.util
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, path))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_read_cli_auto_rotate(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip('PIL.Image')
    import read as read_cli
    from oracle.make_resize_golden import make_input
    upright, other = make_input(40, 150, 1), make_input(30, 111, 0)
    files = [str(tmp_path / 'upright.png'), str(tmp_path / 'turned.png')]
    Image.fromarray(upright, 'RGB').save(files[0])
    Image.fromarray(np.ascontiguousarray(other[::-1, ::-1]), 'RGB').save(files[1])
    m = _model('bf16x3')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    crops = [torch.from_numpy(a.copy()).to(DEV) for a in (upright, np.ascontiguousarray(other[::-1, ::-1]))]
    views, angles = orientation_views(crops, 'flip', tuple(m.hparams.img_size))
    for extra, prior in (([], None), (['--upright-bias', '-50'], [-50.0, 0.0]), (['--upright-bias', '50'], [50.0, 0.0])):
        read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--auto-rotate', 'flip'] + extra)
        printed = capsys.readouterr().out.splitlines()[1:]
        with torch.inference_mode():
            res = m.orient(views, prior=prior)
        labels, _ = m.tokenizer.read(res.logits)
        chosen = [angles[b][k] for b, k in enumerate(res.view.cpu().tolist())]
        assert printed == [f'{f}: {label}' if a == 0 else f'{f}@{a}: {label}' for f, a, label in zip(files, chosen, labels)]
        if prior is not None:
            assert chosen == ([180, 180] if prior[0] < 0 else [0, 0])
    # the other readers run on the chosen crops: the head lines carry the same names
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--auto-rotate', 'flip', '--upright-bias', '-50', '--nbest', '2'])
    heads = [line for line in capsys.readouterr().out.splitlines()[1:] if not line.startswith('    ')]
    assert heads == printed_with_bias(m, views, angles, files, [-50.0, 0.0])
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--auto-rotate', 'flip', '--upright-bias', '-50', '--boxes'])
    out = capsys.readouterr().out.splitlines()[1:]
    assert [line.split(': ')[0] for line in out[0::2]] == [line.split(': ')[0] for line in heads] and len(out) == 4      # (localize reads the chosen crops again)
    with pytest.raises(SystemExit):
        read_cli.main(['pretrained=parseq', '--images', files[0], '--polygons', files[0], '--auto-rotate', 'flip'])
    assert 'polygon' in capsys.readouterr().err


def printed_with_bias(m, views, angles, files, prior):
    with torch.inference_mode():
        res = m.orient(views, prior=prior)
    labels, _ = m.tokenizer.read(res.logits)
    chosen = [angles[b][k] for b, k in enumerate(res.view.cpu().tolist())]
    return [f'{f}: {label}' if a == 0 else f'{f}@{a}: {label}' for f, a, label in zip(files, chosen, labels)]


def test_read_cli_auto_rotate_regions(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip('PIL.Image')
    import read as read_cli
    from oracle.make_resize_golden import make_input
    from parseq_amd.preprocess import orientation_regions, rectify_resize_batch
    scene = make_input(120, 200, 1)
    f = str(tmp_path / 'scene.png')
    Image.fromarray(scene, 'RGB').save(f)
    quads = [[(10, 10), (150, 14), (148, 50), (9, 44)], [(20, 60), (50, 60), (50, 115), (20, 115)]]      # the second stands on end
    rf = tmp_path / 'scene.txt'
    rf.write_text(''.join(','.join(f'{v}' for p in q for v in p) + '\n' for q in quads), encoding='utf-8')
    m = _model('bf16x3')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    read_cli.main(['pretrained=parseq', '--images', f, '--regions', str(rf), '--device', DEV, '--auto-rotate', 'auto'])
    printed = capsys.readouterr().out.splitlines()[1:]
    regions, shifts = orientation_regions([(0, q) for q in quads], 'auto')
    assert shifts == [(0, 2), (1, 3)]
    batch = rectify_resize_batch([torch.from_numpy(scene.copy()).to(DEV)], regions, tuple(m.hparams.img_size))
    with torch.inference_mode():
        res = m.orient(batch.view(2, 2, *batch.shape[1:]))
        labels, _ = m.tokenizer.read(m(res.images))
    names = [f'{f}#{i}' if 90 * s[k] == 0 else f'{f}#{i}@{90 * s[k]}' for i, (s, k) in enumerate(zip(shifts, res.view.cpu().tolist()))]
    assert printed == [f'{name}: {label}' for name, label in zip(names, labels)] and '@' in names[1]


def test_test_cli_auto_rotate(tmp_path, capsys):
    import io
    from PIL import Image
    from parseq_amd import load_from_checkpoint
    from parseq_amd.evaluate import Evaluator
    cli = _load_script('parseq_test_cli_orient', 'test.py')
    d = tmp_path / 'data' / 'pair'
    d.mkdir(parents=True)
    rng = np.random.default_rng(5)
    for i, (h, w) in enumerate([(30, 110), (44, 90)]):
        Image.fromarray(rng.integers(0, 256, size=(h, w, 3), dtype=np.uint8)).save(d / f'{i}.png')
    (d / 'gt.txt').write_text('0.png hello\n1.png world\n', encoding='utf-8')
    model = make_model('parseq-tiny', 'fp32')
    ckpt = str(tmp_path / 'parseq-tiny.ckpt')
    torch.save({'state_dict': {k: v.cpu() for k, v in model.state_dict().items()}, 'hyper_parameters': dict(model.hparams)}, ckpt)
    results = cli.main([ckpt, '--data_root', str(tmp_path / 'data'), '--auto-rotate', 'flip', 'precision:str=fp32'])
    printed = capsys.readouterr().out
    # by hand: the chosen logits into the unchanged Evaluator
    model = load_from_checkpoint(ckpt, charset_test='0123456789abcdefghijklmnopqrstuvwxyz', precision='fp32').eval().to(DEV)
    views, _ = orientation_views(cli.load_crops([str(d / '0.png'), str(d / '1.png')], DEV), 'flip', tuple(model.hparams.img_size))
    with torch.inference_mode():
        res = model.orient(views)

    class Chosen:
        tokenizer, charset_adapter, device = model.tokenizer, model.charset_adapter, model.device

        def forward(self, images):
            return res.logits
    ev = Evaluator(Chosen())
    ev.update(views, ['hello', 'world'])
    r = ev.result()
    want = cli.Result('pair', 2, 100 * r.correct / 2, 100 * (1 - r.ned / 2), 100 * r.confidence / 2, r.label_length / 2)
    assert results == [want]
    table = io.StringIO()
    cli.print_results_table([want], table)
    turned = int((res.view != 0).sum())
    assert f'pair: {turned} of 2 crops read turned ({100 * turned / 2:.2f} %)\n' in printed and printed.endswith(table.getvalue())
    assert open(ckpt + '.log.txt').read() == table.getvalue()
    # with --rotation: the experiment the flag exists for; a bias of 50 nats on the first view leaves nothing turned
    again = cli.main([ckpt, '--data_root', str(tmp_path / 'data'), '--rotation', '180', '--auto-rotate', 'flip', '--upright-bias', '50', 'precision:str=fp32'])
    assert 'pair: 0 of 2 crops read turned' in capsys.readouterr().out and again[0].num_samples == 2
    plain = cli.main([ckpt, '--data_root', str(tmp_path / 'data'), '--rotation', '180', 'precision:str=fp32'])
    capsys.readouterr()
    assert plain[0].num_samples == 2 and abs(plain[0].confidence - again[0].confidence) < 1e-2      # view 0 of the turned crops is what --rotation alone reads
