"""GPU tests of line reading: parseq_op_stitch_lines against the numpy restatement of tests/line_reference.py, bit for
bit; `resize_batch` on column slices; `read_lines` of the models against the restatement on its own window tensors, against `localize` and
`forward` on the window batch, in chunks, and through read.py."""
import functools

import numpy as np
import pytest
import torch

import line_reference as R
from gpu_util import DEV, make_model, native
from parseq_amd.preprocess import line_plan, line_views, resize_batch

pytestmark = pytest.mark.gpu

IMG = (32, 128)
OUT_KEYS = ('len', 'tokens', 'probs', 'boxes', 'x', 'src', 'confidence')


# -------------------------------------------------------------------------------------------------------------------
# 1. the operator against the restatement
# -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _case(L, C, lines, seed=0):
    """Seeded rows for `lines` lines of 1, 2, 3 or 64 windows (mixed), with everything the definition has a clause for: windows of length
    0, lengths below 0 and above L, tokens outside [0, C), a line whose windows are all empty, centres exactly on both edges of a band, NaN
    and +-inf centres and probabilities, and a three-letter alphabet on a 2-pixel grid, so that neighbouring windows hold many readings of
    one token less than min_sep apart, with probabilities from a set of four (ties).  Lines of height 32 have windows of 128 columns: the
    scale is 1 and a centre lands on the number it was given."""
    rng = np.random.default_rng(1000 * L + 10 * lines + seed)
    counts = [(1, 2, 3, 64, 2, 1, 3, 2)[l % 8] for l in range(lines)] if lines > 1 else [3]
    if lines == 3:
        counts = [64, 1, 2]
    win, first, min_sep = [], [0], []
    for l, K in enumerate(counts):
        h = 32 if l % 3 != 2 else 48
        ww, s = 4 * h, 3 * h
        win += [(k * s if k < K - 1 or K == 1 else (k - 1) * s + s // 2 + 1, ww, h) for k in range(K)]      # the last window sits closer, as a right-aligned one
        first.append(len(win))
        min_sep.append(0.25 * h if l % 5 != 4 else 0.0)
    rows = len(win)
    win = np.array(win, np.int32)
    tokens = np.where(rng.random((rows, L)) < 0.85, rng.integers(1, min(C, 4), (rows, L)) if C > 1 else 0, rng.integers(-2, C + 2, (rows, L))).astype(np.int32)
    lengths = np.where(rng.random(rows) < 0.7, rng.integers(0, L + 1, rows), rng.integers(-2, L + 3, rows)).astype(np.int32)
    probs = rng.choice(np.array([0.25, 0.5, 0.9, 0.99], np.float32), (rows, L))
    probs = np.where(rng.random((rows, L)) < 0.3, rng.random((rows, L)).astype(np.float32), probs).astype(np.float32)
    centres = np.zeros((rows, L, 2), np.float32)
    src_x = win[:, :1] + 2.0 * rng.integers(-2, win[0, 1] // 2 + 3, (rows, L))                 # source pixels, on a grid of 2, a little past both edges
    centres[:, :, 0] = ((src_x - win[:, :1]) * IMG[1] / win[:, 1:2]).astype(np.float32)
    centres[:, :, 1] = rng.uniform(0, IMG[0], (rows, L)).astype(np.float32)
    half = rng.uniform(0.5, 6.0, (rows, L, 2)).astype(np.float32)
    boxes = np.concatenate([centres - half, centres + half], axis=2).astype(np.float32)
    for l in range(lines):
        a, b = first[l], first[l + 1]
        if l % 7 == 5:
            lengths[a:b] = 0                                                                    # everything dropped
        if win[a, 2] == 32 and b - a >= 2:                                                      # band edges, exactly: lo_1 (kept by window 1) and hi_0 (not kept by window 0)
            cut, d = (win[a + 1, 0] + win[a, 0] + win[a, 1]) / 2.0, min_sep[l] / 2.0
            lengths[a:a + 2] = L
            tokens[a:a + 2, :2] = 1
            centres[a + 1, 0, 0] = cut - d - win[a + 1, 0]
            centres[a, 0, 0] = cut + d - win[a, 0]
            if L > 1:
                centres[a + 1, 1, 0] = np.nextafter(np.float32(cut - d - win[a + 1, 0]), np.float32(-1e9))
                centres[a, 1, 0] = np.nextafter(np.float32(cut + d - win[a, 0]), np.float32(-1e9))
    odd = rng.random((rows, L))
    centres[:, :, 0] = np.where(odd < 0.02, np.nan, np.where(odd < 0.03, np.inf, np.where(odd < 0.04, -np.inf, centres[:, :, 0])))
    odd = rng.random((rows, L))
    probs = np.where(odd < 0.03, np.nan, np.where(odd < 0.04, np.inf, np.where(odd < 0.05, -np.inf, probs))).astype(np.float32)
    host = dict(tokens=tokens, lengths=lengths, probs=probs, centres=centres, boxes=boxes, win=win, line_first=np.array(first, np.int32),
                min_sep=np.array(min_sep, np.float64))
    want = R.stitch_lines(tokens, lengths, probs, centres, boxes, win, first, C, IMG, host['min_sep'], 2048)
    return host, want


def _filled(shape, dtype):
    n = int(np.prod(shape)) * torch.empty(0, dtype=dtype).element_size()
    return torch.full((n,), 255, dtype=torch.uint8, device=DEV).view(dtype).view(*shape)


def _outputs(lines, max_out):
    return dict(len=_filled((lines,), torch.int32), tokens=_filled((lines, max_out), torch.int32), probs=_filled((lines, max_out), torch.float32),
                boxes=_filled((lines, max_out, 4), torch.float32), x=_filled((lines, max_out), torch.float64), src=_filled((lines, max_out, 2), torch.int32),
                confidence=_filled((lines,), torch.float32))


def _run_op(dev_in, L, C, max_out, stream=None):
    nat, lib = native()
    rows, lines = dev_in['tokens'].shape[0], dev_in['line_first'].numel() - 1
    out = _outputs(lines, max_out)
    torch.cuda.synchronize()
    with torch.cuda.stream(stream if stream is not None else torch.cuda.current_stream()), nat.guard(dev_in['tokens']):
        nat.check(lib.parseq_op_stitch_lines(*[nat.ptr(dev_in[k]) for k in ('tokens', 'lengths', 'probs', 'centres', 'boxes')], rows, L, C, nat.ptr(dev_in['win']),
                                             IMG[0], IMG[1], nat.ptr(dev_in['line_first']), lines, nat.ptr(dev_in['min_sep']), max_out,
                                             *[nat.ptr(out[k]) for k in OUT_KEYS], nat.stream_ptr(dev_in['tokens'])))
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _truncated(want, max_out):
    """The restatement at a smaller max_out: stores stop there (step 6), nothing else changes."""
    return {k: (v if k in ('len', 'confidence') else np.ascontiguousarray(v[:, :max_out])) for k, v in want.items()}


@pytest.mark.parametrize('lines', [1, 3, 70])
@pytest.mark.parametrize('shape', [(1, 37), (7, 95), (26, 95), (32, 201)], ids=lambda s: 'x'.join(map(str, s)))
def test_op_matches_the_restatement(shape, lines):
    L, C = shape
    host, want = _case(L, C, lines)
    dev_in = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
    print('survivors per line:', want['len'].tolist()[:12], 'of', (np.diff(host['line_first']) * L).tolist()[:12])
    assert want['len'].max() > 0 or L == 1
    for max_out in (2048, 5, 1):
        got = _run_op(dev_in, L, C, max_out)
        ref = _truncated(want, max_out)
        for k in OUT_KEYS:
            assert _same_bits(got[k], ref[k]), (k, max_out)
    again = _run_op(dev_in, L, C, 5)
    side = _run_op(dev_in, L, C, 5, stream=torch.cuda.Stream())
    for k in OUT_KEYS:
        assert _same_bits(again[k], _truncated(want, 5)[k]) and _same_bits(side[k], again[k]), k


def test_op_refusals_leave_the_outputs_alone():
    nat, lib = native()
    L, C = 7, 95
    host, _ = _case(L, C, 3)
    d = {k: torch.from_numpy(v).to(DEV) for k, v in host.items()}
    rows, lines = host['tokens'].shape[0], 3
    out = _outputs(lines, 5)

    def call(rows=rows, L=L, C=C, img_h=IMG[0], img_w=IMG[1], lines=lines, max_out=5, null=None):
        ins = {k: None if null == ('in', k) else nat.ptr(v) for k, v in d.items()}
        outs = {k: None if null == ('out', k) else nat.ptr(v) for k, v in out.items()}
        return lib.parseq_op_stitch_lines(ins['tokens'], ins['lengths'], ins['probs'], ins['centres'], ins['boxes'], rows, L, C, ins['win'], img_h, img_w,
                                          ins['line_first'], lines, ins['min_sep'], max_out, *[outs[k] for k in OUT_KEYS], nat.stream_ptr(d['tokens']))
    for name in [('in', k) for k in d] + [('out', k) for k in OUT_KEYS]:
        assert call(null=name) == -1 and b'null' in lib.parseq_last_error(), name
    for kw, word in ((dict(L=0), b'positions'), (dict(L=33), b'positions'), (dict(lines=0), b'lines'), (dict(rows=2), b'lines'), (dict(max_out=0), b'max_out'),
                     (dict(max_out=2049), b'max_out'), (dict(C=0), b'classes'), (dict(img_h=0), b'input'), (dict(img_w=0), b'input')):
        assert call(**kw) == -1 and word in lib.parseq_last_error(), kw
    torch.cuda.synchronize()
    for k, v in out.items():
        assert bool((v.view(torch.uint8) == 255).all()), k
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((out['len'].view(torch.uint8) == 255).all())


# -------------------------------------------------------------------------------------------------------------------
# 2. windows are column slices: resize_batch reads them in place
# -------------------------------------------------------------------------------------------------------------------
def _line_images(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    return [torch.randint(0, 256, (h, w, 3), dtype=torch.uint8, generator=g).to(DEV) for h, w in sizes]


SIZES = [(32, 100), (32, 128), (32, 129), (32, 500), (48, 1000)]


def test_resize_batch_on_window_slices():
    images = _line_images(SIZES + [(17, 333)], 5)
    win, first = line_plan([tuple(im.shape[:2]) for im in images], IMG)
    views = line_views(images, win, first)
    assert len(views) == len(win) and all(v.data_ptr() == images[l].data_ptr() + 3 * x0 for l in range(len(images))
                                          for v, (x0, _, _) in zip(views[first[l]:first[l + 1]], win[first[l]:first[l + 1]]))      # no copy
    got = resize_batch(views, IMG)
    want = resize_batch([v.contiguous() for v in views], IMG)
    assert torch.equal(got, want) and got.shape == (len(win), 3, *IMG)


# -------------------------------------------------------------------------------------------------------------------
# 3. read_lines of the models
# -------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _model(name, precision):
    return make_model(name, precision)      # AR + one refinement iteration, seeded weights


def _postprocess(logits, eos):
    nat, lib = native()
    rows, L, C = logits.shape
    ids = torch.empty(rows, L, dtype=torch.int32, device=DEV)
    lengths = torch.empty(rows, dtype=torch.int32, device=DEV)
    probs = torch.empty(rows, L, dtype=torch.float32, device=DEV)
    conf = torch.empty(rows, dtype=torch.float32, device=DEV)
    with nat.guard(logits):
        nat.check(lib.parseq_postprocess(nat.ptr(logits), rows, L, C, eos, nat.ptr(ids), nat.ptr(lengths), nat.ptr(probs), nat.ptr(conf), nat.stream_ptr(logits)))
    return ids, lengths, probs, conf


def _restated(m, res, min_sep=0.25):
    """The restatement on the result's own window tensors."""
    w = res.windows
    heights = [int(w.win[int(r), 2]) for r in w.line_first[:-1].cpu()]
    return R.stitch_lines(w.tokens.cpu().numpy(), w.lengths.cpu().numpy(), w.probs.cpu().numpy(), w.centres.cpu().numpy(), w.boxes.cpu().numpy(),
                          w.win.cpu().numpy(), w.line_first.cpu().tolist(), m.model._cfg['num_tokens'] - 2, tuple(m.hparams.img_size),
                          np.array([min_sep * h for h in heights], np.float64), res.tokens.shape[1])


def _assert_lines(res, want):
    got = dict(len=res.lengths, tokens=res.tokens, probs=res.probs, boxes=res.boxes, x=res.x, src=res.src, confidence=res.confidence)
    for k in OUT_KEYS:
        assert _same_bits(got[k].cpu().numpy(), want[k]), k


@pytest.mark.parametrize('precision', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_read_lines_matches_the_existing_calls_and_the_restatement(name, precision):
    m = _model(name, precision)
    images = _line_images(SIZES, 11)
    with torch.inference_mode():
        res = m.read_lines(images)
        w = res.windows
        assert w.line_first.tolist() == [0, 1, 2, 4, 9, 16] and w.images.shape == (16, 3, *IMG)
        _assert_lines(res, _restated(m, res))
        loc = m.localize(w.images)
        for k in ('tokens', 'lengths', 'centres', 'boxes'):
            assert _same_bits(getattr(w, k).cpu().numpy(), getattr(loc, k).cpu().numpy()), k
        logits = m(w.images)
        _, _, probs, conf = _postprocess(logits, m.eos_id)
        assert _same_bits(w.probs.cpu().numpy(), probs.cpu().numpy())
        texts, confs = m.tokenizer.decode_lines(res)
        want_text, _ = m.tokenizer.decode_logits(logits)
        print('lines:', [(t, c) for t, c in zip(texts, confs)], 'survivors', res.lengths.tolist())
        for l in (0, 1):                                 # the one-window lines are the crops as `forward` reads them
            assert texts[l] == want_text[l]
            # the line's confidence is the fp64 product of at most 33 fp32 factors, rounded to fp32 once (2^-24, the fp64 roundings are far below
            # it); parseq_postprocess multiplies the same factors in fp32, at most 32 inexact products of 2^-24 each (its factors of 1.0 are
            # exact): together at most 33 * 2^-24 to first order, and 64 * 2^-24 bounds it with room for the second-order terms
            assert abs(confs[l] - float(conf[l])) <= 64 * 2.0 ** -24 * abs(float(conf[l]))
        # a line of more windows really is stitched from more than one of them
        assert len(set(res.src[4, :int(res.lengths[4]), 0].tolist())) > 1 or int(res.lengths[4]) <= 1


def test_read_lines_in_chunks_equals_single_calls():
    m = _model('parseq-tiny', 'bf16x3')
    images = _line_images([(32, 500)] * 3, 12)
    with torch.inference_mode():
        res = m.read_lines(images, max_batch=8, max_chars=40)
        assert res.windows.line_first.tolist() == [0, 5, 10, 15]
        _assert_lines(res, _restated(m, res))
        for l, im in enumerate(images):
            one = m.read_lines([im], max_chars=40)
            for k in ('lengths', 'tokens', 'probs', 'boxes', 'x', 'src', 'confidence'):
                assert _same_bits(getattr(res, k)[l:l + 1].cpu().numpy(), getattr(one, k).cpu().numpy()), (l, k)
            for k in ('tokens', 'lengths', 'probs', 'centres', 'boxes', 'win'):
                assert _same_bits(getattr(res.windows, k)[5 * l:5 * l + 5].cpu().numpy(), getattr(one.windows, k).cpu().numpy()), (l, k)
        other = m.read_lines(images, min_sep=0.0, overlap=0.5)
        _assert_lines(other, _restated(m, other, 0.0))
        assert other.windows.line_first.tolist() == [0, 7, 14, 21]


def test_read_lines_refusals():
    from parseq_amd import create_model
    nat, lib = native()
    m = _model('parseq-tiny', 'bf16x3')
    images = _line_images([(32, 1000)], 13)              # 11 windows
    with pytest.raises(ValueError, match='max_batch'):
        m.read_lines(images, max_batch=8)
    with pytest.raises(ValueError, match='overlap'):
        m.read_lines(images, overlap=0.9)
    with pytest.raises(ValueError, match='windows'):
        m.read_lines(_line_images([(4, 4000)], 14))
    vit = create_model('vitstr', precision='bf16').eval().to(DEV)
    with pytest.raises(ValueError, match='ViTSTR'):
        vit.read_lines(images)
    deep = create_model('parseq-tiny', dec_depth=2, precision='fp32').eval().to(DEV)
    with pytest.raises(ValueError, match='dec_depth'):
        deep.read_lines(images)
    assert lib.parseq_read_lines_workspace_bytes(deep.model._plan(2), 2) == 0 and b'dec_depth' in lib.parseq_last_error()
    plan = m.model._plan(8)
    assert lib.parseq_read_lines_workspace_bytes(plan, 4096) == 0 and lib.parseq_read_lines_workspace_bytes(plan, 0) == 0
    need = lib.parseq_read_lines_workspace_bytes(plan, 2)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    z = torch.zeros(2, 3, *IMG, dtype=torch.uint8, device=DEV)
    out = _filled((1 << 12,), torch.float64)
    table = torch.tensor([0, 128, 32, 96, 128, 32, 0, 2], dtype=torch.int32, device=DEV)
    sep = torch.tensor([8.0], dtype=torch.float64, device=DEV)
    p = nat.ptr(out)

    def call(rows=2, lines=1, max_out=8, first=nat.ptr(table[6:]), nbytes=need, last=p):
        return lib.parseq_read_lines(plan, nat.ptr(z), 2, rows, 1, 1, nat.ptr(table), first, lines, nat.ptr(sep), max_out, p, p, p, p, p, p, p, p, p, p, p, last,
                                     nat.ptr(ws), nbytes, nat.stream_ptr(z))
    for kw, word in ((dict(lines=0), b'lines'), (dict(lines=3), b'lines'), (dict(max_out=0), b'max_out'), (dict(max_out=4096), b'max_out'), (dict(first=None), b'null'),
                     (dict(last=None), b'null'), (dict(nbytes=need - 1), b'workspace'), (dict(rows=4096), b'batch')):
        assert call(**kw) == -1 and word in lib.parseq_last_error(), kw
    torch.cuda.synchronize()
    assert bool((out.view(torch.uint8) == 255).all())      # refused before any device work


# -------------------------------------------------------------------------------------------------------------------
# 4. the command line
# -------------------------------------------------------------------------------------------------------------------
def test_read_cli_lines(tmp_path, monkeypatch, capsys):
    Image = pytest.importorskip('PIL.Image')
    import read as read_cli
    g = np.random.default_rng(3)
    arrays = [g.integers(0, 256, (32, 500, 3), dtype=np.uint8), g.integers(0, 256, (40, 90, 3), dtype=np.uint8)]
    files = [str(tmp_path / 'line.png'), str(tmp_path / 'word.png')]
    for a, f in zip(arrays, files):
        Image.fromarray(a, 'RGB').save(f)
    m = _model('parseq-tiny', 'bf16x3')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', lambda ckpt, **kw: m)
    crops = [torch.from_numpy(a.copy()).to(DEV) for a in arrays]
    with torch.inference_mode():
        labels, _, chars = m.tokenizer.decode_lines(m.read_lines(crops), boxes=True)
        half, _ = m.tokenizer.decode_lines(m.read_lines(crops, overlap=0.5, min_sep=0.0))
        plain, _ = m.tokenizer.read(m(resize_batch(crops, IMG)))
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--lines', '--boxes'])
    printed = capsys.readouterr().out.splitlines()[1:]
    want = []
    for f, label, row in zip(files, labels, chars):
        want += [f'{f}: {label}', '    ' + ' '.join(f'{ch}[{x0:.1f},{y0:.1f},{x1:.1f},{y1:.1f}]' for ch, (x0, y0, x1, y1) in row)]
    assert printed == want
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV, '--lines', '--line-overlap', '0.5', '--line-sep', '0'])
    assert capsys.readouterr().out.splitlines()[1:] == [f'{f}: {label}' for f, label in zip(files, half)]
    # without the flag: what read.py printed before there was one
    read_cli.main(['pretrained=parseq', '--images', *files, '--device', DEV])
    assert capsys.readouterr().out == 'Additional keyword arguments: {}\n' + ''.join(f'{f}: {label}\n' for f, label in zip(files, plain))
    # a whole-image quadrilateral read as a line is the line itself, its boxes led back as quadrilaterals
    regions = tmp_path / 'line.txt'
    regions.write_text('0,0,500,0,500,32,0,32\n')
    read_cli.main(['pretrained=parseq', '--images', files[0], '--device', DEV, '--lines', '--boxes', '--regions', str(regions)])
    out = capsys.readouterr().out.splitlines()[1:]
    assert out[0] == f'{files[0]}#0: {labels[0]}' and len(out) == 2
    assert out[1] == '    ' + ' '.join(f'{ch}[{x0:.1f},{y0:.1f},{x1:.1f},{y0:.1f},{x1:.1f},{y1:.1f},{x0:.1f},{y1:.1f}]' for ch, (x0, y0, x1, y1) in chars[0])
    with pytest.raises(SystemExit):
        read_cli.main(['pretrained=parseq', '--images', files[0], '--lines', '--nbest', '2'])
    assert '--lines' in capsys.readouterr().err
