"""Character localisation on the device: the cross-attention map kernel against the CPU restatement
(tests/attn_map_reference.py) and the reference-minted goldens, the geometry kernel against the float64 restatement, `localize`, refusals.

Tolerances of the maps.  fp32: 1e-5, set by the definition (the same operations in fp32, other summation orders).  bf16 and bf16x3: about
four times the largest error of the first run on an MI355X, profiles/attn_maps.md section "Errors of the maps" (the lines `bf16` and
`bf16x3`); the probabilities themselves reach 4e-2 on these weights."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import attn_map_reference as AR
from gpu_util import DEV, make_model, native
from oracle.synth import CONFIGS, synth_images, synth_state_dict

GRIDS, block_map, load_attn_golden = AR.GRIDS, AR.block_map, AR.load_attn_golden
pytestmark = pytest.mark.gpu

# max |A - restatement| allowed; profiles/attn_maps.md "Errors of the maps"
TOL = {'fp32': 1e-5, 'bf16': 2.5e-3, 'bf16x3': 6e-6}      # first run: bf16 6.27e-4, bf16x3 1.52e-6 (fp32 1.97e-7)
LABELS = ['a', 'Hello77', 'abcdefghijklmnopqrstuvwxy']      # one character, a middle length, the full max_label_length = 25


@functools.lru_cache(maxsize=None)
def _model(name, precision):
    return make_model(name, precision)


@functools.lru_cache(maxsize=None)
def _sd(name):
    return synth_state_dict(CONFIGS[name], 0)


def _readings(m, labels):
    """[B, max_label_length + 1] int32 on the host: characters, <eos>, <pad>."""
    L = m.model.max_label_length + 1
    enc = m.tokenizer.encode(labels)[:, 1:]
    rows = torch.full((len(labels), L), m.tokenizer.pad_id, dtype=torch.int32)
    rows[:, :enc.shape[1]] = enc
    return rows


@functools.lru_cache(maxsize=None)
def _reference_maps(name, rounding):
    """The restatement's maps of LABELS on three synthetic crops — computed once per (model, rounding mode) and shared."""
    cfg = CONFIGS[name]
    images = synth_images(3, cfg, seed=77)
    rows = _readings(_model(name, 'fp32'), LABELS)
    with torch.inference_mode():
        memory = AR.encode(_sd(name), cfg, images, rounding)
        maps = AR.attention_map(_sd(name), cfg, AR.content_of(cfg, rows), memory, rounding)
    return images, rows, maps


def _max_err(tag, got, want):
    d = (got.detach().float().cpu() - want).abs().max().item()
    print(f'[{tag}] max |A - restatement| {d:.3e}  (largest entry {want.max().item():.3e})')
    return d


@pytest.mark.parametrize('precision', ['fp32', 'bf16', 'bf16x3'])
@pytest.mark.parametrize('name', ['parseq-tiny', 'parseq'])
def test_maps_against_the_restatement(name, precision):
    images, rows, want = _reference_maps(name, 'bf16' if precision == 'bf16' else None)
    m = _model(name, precision)
    with torch.inference_mode():
        m.model.encode(images.to(DEV))
        got = m.model.attention_maps(rows.to(DEV))
    assert got.shape == want.shape == (3, 26, 128)
    assert _max_err(f'{name} {precision}', got, want) <= TOL[precision]
    lengths = torch.tensor([len(y) for y in LABELS])
    valid = torch.arange(26)[None, :] <= lengths[:, None]
    sums = got.sum(-1).cpu()
    assert (sums[valid] - 1).abs().max() <= 1e-5 and (got.cpu()[~valid] == 0).all()


def _raw_maps(m, content, guard=64, fill=-7.0, ctx_len=None, tokens_null=False, out_null=False):
    """parseq_decode_attention straight on a buffer with `guard` words before and after the map: (status, map, guards intact, buffer)."""
    nat, lib = native()
    B, L = content.shape
    S = m.model.encoder.pos_embed.shape[1]
    buf = torch.full((guard + B * L * S + guard,), fill, dtype=torch.float32, device=DEV)
    plan = m.model._plan(B)
    out = C.c_void_p(buf.data_ptr() + 4 * guard)
    status = lib.parseq_decode_attention(plan, None if tokens_null else nat.ptr(content), B, L if ctx_len is None else ctx_len, None,
                                         None if out_null else out, None, nat.stream_ptr(buf))
    torch.cuda.synchronize()
    intact = bool((buf[:guard] == fill).all() and (buf[-guard:] == fill).all())
    return status, buf[guard:-guard].view(B, L, S), intact, buf


def test_maps_patch16_224_against_the_golden_with_guards():
    """S = 196 is no multiple of the wave size: the last chunk of keys is ragged.  The map is written into the middle of a buffer whose
    words before and after must stay what they were."""
    g, meta = load_attn_golden('parseq-patch16-224')
    cfg = CONFIGS['parseq-patch16-224']
    images = synth_images(meta['candidates'], cfg, seed=meta['crop_seed'])[torch.tensor(meta['candidate_ids'])]
    m = _model('parseq-patch16-224', 'fp32')
    content = torch.from_numpy(g['tgt_in']).to(DEV, torch.int32).contiguous()
    with torch.inference_mode():
        m.model.encode(images.to(DEV))
    status, got, intact, _ = _raw_maps(m, content)
    assert status == 0 and intact
    assert got.shape == (1, 26, 196)
    assert _max_err('parseq-patch16-224 fp32 vs golden', got, torch.from_numpy(g['maps'])) <= TOL['fp32']


def test_maps_parseq_s_bf16x3_from_24_bit_planes_and_from_f32_rows():
    """After `forward` a PARSeq-S bf16x3 plan holds the memory's K as 24-bit planes (the one-launch encoder's tail); after `encode` it
    holds f32 rows.  The map kernel reads either."""
    images, rows, want = _reference_maps('parseq', None)
    m = _model('parseq', 'bf16x3')
    with torch.inference_mode():
        m(images.to(DEV), 25)
        a24 = m.model.attention_maps(rows.to(DEV)).clone()
        m.model.encode(images.to(DEV))
        a32 = m.model.attention_maps(rows.to(DEV)).clone()
    assert _max_err('parseq bf16x3 24-bit planes', a24, want) <= TOL['bf16x3']
    assert _max_err('parseq bf16x3 f32 rows', a32, want) <= TOL['bf16x3']
    d = (a24 - a32).abs().max().item()
    print(f'[parseq bf16x3] 24-bit planes vs f32 rows: max |d| {d:.3e}')
    assert d <= TOL['bf16x3']
    assert not torch.equal(a24, a32)      # the planes hold 16 significant bits: were both maps read from f32 rows they would be equal


def test_map_properties_and_batch_invariance():
    m = _model('parseq-tiny', 'fp32')
    images = synth_images(5, CONFIGS['parseq-tiny'], seed=78).to(DEV)
    labels = ['Q', 'ab', 'Hello', 'x' * 25, '']
    rows = _readings(m, labels).to(DEV)
    with torch.inference_mode():
        m.model.encode(images)
        a5 = m.model.attention_maps(rows).clone()
        m.model.encode(images[:1])
        a1 = m.model.attention_maps(rows[:1]).clone()
    lengths = torch.tensor([len(y) for y in labels])
    valid = torch.arange(26)[None, :] <= lengths[:, None]
    sums = a5.sum(-1).cpu()
    assert (sums[valid] - 1).abs().max() <= 1e-5
    assert (a5.cpu()[~valid] == 0).all() and (a5 >= 0).all()
    assert torch.equal(a1[0], a5[0])      # a wave owns its queries through every head: nothing depends on the batch
    # fewer positions than the model has: the same rows
    with torch.inference_mode():
        m.model.encode(images[:3])
        a_short = m.model.attention_maps(rows[:3, :7].contiguous())
    assert a_short.shape == (3, 7, 128) and (a_short - a5[:3, :7]).abs().max() <= 1e-6


def _geometry_op(maps, lengths, gh, gw, ph, pw):
    nat, lib = native()
    a = torch.as_tensor(maps, dtype=torch.float32).contiguous().to(DEV)
    B, L, _ = a.shape
    ln = torch.as_tensor(lengths, dtype=torch.int32).to(DEV)
    centres = torch.full((B, L, 2), -1.0, device=DEV); boxes = torch.full((B, L, 4), -1.0, device=DEV)
    peak = torch.full((B, L), -5, dtype=torch.int32, device=DEV); mass = torch.full((B, L), -1.0, device=DEV)
    with nat.guard(a):
        nat.check(lib.parseq_op_attention_geometry(nat.ptr(a), nat.ptr(ln), B, L, gh, gw, ph, pw, nat.ptr(centres), nat.ptr(boxes), nat.ptr(peak),
                                                   nat.ptr(mass), nat.stream_ptr(a)))
    return centres, boxes, peak, mass


def _check_geometry(tag, maps, lengths, grid):
    a32 = np.asarray(maps, dtype=np.float32)
    want = AR.geometry(a32, lengths, *grid)
    got = [t.cpu().numpy() for t in _geometry_op(a32, lengths, *grid)]
    dc, db = np.abs(got[0] - want[0]).max(), np.abs(got[1] - want[1]).max()
    print(f'[{tag}] centres max |d| {dc:.3e} px, boxes max |d| {db:.3e} px')
    assert dc <= 1e-2 and db <= 1e-2            # worst-case fp32 accumulation of 256 terms over 224 px is about 3e-3
    assert (got[2] == want[2]).all()
    assert np.abs(got[3] - want[3]).max() == 0
    return got


@pytest.mark.parametrize('grid', GRIDS)
def test_geometry_operator(grid):
    gh, gw, ph, pw = grid
    S = gh * gw
    rng = np.random.default_rng(5)
    a = rng.random((3, 26, S)) ** 4
    a /= a.sum(-1, keepdims=True)
    _check_geometry(f'random {gh}x{gw}', a, [25, 0, 9], grid)
    # the hand-made maps of the host tests: one-hot, blocks, a block on the border, a tie, and an invalid row
    rows = [block_map(gh, gw, r, c, 1, 1) for r, c in ((0, 0), (3, 5), (gh - 1, gw - 1))]
    rows += [block_map(gh, gw, 2, 3, k, mm) for k in (1, 2, 5) for mm in (1, 2, 5)]
    rows += [block_map(gh, gw, gh - 2, gw - 2, 2, 2)]
    edge = np.zeros((gh, gw)); edge[0, 0] = 0.45; edge[1, 0] = 0.45; edge[0, gw - 1] = 0.10
    tie = np.full((1, 1, S), 0.5 / (S - 2)); tie[0, 0, 70] = 0.25; tie[0, 0, 17] = 0.25
    rows += [edge.reshape(1, 1, S), tie, block_map(gh, gw, 1, 1, 1, 1)]
    hand = np.concatenate(rows, axis=1)
    L = hand.shape[1]
    centres, boxes, peak, mass = _check_geometry(f'hand-made {gh}x{gw}', hand, [L - 2], grid)
    np.testing.assert_allclose(boxes[0, 1], [5 * pw, 3 * ph, 6 * pw, 4 * ph], rtol=0, atol=1e-3)      # a one-hot map: its cell
    np.testing.assert_allclose(boxes[0, 3 + 8], [3 * pw, 2 * ph, 8 * pw, 7 * ph], rtol=0, atol=1e-3)  # the 5 x 5 block: its rectangle
    assert boxes[0, L - 3, 0] == 0 and peak[0, L - 2] == 17
    assert peak[0, L - 1] == -1 and (boxes[0, L - 1] == 0).all() and (centres[0, L - 1] == 0).all() and mass[0, L - 1] == 0


def test_localize_reads_what_forward_reads_and_aligns_labels():
    m = _model('parseq-tiny', 'fp32')
    cfg = CONFIGS['parseq-tiny']
    images = synth_images(4, cfg, seed=79).to(DEV)
    with torch.inference_mode():
        want_strings, _ = m.tokenizer.decode(m(images).softmax(-1))
        loc = m.localize(images)
    strings, chars = m.tokenizer.decode_localization(loc)
    assert strings == want_strings
    assert [''.join(ch for ch, _ in row) for row in chars] == want_strings
    lengths = loc.lengths.cpu()
    assert lengths.tolist() == [len(s) for s in want_strings]
    valid = torch.arange(26)[None, :] <= lengths[:, None]
    assert (loc.maps.sum(-1).cpu()[valid] - 1).abs().max() <= 1e-5 and (loc.peak.cpu()[~valid] == -1).all() and (loc.peak.cpu()[valid] >= 0).all()
    for row in chars:
        for _, (x0, y0, x1, y1) in row:
            assert 0 <= x0 < x1 <= 128 and 0 <= y0 < y1 <= 32
    # labels: the maps of those tokens, then the geometry operator
    labels = ['Hi', 'localize', '', 'z' * 25]
    rows = _readings(m, labels).to(DEV)
    with torch.inference_mode():
        loc = m.localize(images, labels)
        m.model.encode(images)
        maps = m.model.attention_maps(rows)
    assert torch.equal(loc.tokens, rows) and loc.lengths.tolist() == [len(y) for y in labels]
    assert torch.equal(loc.maps, maps)
    centres, boxes, peak, mass = _geometry_op(maps, loc.lengths, 8, 16, 4, 8)
    assert torch.equal(loc.centres, centres) and torch.equal(loc.boxes, boxes) and torch.equal(loc.peak, peak) and torch.equal(loc.peak_mass, mass)
    assert m.tokenizer.decode_localization(loc)[0] == labels
    # raw pixels equal their normalised floats
    g = torch.Generator().manual_seed(3)
    u8 = torch.randint(0, 256, (2, 3, 32, 128), generator=g, dtype=torch.uint8)
    from oracle.parseq_oracle import normalize_u8
    with torch.inference_mode():
        a = m.localize(u8.to(DEV))
        b = m.localize(normalize_u8(u8).to(DEV))
    for f in ('tokens', 'lengths', 'maps', 'centres', 'boxes', 'peak', 'peak_mass'):
        assert torch.equal(getattr(a, f), getattr(b, f)), f


def test_centres_follow_a_memory_built_band_by_band():
    """A memory whose K rows are built so that position i must look at columns 2 i and 2 i + 1.  At depth 1 the cross-attention queries do not
    depend on the memory (AR.cross_attention_queries), so the memory is solved for: token t in band j gets K_h(t) = beta q_h(j) / |q_h(j)| in
    every head h, i.e. memory(t) = Wk^-1 (K(t) - bk).  By Cauchy-Schwarz q_h(i) . K_h(t) is largest on band i in every head, so the peak of
    row i lies in band i whatever beta; with beta large the whole mass does, and the centres' x increase with i."""
    name = 'parseq-tiny'
    cfg, sd = CONFIGS[name], _sd(name)
    m = _model(name, 'fp32')
    label = 'abcdefg'                                 # positions 0 .. 7 (<eos> included): eight bands of two columns on the 8 x 16 grid
    rows = _readings(m, [label])
    n, gh, gw, E, H = len(label) + 1, 8, 16, cfg.embed_dim, cfg.dec_num_heads
    with torch.inference_mode():
        q = AR.cross_attention_queries(sd, cfg, AR.content_of(cfg, rows))[0, :n].double()            # [n, E]
    qh = q.view(n, H, E // H)
    beta = 400.0 * (E // H) ** 0.5 / qh.norm(dim=-1).min().item()      # a head's margin in the scaled scores: 400 (1 - cos) |q| / min |q|
    khat = (beta * qh / qh.norm(dim=-1, keepdim=True)).reshape(n, E)
    w, b = sd['decoder.layers.0.cross_attn.in_proj_weight'][E:2 * E].double(), sd['decoder.layers.0.cross_attn.in_proj_bias'][E:2 * E].double()
    band = (torch.arange(gh * gw) % gw) // 2                                                           # token -> band
    memory = torch.linalg.solve(w, (khat[band] - b).T).T.float().reshape(1, gh * gw, E)
    with torch.inference_mode():
        maps = m.model.attention_maps(rows.to(DEV), memory=memory.to(DEV).contiguous())
    centres, boxes, peak, _ = _geometry_op(maps, [len(label)], gh, gw, 4, 8)
    cx = centres[0, :n, 0].cpu()
    print('[band memory] centre x per position:', [round(v, 2) for v in cx.tolist()])
    assert ((peak[0, :n].cpu() % gw) // 2 == torch.arange(n)).all()
    assert (cx[1:] > cx[:-1]).all()


def test_refusals():
    from parseq_amd import create_model
    nat, lib = native()
    x = torch.zeros(2, 3, 32, 128, device=DEV)
    vit = create_model('vitstr', precision='bf16').eval().to(DEV)
    with pytest.raises(ValueError, match='ViTSTR'):
        vit.localize(torch.zeros(2, 3, *vit.hparams.img_size, device=DEV))
    deep = create_model('parseq-tiny', dec_depth=2, precision='fp32').eval().to(DEV)
    with pytest.raises(ValueError, match='dec_depth'):
        deep.localize(x)
    with pytest.raises(ValueError, match='dec_depth'):
        deep.model.attention_maps(torch.zeros(2, 5, dtype=torch.int32, device=DEV))
    content = torch.zeros(2, 26, dtype=torch.int32, device=DEV)
    with torch.inference_mode():
        deep.model.encode(x)
    status, _, _, buf = _raw_maps(deep, content)
    assert status == -1 and (buf == -7.0).all() and b'dec_depth' in lib.parseq_last_error()
    assert lib.parseq_localize_workspace_bytes(deep.model._plan(2), 2) == 0 and b'dec_depth' in lib.parseq_last_error()
    # the raw call on a model that has the route: context length, null pointers
    m = _model('parseq-tiny', 'fp32')
    with torch.inference_mode():
        m.model.encode(x)
    for ctx_len in (1, 27):
        status, _, _, buf = _raw_maps(m, content, ctx_len=ctx_len)
        assert status == -1 and (buf == -7.0).all() and b'ctx_len' in lib.parseq_last_error()
    status, _, _, buf = _raw_maps(m, content, tokens_null=True)
    assert status == -1 and (buf == -7.0).all() and b'null' in lib.parseq_last_error()
    status, _, _, buf = _raw_maps(m, content, out_null=True)
    assert status == -1 and (buf == -7.0).all() and b'null' in lib.parseq_last_error()
    assert _raw_maps(m, content)[0] == 0
    with pytest.raises(ValueError, match='positions'):
        m.model.attention_maps(torch.zeros(2, 1, dtype=torch.int32, device=DEV))
    # parseq_localize with a null output: refused before the encoder runs
    plan = m.model._plan(2)
    nbytes = lib.parseq_localize_workspace_bytes(plan, 2)
    assert nbytes > 0
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    outs = [torch.full((2 * 26 * 128,), -7.0, device=DEV) for _ in range(6)]
    status = lib.parseq_localize(plan, nat.ptr(x), nat.dtype_code(x.dtype), 2, None, 1, 1, nat.ptr(outs[0]), nat.ptr(outs[1]), nat.ptr(outs[2]),
                                 nat.ptr(outs[3]), nat.ptr(outs[4]), nat.ptr(outs[5]), None, nat.ptr(ws), nbytes, nat.stream_ptr(x))
    torch.cuda.synchronize()
    assert status == -1 and all((o == -7.0).all() for o in outs) and b'null' in lib.parseq_last_error()
    status = lib.parseq_localize(plan, nat.ptr(x), nat.dtype_code(x.dtype), 2, None, 1, 1, nat.ptr(outs[0]), nat.ptr(outs[1]), nat.ptr(outs[2]),
                                 nat.ptr(outs[3]), nat.ptr(outs[4]), nat.ptr(outs[5]), nat.ptr(outs[5]), nat.ptr(ws), nbytes - 1, nat.stream_ptr(x))
    torch.cuda.synchronize()
    assert status == -1 and all((o == -7.0).all() for o in outs) and b'workspace' in lib.parseq_last_error()
