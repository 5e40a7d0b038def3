"""The in-flight AR decode as one launch (csrc/decoder_tile_loop.h: a workgroup owns 16 images through every step) against the three
launches per step it replaces (csrc/decoder_step.h).  The contract is bit-identity: every accumulator of the loop kernel receives the same
products in the same order, and both cross-attention kernels call one wave-level body (csrc/decoder_attn.h ca24_pair).

The route is taken by `bf16x3` PARSeq-S plans whose K / V are 24-bit rows, for calls with an explicit `slot` (batches in flight), from
PARSEQ_TILE_LOOP_MIN images up; PARSEQ_NO_TILE_LOOP=1 keeps the three-launch form.  Both are read when a plan is created, so every model
below makes its plans, and runs, under its own setting.  Batches: 16 (one full tile), 17 (a second tile with one live row), 33."""
import functools

import pytest
import torch

from gpu_util import DEV, native
from oracle.synth import CONFIGS, synth_images, synth_state_dict

pytestmark = pytest.mark.gpu

NAME = 'parseq'
CFG = CONFIGS[NAME]
BATCHES = (16, 17, 33)
NAN, INF = float('nan'), float('inf')


@functools.lru_cache(maxsize=None)
def _crops():
    return synth_images(max(BATCHES), CFG, seed=977)


def _model(sd, monkeypatch, loop):
    """A bf16x3 model whose plans are made with the tile loop on (from one image up) or off; call `_use` again before running it."""
    from parseq_amd import create_model
    _use(monkeypatch, loop)
    m = create_model(NAME, decode_ar=True, refine_iters=1, precision='bf16x3')
    m.model.load_state_dict(sd)
    return m.eval().to(DEV)


def _use(monkeypatch, loop):
    monkeypatch.setenv('PARSEQ_TILE_LOOP_MIN', '1')
    if loop:
        monkeypatch.delenv('PARSEQ_NO_TILE_LOOP', raising=False)
    else:
        monkeypatch.setenv('PARSEQ_NO_TILE_LOOP', '1')


def _run(m, n, refine_iters, testing=False, crops=None):
    m.model.decode_ar, m.model.refine_iters = True, refine_iters
    with torch.inference_mode():
        out = m((_crops() if crops is None else crops)[:n].to(DEV), None if testing else CFG.max_label_length, slot=0)
    torch.cuda.synchronize()
    return out.float().cpu()


def _both(sd, monkeypatch, runs):
    """{run: logits} of the three-launch form and of the tile loop; the larger batches first, so that neither plan is made twice."""
    out = []
    for loop in (False, True):
        m = _model(sd, monkeypatch, loop)
        out.append({r: _run(m, *r) for r in runs})
        # the route each plan takes, by the profiling families of its launches: one launch for the whole loop, or 27 + 26 around 26 cross-attentions
        n = max(r[0] for r in runs)
        m.model.set_profiling(True, n)
        _run(m, n, 0)
        prof = m.model.get_profile(n)
        print(f'[tile loop {"on" if loop else "off"}, batch {n}] AR loop alone on the device: ' + ', '.join(f'{k} {prof[k][0]:.3f} ms / {prof[k][1]}' for k in
              ('dec.ar_tile_loop', 'dec.step_pre', 'dec.cross_attention', 'dec.step_post')))
        prof = {k: v[1] for k, v in prof.items()}
        m.model.set_profiling(False, n)
        steps = CFG.max_label_length + 1
        want = {'dec.ar_tile_loop': 1, 'dec.step_pre': 0, 'dec.step_post': 0, 'dec.cross_attention': 0} if loop else \
               {'dec.ar_tile_loop': 0, 'dec.step_pre': steps + 1, 'dec.step_post': steps, 'dec.cross_attention': steps}
        assert {k: prof[k] for k in want} == want, (loop, prof)
    return out


def _same(a, b):
    """Equal bits, NaNs included."""
    return a.shape == b.shape and torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_tile_loop_is_bit_identical(monkeypatch):
    runs = [(n, ri) for n in sorted(BATCHES, reverse=True) for ri in (0, 1)]
    off, on = _both(synth_state_dict(CFG, 0), monkeypatch, runs)
    for r in runs:
        assert off[r].shape == (r[0], CFG.max_label_length + 1, 95) and torch.isfinite(off[r]).all()
        assert torch.equal(off[r], on[r]), f'batch {r[0]}, AR + {r[1]}: max |d| {(off[r] - on[r]).abs().max().item():.3e}'


def test_natural_exit(monkeypatch):
    """The testing mode (`max_length=None`, no refinement): the returned length is the step after which every row has read <eos>.  The
    crops are those of a pool that read <eos> before the last step (rows are independent, so they do in any batch), taken in pool order."""
    pool = synth_images(96, CFG, seed=978)
    sd = synth_state_dict(CFG, 0)
    off = _model(sd, monkeypatch, False)
    first = [(row.argmax(-1) == CFG.eos_id).nonzero()[:1].flatten().tolist() for row in _run(off, 96, 0, crops=pool)]
    keep = [i for i, f in enumerate(first) if f and f[0] < CFG.max_label_length][:max(BATCHES)]
    assert len(keep) == max(BATCHES)
    crops = pool[keep]
    want = {n: _run(off, n, 0, True, crops) for n in BATCHES}
    on = _model(sd, monkeypatch, True)
    lengths = []
    for n in BATCHES:
        steps = {first[i][0] for i in keep[:n]}
        assert len(steps) > 1, 'rows finish at different steps'
        assert want[n].shape == (n, max(steps) + 1, 95) and max(steps) + 1 < CFG.max_label_length + 1
        got = _run(on, n, 0, True, crops)
        assert got.shape == want[n].shape and torch.equal(got, want[n]), f'batch {n}: length {got.shape[1]} against {want[n].shape[1]}'
        lengths.append(got.shape[1])
    print(f'[natural exit] returned lengths at batches {BATCHES}: {lengths}')


def _op(qc, kmem, vmem, plane_elems, tile):
    nat, lib = native()
    out = torch.full_like(qc, NAN)
    nat.check(lib.parseq_op_cross_attention_ar24(nat.ptr(qc), nat.ptr(kmem), nat.ptr(vmem), plane_elems, qc.shape[0], tile, nat.ptr(out), nat.stream_ptr()))
    torch.cuda.synchronize()
    return out.cpu()


def _planes(x):
    """f32 [B, 12, 128, 32] -> (the u16 plane followed by the u8 plane as one byte tensor, the values those 24 bits hold)."""
    bits = x.contiguous().view(torch.int32)
    hi = ((bits >> 16) & 0xFFFF).to(torch.int32)
    lo = ((bits >> 8) & 0xFF).to(torch.uint8)
    hi_bytes = torch.stack([(hi & 0xFF).to(torch.uint8), (hi >> 8).to(torch.uint8)], -1)      # little-endian u16
    held = (bits & ~0xFF).view(torch.float32)
    return torch.cat([hi_bytes.flatten(), lo.flatten()]), held


@pytest.mark.parametrize('B', [1, 16, 17])
def test_cross_attention_tile_owner_equals_one_image_per_workgroup(B):
    g = torch.Generator().manual_seed(B)
    H, NK, HD = 12, 128, 32
    qc = torch.randn(B, H * HD, generator=g) * 2.0
    k, v = torch.randn(B, H, NK, HD, generator=g), torch.randn(B, H, NK, HD, generator=g)
    (kp, kh), (vp, vh) = _planes(k), _planes(v)
    plane_elems = B * H * NK * HD
    one = _op(qc.to(DEV), kp.to(DEV), vp.to(DEV), plane_elems, 0)
    tile = _op(qc.to(DEV), kp.to(DEV), vp.to(DEV), plane_elems, 1)
    assert torch.equal(one, tile)
    # and both are the attention: float64 on the values the 24-bit rows hold
    q = (qc.double() * (1.0 / HD) ** 0.5).view(B, H, 1, HD)
    want = (torch.softmax(q @ kh.double().transpose(-1, -2), -1) @ vh.double()).reshape(B, H * HD)
    err = (one.double() - want).abs().max().item()
    print(f'[cross-attention, {B} images] max |d| against float64 {err:.3e}')
    assert err <= 1e-5      # f32 dot products of 32 and 128 terms of O(1) values: a few 1e-7 each


def _mixed_head():
    """A head under which one tile holds rows of every kind the pick has a rule for.  Classes 7 and 70 tie at 48.0 in every row (zero
    weight rows, as tests/test_picks.py 'tie').  Class 33 reads two columns of decoder.norm's output with weights of +3e38 and -3e38: a
    product overflows where the column's value is past 1.13 in magnitude, so by row the logit is NaN (+inf and -inf meet), +inf, -inf, or
    finite and huge — the pick is 33 (NaN or a positive value) or falls through to the tied pair (a negative value or -inf)."""
    sd = synth_state_dict(CFG, 0)
    w, b = sd['head.weight'], sd['head.bias']
    w[7], w[70] = 0.0, 0.0
    b[7] = b[70] = 48.0
    w[33] = 0.0
    w[33, 5], w[33, 200] = 3.0e38, -3.0e38
    return sd


def _neginf_head():
    sd = synth_state_dict(CFG, 0)
    sd['head.bias'][:] = -INF
    return sd


def test_picks_under_ties_and_non_finite_logits(monkeypatch):
    runs = [(33, 0), (33, 1), (17, 0)]
    off, on = _both(_mixed_head(), monkeypatch, runs)
    ar = off[(33, 0)]
    planted = ar[:, :, 33]
    first_tile = planted[:16]
    kinds = {'nan': torch.isnan(first_tile).any(-1), '-inf': (first_tile == -INF).any(-1), '+inf': (first_tile == INF).any(-1),
             'tied': (torch.isfinite(first_tile) & (first_tile < 0)).any(-1)}
    print('[mixed head] rows of the first tile per kind: ' + ', '.join(f'{k} {int(v.sum())}' for k, v in kinds.items()))
    assert all(bool(v.any()) for v in kinds.values()), 'the first tile holds a NaN row, a -inf row, a +inf row and a tied row'
    assert (ar[:, :, 7] == 48.0).all() and (ar[:, :, 70] == 48.0).all()
    for r in runs:
        assert _same(off[r], on[r]), f'batch {r[0]}, AR + {r[1]}'
    # the picks themselves: torch.argmax's rule on these logits (first maximum, NaN above everything)
    pk = ar.argmax(-1)
    assert set(pk.unique().tolist()) == {7, 33}


def test_picks_with_every_logit_minus_inf(monkeypatch):
    """No candidate in any row: the pick is 0 = <eos>, so the testing mode stops after the first step."""
    runs = [(17, 0), (17, 1), (17, 0, True)]
    off, on = _both(_neginf_head(), monkeypatch, runs)
    assert off[(17, 0, True)].shape == (17, 1, 95) and (off[(17, 0)] == -INF).all()
    for r in runs:
        assert _same(off[r], on[r]), r
