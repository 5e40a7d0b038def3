"""The training step's attention ONE ROUTE AT A TIME, through parseq_op_train_attention_desc: every case of oracle/train_attn_ref.py's
attn_cases() forward and backward.

Every case: seeded inputs; operands in rows wider than H * head_dim (the pad columns NaN) with NaN guard rows behind the last image
(staging is bounded by the row counts, so nothing of them may reach an output); outputs pre-filled with NaN (the old values where the
call accumulates) in rows wider than H * head_dim with FINITE extra rows behind the last image; the reported route equals the route the
case was written for, forward and backward; every stored element within the DERIVED bound of the float64 reference (the bound's terms,
its one chosen constant and the proof that it bites: oracle/train_attn_ref.py, tests/test_train_attn_bound.py); everything outside the
stored elements bit for bit as before — pad columns, extra rows, fp32 outputs replaced by bf16 ones, lse / dsum on the resident routes;
a second run bit-identical.  The worst error / bound per route of one run is recorded in profiles/train_attn_tests.md."""
import ctypes as C
from dataclasses import replace

import pytest
import torch

from oracle import train_attn_ref as A

pytestmark = pytest.mark.gpu
DEV = 'cuda'
EXTRA = 3            # guard rows behind every buffer's last image: NaN behind operands, finite behind outputs
CASES = A.attn_cases()
RATIOS = {}          # route (and key tiles) -> worst error / bound seen (printed by the coverage test)
PAD = {'q': 8, 'kv': 4, 'o': 12, 'dq': 4, 'dkv': 8}      # pad columns per row, by stride (multiples of 4: the bf16 routes want 16-byte rows)


def _nat():
    from gpu_util import native
    return native()


def _bits(x):
    return x.view(torch.int16 if x.dtype == torch.bfloat16 else torch.int32)


class Rows:
    """A device buffer of [images * L + EXTRA, H * hd + pad] elements holding a logical [images, L, H, hd] tensor."""

    def __init__(self, images, L, H, hd, pad, dtype=torch.float32, body=None, fill=float('nan'), extra=float('nan')):
        self.images, self.L, self.H, self.hd, self.ld = images, L, H, hd, H * hd + pad
        buf = torch.full((images * L + EXTRA, self.ld), fill, dtype=dtype)
        buf[images * L:] = extra
        if body is not None:
            buf[:images * L, :H * hd] = body.reshape(images * L, H * hd).to(dtype)
        self.buf = buf.to(DEV)
        self.before = self.buf.clone()

    def ptr(self, image=0):
        return C.c_void_p(self.buf.data_ptr() + image * self.L * self.ld * self.buf.element_size())

    def body(self):
        return self.buf[:self.images * self.L, :self.H * self.hd].cpu().view(self.images, self.L, self.H, self.hd)

    def untouched_outside_body(self):
        a, b = _bits(self.buf).clone(), _bits(self.before).clone()
        a[:self.images * self.L, :self.H * self.hd] = 0
        b[:self.images * self.L, :self.H * self.hd] = 0
        return torch.equal(a, b)

    def untouched(self):
        return torch.equal(_bits(self.buf), _bits(self.before))


BUFFERS = ('q', 'k', 'v', 'd_o', 'out', 'out16', 'lse', 'dsum', 'with_slots', 'qmask', 'kmask')


class Call:
    """The buffers of one case and the descriptor over them.  over, pass_index: no buffers of its own but pass `pass_index` of the
    call `over` as a launch by itself — B images, no pass_B, that pass's query mask, dropout site and slot of every per-image buffer."""

    def __init__(self, c, t, lse_slots=None, over=None, pass_index=None):
        self.c = c
        if over is None:
            self._allocate(c, t, lse_slots)
        else:
            for name in BUFFERS:
                setattr(self, name, getattr(over, name))
        self._describe(c, pass_index)

    def _allocate(self, c, t, lse_slots):
        H, hd = c.H, c.hd
        self.q = Rows(t['q'].shape[0], c.Lq, H, hd, PAD['q'], body=t['q'])
        self.k = Rows(t['k'].shape[0], c.Lk, H, hd, PAD['kv'], body=t['k'])
        self.v = Rows(t['v'].shape[0], c.Lk, H, hd, PAD['kv'], body=t['v'])
        self.d_o = Rows(c.images, c.Lq, H, hd, PAD['o'], body=t['dO'])
        acc = c.kv_accumulate
        self.out = {'o': Rows(c.images, c.Lq, H, hd, PAD['o'], extra=7.0), 'dq': Rows(c.images, c.Lq, H, hd, PAD['dq'], extra=7.0),
                    'dk': Rows(c.dkv_images, c.Lk, H, hd, PAD['dkv'], body=t['dk_old'] if acc else None, extra=7.0),
                    'dv': Rows(c.dkv_images, c.Lk, H, hd, PAD['dkv'], body=t['dv_old'] if acc else None, extra=7.0)}
        self.out16 = {}
        if c.out16:
            self.out16 = {n: Rows(r.images, r.L, H, hd, r.ld - H * hd, dtype=torch.bfloat16, extra=7.0) for n, r in self.out.items()}
        with_slots = c.route == 'wide' if lse_slots is None else lse_slots
        self.lse = torch.full((c.images, H, c.Lq), float('nan'), device=DEV)
        self.dsum = torch.full((c.images, H, c.Lq), float('nan'), device=DEV)
        self.with_slots = with_slots
        self.qmask = t['qmask'].to(torch.uint8).contiguous().to(DEV) if t['qmask'] is not None else None
        self.kmask = None
        if t['kmask'] is not None:
            km = torch.ones(c.B, c.Lk + 3, dtype=torch.uint8)      # the pad columns say "masked": a wrong stride shows
            km[:, :c.Lk] = t['kmask'].to(torch.uint8)
            self.kmask = km.to(DEV)

    def _describe(self, c, pass_index):
        _native, _ = _nat()
        H, hd = c.H, c.hd
        one = pass_index is not None
        p = pass_index if one else 0
        img = p * c.B                                  # the first image of the pass, in every buffer that has one slot per image
        kv_img = 0 if c.kv_shared else img
        assert not (one and (c.pass_loop or c.out16)) and (not one or self.out['dk'].images == c.images)
        d = _native.TrainAttnDesc()
        d.q, d.q_bstride, d.ldq = self.q.ptr(0 if c.q_shared else img), (0 if c.q_shared else c.Lq * self.q.ld), self.q.ld
        d.k, d.v, d.ldkv = self.k.ptr(kv_img), self.v.ptr(kv_img), self.k.ld
        d.qmask = self.qmask.data_ptr() + p * c.Lq * c.Lk if self.qmask is not None else None
        d.kmask, d.ldkm = (self.kmask.data_ptr() if self.kmask is not None else None), c.Lk + 3
        d.o, d.ldo, d.d_o = self.out['o'].ptr(img), self.out['o'].ld, self.d_o.ptr(img)
        d.dq, d.lddq = self.out['dq'].ptr(img), self.out['dq'].ld
        d.dk, d.dv, d.lddkv = self.out['dk'].ptr(img), self.out['dv'].ptr(img), self.out['dk'].ld
        if c.out16:
            d.o16, d.dq16, d.dk16, d.dv16 = (self.out16[n].ptr() for n in ('o', 'dq', 'dk', 'dv'))
        d.kv_accumulate, d.Lq, d.Lk, d.H, d.scale = int(c.kv_accumulate), c.Lq, c.Lk, H, c.scale
        d.drop_site, d.qmask_pstride, d.site_pstride = c.drop_site + p * c.site_pstride, c.Lq * c.Lk, c.site_pstride
        d.pass_B, d.kv_shared, d.pass_loop = (0, 0, 0) if one else (c.pass_B, int(c.kv_shared), c.P if c.pass_loop else 0)
        d.lse, d.dsum = self.lse.data_ptr(), self.dsum.data_ptr()      # given on every route: only the key-streaming one may touch them
        d.head_dim, d.bf16_ops = hd, (_native.PARSEQ_BF16 if c.bf16_ops else _native.PARSEQ_F32)
        d.dropout_p, d.seed = c.dropout, c.drop_seed
        self.d, self.batch = d, (c.B if one else c.images)

    def launch(self, backward):
        _native, lib = _nat()
        route = C.c_int32(-1)
        rc = lib.parseq_op_train_attention_desc(C.byref(self.d), self.batch, 1 if backward else 0, C.byref(route), _native.stream_ptr())
        torch.cuda.synchronize()
        return rc, route.value

    def stored(self):
        """name -> the logical tensor of every output, from the buffers the case says are written"""
        return {n: (self.out16[n] if self.c.out16 else r).body() for n, r in self.out.items()}

    def operands_untouched(self):
        return all(r.untouched() for r in (self.q, self.k, self.v, self.d_o))

    def nothing_else_written(self):
        """pad columns and extra rows of every output; the fp32 outputs when bf16 ones replace them; lse / dsum off the key-streaming route"""
        ok = all(r.untouched_outside_body() for r in list(self.out.values()) + list(self.out16.values()))
        if self.c.out16:
            ok = ok and all(r.untouched() for r in self.out.values())
        if not self.with_slots:
            ok = ok and bool(torch.isnan(self.lse).all()) and bool(torch.isnan(self.dsum).all())
        return ok

    def all_outputs_untouched(self):
        return all(r.untouched() for r in list(self.out.values()) + list(self.out16.values())) and bool(torch.isnan(self.lse).all()) and bool(torch.isnan(self.dsum).all())


def _run(c, t):
    _, lib = _nat()
    call = Call(c, t)
    for backward in (False, True):
        rc, route = call.launch(backward)
        assert rc == 0, (rc, lib.parseq_last_error())
        assert A.ROUTES[route] == c.route, f'{"backward" if backward else "forward"} took {A.ROUTES[route]}, the case was written for {c.route}'
    return call


@pytest.mark.parametrize('case', CASES, ids=[c.name for c in CASES])
def test_attention_against_float64_within_the_derived_bound(case):
    t = A.make_inputs(case)
    want = A.reference(case, t)
    call = _run(case, t)
    got = call.stored()
    key = case.route + (f'/KT{case.kt}' if case.kt else '')
    for name, (v, b) in want.items():
        r = ((got[name].double() - v).abs() / b.clamp_min(1e-300)).nan_to_num(nan=float('inf'))
        nan = int(torch.isnan(got[name].float()).sum())
        ratio, idx = float(r.max()), int(r.flatten().argmax())
        print(f'{case.name}: {name} worst error / bound {ratio:.4f} at flat index {idx} (NaN {nan})')
        RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
        assert nan == 0 and ratio <= 1.0, f'{name}: error / bound {ratio} at flat index {idx}, {nan} NaN'
    assert call.operands_untouched()
    assert call.nothing_else_written(), 'something outside the stored elements was written'
    if case.route == 'wide':
        assert bool(torch.isfinite(call.lse).all()) and bool(torch.isfinite(call.dsum).all())
    call2 = _run(case, t)
    for name, x in call2.stored().items():
        assert torch.equal(_bits(x), _bits(got[name])), f'{name}: two runs differ'


def test_the_cases_reach_every_route():
    """The parametrization as a whole (each case's own test holds the device's report to its route); prints the worst ratio per route."""
    _native, _ = _nat()
    assert tuple(_native.TRAIN_ATTN_ROUTES) == tuple(A.ROUTES)
    assert {c.route for c in CASES} == set(A.ROUTES) - {'none'}
    assert {c.kt for c in CASES if c.route == 'dec_bf16'} == {2, 8}
    for k, r in sorted(RATIOS.items()):
        print(f'worst error / bound  {k:14s} {r:.4f}')


LOOP_CASES = [c for c in CASES if c.pass_loop]


@pytest.mark.parametrize('case', LOOP_CASES, ids=[c.name for c in LOOP_CASES])
def test_pass_walk_pass_batch_and_one_launch_per_pass_agree(case):
    """train_attn_dec_bf16_kernel's three ways through the passes of a batch — pass_loop, pass_B alone, one launch per pass: o and dq are
    the same bits (a pass's soft-max does not see how it was launched); dK / dV are summed in different orders (in the accumulators, or by
    the caller over per-pass copies), so each form's sum over the passes is held to the bound."""
    _, lib = _nat()
    t = A.make_inputs(case)
    want = A.reference(case, t)
    loop = _run(case, t).stored()
    plain = replace(case, pass_loop=False, kv_accumulate=False)
    tp = dict(A.make_inputs(plain))
    for n in ('q', 'k', 'v', 'dO'):
        assert torch.equal(tp[n], t[n])
    batch = _run(plain, tp).stored()
    each = Call(plain, tp)
    for p in range(case.P):
        one = Call(plain, tp, over=each, pass_index=p)
        for backward in (False, True):
            rc, route = one.launch(backward)
            assert rc == 0 and A.ROUTES[route] == 'dec_bf16', (rc, route, lib.parseq_last_error())
    per_pass = each.stored()
    for name in ('o', 'dq'):
        assert torch.equal(_bits(loop[name]), _bits(batch[name])), f'{name}: pass_loop and pass_B differ'
        assert torch.equal(_bits(loop[name]), _bits(per_pass[name])), f'{name}: pass_loop and one launch per pass differ'
    for name in ('dk', 'dv'):
        assert torch.equal(_bits(batch[name]), _bits(per_pass[name])), f'{name}: pass_B and one launch per pass differ'
        old = t[name + '_old'].double() if case.kv_accumulate else 0.0
        summed = batch[name].double().view(case.P, case.B, case.Lk, case.H, case.hd).sum(0) + old
        for tag, got in (('pass_loop', loop[name]), ('sum of the per-pass copies', summed)):
            r = A.worst_ratio({name: got}, {name: want[name]})
            print(f'{case.name}: {name} {tag}: worst error / bound {r:.4f}')
            assert r <= 1.0, (name, tag, r)


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def _base(route, **kw):
    base = {'dec_bf16': dict(hd=32, Lq=17, Lk=49, B=2, H=2, P=2, bf16_ops=True, kv_shared=True), 'enc_bf16': dict(hd=64, Lq=128, Lk=128, bf16_ops=True),
            'mfma': dict(hd=64, Lq=32, Lk=48), 'hd32': dict(hd=32, Lq=17, Lk=49, B=2, H=2, P=2, kv_shared=True), 'hd64': dict(hd=64, Lq=33, Lk=33)}[route]
    return A.AttnCase(name='refusal', route=route, **{**base, **kw})


def _bf16_buffer(call, name):
    r = call.out[name]
    call.out16[name] = Rows(r.images, r.L, r.H, r.hd, r.ld - r.H * r.hd, dtype=torch.bfloat16, extra=7.0)
    return call.out16[name].ptr()


EDGE = A.largest_backward_keys(32, 32)
REFUSALS = [
    # name, case, what to change in the descriptor (call -> None), direction, route reported, fragment of the message
    ('pass_loop-on-enc_bf16', _base('enc_bf16'), lambda k: setattr(k.d, 'pass_loop', 2), False, 'enc_bf16', b"pass_loop is train_attn_dec_bf16_kernel's alone"),
    ('pass_loop-on-mfma', _base('mfma'), lambda k: setattr(k.d, 'pass_loop', 2), True, 'mfma', b"pass_loop is train_attn_dec_bf16_kernel's alone"),
    ('pass_loop-on-hd32', _base('hd32'), lambda k: setattr(k.d, 'pass_loop', 2), True, 'hd32', b"pass_loop is train_attn_dec_bf16_kernel's alone"),
    ('pass_loop-on-hd64', _base('hd64'), lambda k: setattr(k.d, 'pass_loop', 2), False, 'hd64', b"pass_loop is train_attn_dec_bf16_kernel's alone"),
    ('pass_loop-at-the-key-streaming-shape', _base('hd64', Lq=130, Lk=130), lambda k: setattr(k.d, 'pass_loop', 2), False, 'hd64',
     b"pass_loop is train_attn_dec_bf16_kernel's alone"),      # the key-streaming match asks for no pass_loop: the call falls through and is refused there
    ('pass_loop-without-pass_B', _base('dec_bf16'), lambda k: (setattr(k.d, 'pass_loop', 2), setattr(k.d, 'pass_B', 0)), True, 'dec_bf16', b'pass_loop needs pass_B'),
    ('pass_loop-without-kv_shared', _base('dec_bf16'), lambda k: (setattr(k.d, 'pass_loop', 2), setattr(k.d, 'kv_shared', 0)), True, 'dec_bf16', b'pass_loop needs pass_B'),
    ('pass_loop-batch-mismatch', _base('dec_bf16'), lambda k: setattr(k.d, 'pass_loop', 3), False, 'dec_bf16', b'pass_loop needs pass_B'),
    ('pass_B-at-head-width-64', _base('hd64'), lambda k: setattr(k.d, 'pass_B', 2), False, 'hd64', b"several passes per launch only at the decoder's head width"),
    ('o16-on-dec_bf16', _base('dec_bf16'), lambda k: setattr(k.d, 'o16', _bf16_buffer(k, 'o')), False, 'dec_bf16', b'a bf16 output is only written by'),
    ('dq16-on-hd32', _base('hd32'), lambda k: setattr(k.d, 'dq16', _bf16_buffer(k, 'dq')), True, 'hd32', b'a bf16 output is only written by'),
    ('dk16-dv16-on-mfma', _base('mfma'), lambda k: (setattr(k.d, 'dk16', _bf16_buffer(k, 'dk')), setattr(k.d, 'dv16', _bf16_buffer(k, 'dv'))), True, 'mfma',
     b'a bf16 output is only written by'),
    ('dk16-without-dv16', _base('enc_bf16'), lambda k: setattr(k.d, 'dk16', _bf16_buffer(k, 'dk')), True, 'enc_bf16', b'come as a pair'),
    ('dk16-with-kv_accumulate', _base('enc_bf16', kv_accumulate=True),
     lambda k: (setattr(k.d, 'dk16', _bf16_buffer(k, 'dk')), setattr(k.d, 'dv16', _bf16_buffer(k, 'dv'))), True, 'enc_bf16', b'stored, not accumulated'),
    ('head-width-48', _base('hd32'), lambda k: setattr(k.d, 'head_dim', 48), False, 'none', b'head width 48 not in {32, 64}'),
    ('keys-over-the-register-capacity', _base('hd32', Lq=1, Lk=257, P=1, kv_shared=False), lambda k: None, False, 'hd32', b'do not fit'),
    ('lds-backward-one-key-past-the-edge', _base('hd32', Lq=32, Lk=EDGE + 1, P=1, kv_shared=False), lambda k: None, True, 'hd32', b'do not fit'),
]


@pytest.mark.parametrize('name,case,change,backward,route,message', REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals_report_the_route_and_leave_every_output_untouched(name, case, change, backward, route, message):
    _, lib = _nat()
    t = A.make_inputs(case)
    call = Call(case, t, lse_slots=False)
    change(call)
    rc, took = call.launch(backward)
    err = lib.parseq_last_error()
    print(f'{name}: rc {rc} route {A.ROUTES[took]} ({err.decode()})')
    assert rc != 0 and A.ROUTES[took] == route
    assert message in err
    assert call.all_outputs_untouched() and call.operands_untouched()


def test_the_lds_edge_admits_the_forward_on_both_sides_and_the_backward_on_one():
    """train_attn_lds_floats against TA_LDS_CAP at head width 32 and 32 queries: the backward keeps three [queries, keys] images and two
    query-row images where the forward keeps one each, so there is a range of key counts (EDGE + 1 .. 256) whose forward runs and whose
    backward is refused.  Both sides of its lower end, from the plan's own formula; parseq_train_decoder plans both directions before its
    passes start, so a step cannot find this out between its forward and its backward."""
    _, lib = _nat()
    assert A.admitted(32, EDGE, 32, True) and not A.admitted(32, EDGE + 1, 32, True) and A.admitted(32, EDGE + 1, 32, False)
    case = _base('hd32', Lq=32, Lk=EDGE + 1, P=1, kv_shared=False)
    t = A.make_inputs(case)
    call = Call(case, t)
    rc, took = call.launch(False)
    assert rc == 0 and A.ROUTES[took] == 'hd32', lib.parseq_last_error()
    want = A.reference(case, t)
    r = A.worst_ratio({'o': call.out['o'].body()}, {'o': want['o']})
    print(f'{EDGE + 1} keys, forward: worst error / bound {r:.4f}')
    assert r <= 1.0
    rc, took = call.launch(True)
    assert rc != 0 and A.ROUTES[took] == 'hd32' and b'do not fit' in lib.parseq_last_error()
    assert all(call.out[n].untouched() for n in ('dq', 'dk', 'dv'))
    # (EDGE keys, forward and backward, is the case hd32-q32-largest-backward of the parametrized test)
    assert any((c.route, c.Lq, c.Lk) == ('hd32', 32, EDGE) for c in CASES)
