"""Float64 reference of the training step's attention, one call of train_attn() at a time, with a DERIVED componentwise bound on
the device's error (tests/test_train_attn.py drives every route of lib_train.hip's train_attn_plan() through
parseq_op_train_attention_desc; tests/test_train_attn_bound.py proves on the CPU that the bound holds and bites).

The operation (parseq_amd/csrc/train_attn.h TrainAttnArgs): a batch of P passes of B images, image bf = p B + bl, H heads.
    x[l, j] = scale q[l] . k[j];  masked where qmask[p][l, j] or kmask[bl][j];  p = softmax_j(x);  f = the dropout factor of element
    ((bl H + h) Lq + l) Lk + j at site drop_site + p site_pstride (oracle/decoder_backward.py Dropout, the device generator bit for bit)
    o = (p f) v;   dp = (dO v^T) f;   dS = p (dp - sum_j p dp) scale;   dq = dS k;   dk = dS^T q;   dv = (p f)^T dO
q is image bf's or shared by all; k / v are image bf's or, kv_shared, image bl's; dk / dv are stored per image bf or, pass_loop, summed
over the passes into image bl's rows; kv_accumulate adds the old values.  On the two bf16 routes q, k, v and dO are first rounded to
bf16 (round to nearest even): that is the operation those kernels define.

The bound.  u = 2^-24 (fp32), U16 = 2^-8 (bf16: eight significand bits, so round-to-nearest errs by up to 2^-9 of the binade's TOP,
which is 2^-8 of a value at its bottom — the same figure oracle/train_gemm_ref.py uses for a bf16 output).  Every accumulation on every
route is fp32 over exact (bf16 x bf16) or once-rounded (fp32 x fp32) products, so a sum of n terms errs by at most (n + 1) u sum|terms|
whatever its order (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2).  Term by term, first order:
  score      |d x|   <= (hd + 2) u scale sum_d |q||k|  +  4 u (|x| + |x - max|)     the product, the scale, the subtraction of the row maximum,
                                                                                    the factor scale log2(e) and its own two roundings
  exponent   A       =  |d x| + E_EXP 2^-23                                         relative error of e = exp(x - max); 0 where masked
  soft-max   rho     =  A + sum_j p A + (Lk + 4) u                                  relative error of p = e / sum e (the sum, 1 / sum, the product)
  forward    |d o|   <= sum_j p f |v| (rho + (Lk + 3) u)  +  U_P sum_j p f |v|      U_P = U16 on the bf16 routes (the un-normalised e f is rounded
                                                                                    to bf16 before it meets V; 1 / sum is applied to the result), 0 on fp32
  d P        |d dp|  <= f (hd + 2) u sum_d |dO||v|
  row dot    |d dot| <= sum_j p |dp| (rho + (Lk + 2) u) + sum_j p |d dp|
  d S        E_dS    =  |dS| (rho + 4 u) + p scale (|d dp| + |d dot|)
  dq         <= sum_j |k| E_dS + (Lk + 1) u sum_j |dS||k|  +  U_S sum_j |dS||k|     U_S = U16 on the bf16 routes (dS is rounded before dq and dk)
  dk         <= sum_l |q| E_dS + (n + 1) u sum_l |dS||q|  +  U_S sum_l |dS||q|      n = Lq, or P Lq when pass_loop sums the passes in the accumulators
  dv         <= sum_l p f |dO| (rho + u) + (n + 1) u sum_l p f |dO|  +  U_P sum_l p f |dO|     (on the bf16 routes the backward rounds the normalised p f)
  kv_accumulate: + u (|old| + |new|);   a bf16 output (o16, dq16, dk16, dv16): + U16 |value|
The fp32 terms (everything with u, rho, E_dS) are multiplied by C_TREE = 2: the matrix cores' internal adders are not promised to round
to nearest (a truncating adder errs by one ulp, not half), and the factor swallows the second-order terms (rho < 1e-3 everywhere here).
The U16 terms are NOT: they are conversions to bf16, which round to nearest and so err by at most U16 / (1 + U16) of the exact value; the
U16^2 this leaves is what the rounding of an already rounded-and-erring value (second order) can use.  The key-streaming route
(train_attn_wide.h) takes p = exp(x - lse) with lse = max + log(sum) from the forward and the row dot as rowsum(dO o) from the stored o:
its rho carries 4 u (|lse| + |x - lse|) more and its row-dot term takes sum_d |dO||v| in place of |dp| and hd + 2 more roundings.

E_EXP = 4 (ulps of fp32) is the one constant not read off the kernels.  No stated accuracy of v_exp_f32 was available to take it
from, so it was chosen against torch's float32 exp2 / exp on the CPU, which stay below
1 ulp of the float64 value over [-60, 0] (tests/test_train_attn_bound.py::test_the_exponent_constant_covers_float32_exp2 measures it),
with the room OpenCL's full profile gives a device exponential (3 ulp) and one ulp more for expf's own argument scaling.

Inputs (make_inputs): Gaussian q, k, v, dO and, so that what can go wrong shows:
  * keys 0 and Lk - 1 are never masked (every query keeps a key: the kernels' precondition, asserted), and their value rows are +-8 times
    the others': a lost last tile, a last key taken for padding or a wrong key count in the dropout index moves outputs far outside the bound;
  * the last query row and key 0 are COHERENT rows in the manner of train_gemm_ref._operand (positive, low mantissa bits set so that bf16
    rounding moves every element down by 0.44 ulp), scaled by 4 and 2, and key Lk - 1 is the bf16 rounding of key 0: on rounded operands the
    two keys tie exactly and share the row's probability, on unrounded ones key 0's score is 0.2 % larger at a score near 30 — 6 % in the odds,
    against value rows of opposite sign.  An operand that was not rounded cannot hide behind U16 there.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import torch

from oracle.decoder_backward import Dropout

U = 2.0 ** -24
U16 = 2.0 ** -8
C_TREE = 2
E_EXP = 4
LOG2E = 1.44269504088896340736

# enum parseq_train_attn_route (include/parseq_hip.h), by value
ROUTES = ('dec_bf16', 'enc_bf16', 'mfma', 'wide', 'hd32', 'hd64', 'none')
BF16_ROUTES = ('dec_bf16', 'enc_bf16')
TA_QB, TA_NACC, TA_LDS_CAP = 32, 32, 150 * 1024      # train_attn.h / lib_train.hip

MUTANTS = ('last_tile', 'last_key_padding', 'drop_index_padded', 'no_drop_on_dp', 'site_of_pass0', 'qmask_of_pass0', 'kmask_by_image',
           'kv_shared_ignored', 'no_accumulate', 'accumulate_unasked', 'pass_loop_last_only', 'no_scale_in_ds', 'not_rounded', 'dq_summed')


@dataclass(frozen=True)
class AttnCase:
    name: str
    route: str                   # ROUTES: the route the case must take
    hd: int
    Lq: int
    Lk: int
    B: int = 2                   # images of a pass
    H: int = 2
    P: int = 1                   # passes; P > 1 goes with pass_B = B
    bf16_ops: bool = False
    qmask: bool = False          # one [Lq, Lk] mask per pass
    kmask: bool = False          # [B, ldkm] key padding, ldkm = Lk + 3
    dropout: float = 0.0
    kv_shared: bool = False
    pass_loop: bool = False
    kv_accumulate: bool = False
    q_shared: bool = False
    out16: bool = False          # the bf16 outputs of the 128 x 128 kernel
    seed: int = 0
    drop_site: int = 2
    site_pstride: int = 8
    drop_seed: int = 0x1234_5678_9ABC_DEF1

    @property
    def kt(self):                # key tiles of the train_attn_dec_bf16_kernel instantiation
        return 0 if self.route != 'dec_bf16' else (8 if self.Lk > 32 else 2)

    @property
    def pass_B(self):
        return self.B if self.P > 1 or self.kv_shared else 0

    @property
    def images(self):
        return self.P * self.B

    @property
    def scale(self):
        return float(torch.tensor(1.0 / math.sqrt(self.hd), dtype=torch.float32))

    @property
    def rounded(self):
        return self.route in BF16_ROUTES

    @property
    def dkv_images(self):
        return self.B if self.pass_loop else self.images


def lds_floats(Lq, Lk, hd, backward):
    """train_attn.h train_attn_lds_floats: the dynamic LDS of train_attn_kernel, in floats"""
    nq = min(Lq, TA_QB)
    return 2 * Lk * (hd + 1) + (2 if backward else 1) * nq * (hd + 1) + (3 if backward else 1) * nq * (Lk + 1)


def admitted(Lq, Lk, hd, backward):
    """what train_attn_plan's `fits` answers for the VALU route: LDS within TA_LDS_CAP and dK / dV within the 32 accumulators of 256 threads"""
    return lds_floats(Lq, Lk, hd, backward) * 4 <= TA_LDS_CAP and Lk * hd <= TA_NACC * 256


def largest_backward_keys(Lq, hd):
    Lk = 1
    while admitted(Lq, Lk + 1, hd, True):
        Lk += 1
    return Lk


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _coherent(g, n):
    """n values in [0.67, 1) whose bf16 rounding moves each DOWN by 0.44 of a bf16 ulp (train_gemm_ref._operand)"""
    coh = torch.rand(n, generator=g, dtype=torch.float32) * 0.3 + 0.68
    return ((coh.view(torch.int32) & ~0x3FFFF) | 0x17000).view(torch.float32)


def make_inputs(c: AttnCase):
    """The logical tensors of a case, float32 / bool on the CPU.  q [1 or P B, Lq, H, hd]; k, v [B or P B, Lk, H, hd] (kv_shared: one per
    image of a pass); dO [P B, Lq, H, hd]; qmask [P, Lq, Lk]; kmask [B, Lk]; dk_old, dv_old [B or P B, Lk, H, hd] (pass_loop: one per image of a pass)."""
    g = torch.Generator().manual_seed(5000 + c.seed)
    nq, nkv = (1 if c.q_shared else c.images), (c.B if c.kv_shared else c.images)
    t = {'q': torch.randn(nq, c.Lq, c.H, c.hd, generator=g) * 1.5, 'k': torch.randn(nkv, c.Lk, c.H, c.hd, generator=g) * 1.5,
         'v': torch.randn(nkv, c.Lk, c.H, c.hd, generator=g), 'dO': torch.randn(c.images, c.Lq, c.H, c.hd, generator=g)}
    t['q'][:, -1] = 4.0 * _coherent(g, nq * c.H * c.hd).view(nq, c.H, c.hd)
    t['k'][:, 0] = 2.0 * _coherent(g, nkv * c.H * c.hd).view(nkv, c.H, c.hd)
    t['v'][:, 0] *= 8.0
    if c.Lk > 1:
        t['k'][:, -1] = bf16_round(t['k'][:, 0])
        t['v'][:, -1] = -8.0 * t['v'][:, -1].abs() * torch.sign(t['v'][:, 0])
    t['dO'][:, -1] *= 4.0
    qm = torch.rand(c.P, c.Lq, c.Lk, generator=g) < 0.3
    km = torch.rand(c.B, c.Lk, generator=g) < 0.25
    qm[..., 0] = qm[..., -1] = False
    km[:, 0] = km[:, -1] = False
    t['qmask'] = qm if c.qmask else None
    t['kmask'] = km if c.kmask else None
    t['dk_old'] = torch.randn(c.dkv_images, c.Lk, c.H, c.hd, generator=g) * 2.0
    t['dv_old'] = torch.randn(c.dkv_images, c.Lk, c.H, c.hd, generator=g) * 2.0
    assert not _masked(c, t).all(-1).any(), 'a query row without a key'
    return t


def _masked(c, t, qmask0=False, kmask_by_image=False):
    """[P, B, 1, Lq, Lk] bool"""
    m = torch.zeros(c.P, c.B, 1, c.Lq, c.Lk, dtype=torch.bool)
    if t['qmask'] is not None:
        qm = t['qmask'][:1].expand(c.P, -1, -1) if qmask0 else t['qmask']
        m = m | qm[:, None, None]
    if t['kmask'] is not None:
        km = t['kmask'][None].expand(c.P, -1, -1)
        if kmask_by_image:       # image p B + bl reads row p B + bl of a mask that has B rows: what lies behind it (here: the rows again, rolled)
            km = torch.stack([t['kmask'].roll(p, 1) if p else t['kmask'] for p in range(c.P)])
        m = m | km[:, :, None, None]
    return m


def _factors(c, site0=False, padded=False):
    """dropout multipliers [P, B, H, Lq, Lk] of the case"""
    d = Dropout(c.dropout, c.drop_seed)
    nk = -(-c.Lk // 32) * 32 if padded else c.Lk
    return torch.stack([d.factor(c.drop_site + (0 if site0 else p * c.site_pstride), (c.B, c.H, c.Lq, nk))[..., :c.Lk] for p in range(c.P)]).double()


def _heads(x, c, n):
    """[n images, L, H, hd] -> [P, B, H, L, hd] (one image for all, or one per image of a pass, broadcast)"""
    x = x.permute(0, 2, 1, 3)
    if n == c.images:
        return x.reshape(c.P, c.B, *x.shape[1:])
    return x.reshape(1, n, *x.shape[1:]).expand(c.P, c.B if n == 1 else n, *x.shape[1:])


def _rows(x, c):
    """[P, B, H, L, hd] -> [P B, L, H, hd]"""
    return x.reshape(c.images, *x.shape[2:]).permute(0, 2, 1, 3)


def reference(c: AttnCase, t, mutant: str = ''):
    """name -> (value float64, bound float64) for 'o', 'dq', 'dk', 'dv', each [images, L, H, hd] ('dk', 'dv': dkv_images).
    mutant: one deliberate error in the REFERENCE (MUTANTS; tests/test_train_attn_bound.py: each must leave the bound)."""
    assert not mutant or mutant in MUTANTS
    rnd = (lambda x: bf16_round(x)) if c.rounded and mutant != 'not_rounded' else (lambda x: x)
    kv_n = t['k'].shape[0]
    if mutant == 'kv_shared_ignored':        # image p B + bl reads K / V rows of image p B + bl: pass 0 is right, the others read what lies behind
        kx = torch.cat([t['k'].roll(p, 0) for p in range(c.P)])
        vx = torch.cat([t['v'].roll(p, 0) for p in range(c.P)])
        k, v = _heads(rnd(kx).double(), c, c.images), _heads(rnd(vx).double(), c, c.images)
    else:
        k, v = _heads(rnd(t['k']).double(), c, kv_n), _heads(rnd(t['v']).double(), c, kv_n)
    q = _heads(rnd(t['q']).double(), c, t['q'].shape[0])
    dO = _heads(rnd(t['dO']).double(), c, c.images)
    hd, Lq, Lk, scale = c.hd, c.Lq, c.Lk, c.scale
    masked = _masked(c, t, qmask0=mutant == 'qmask_of_pass0', kmask_by_image=mutant == 'kmask_by_image').expand(-1, -1, c.H, -1, -1).clone()
    if mutant == 'last_tile':
        masked[..., (Lk - 1) // 16 * 16:] = True
    elif mutant == 'last_key_padding':
        masked[..., Lk - 1] = True
    f = _factors(c, site0=mutant == 'site_of_pass0', padded=mutant == 'drop_index_padded')
    wide = c.route == 'wide'
    UP = US = U16 if c.rounded else 0.0

    x = scale * (q @ k.transpose(-1, -2))
    absx = scale * (q.abs() @ k.abs().transpose(-1, -2))
    xm = x.masked_fill(masked, float('-inf'))
    mx = xm.amax(-1, keepdim=True)
    a = torch.where(masked, torch.zeros_like(x), xm - mx)
    e = torch.where(masked, torch.zeros_like(x), torch.exp(a))
    lsum = e.sum(-1, keepdim=True)
    p = e / lsum
    A = (hd + 2) * U * absx + 4 * U * (x.abs() + a.abs()) + E_EXP * 2.0 ** -23
    if wide:
        lse = mx + torch.log(lsum)
        A = A + 4 * U * (lse.abs() + (x - lse).abs())
    A = torch.where(masked, torch.zeros_like(A), A)
    rho = A + (p * A).sum(-1, keepdim=True) + (Lk + 4) * U
    pf = p * f
    # every output: (value, fp32 terms, bf16 terms) — C_TREE multiplies the fp32 terms only
    out = {'o': (pf @ v, (pf * (rho + (Lk + 3) * U)) @ v.abs(), UP * (pf @ v.abs()))}

    dP = dO @ v.transpose(-1, -2)
    absdP = dO.abs() @ v.abs().transpose(-1, -2)
    fb = torch.ones_like(f) if mutant == 'no_drop_on_dp' else f
    dp = dP * fb
    ddp = f * (hd + 2) * U * absdP
    W = f * absdP if wide else dp.abs()
    ddot = (p * W * (rho + (Lk + 2 + (hd + 2 if wide else 0)) * U)).sum(-1, keepdim=True) + (p * ddp).sum(-1, keepdim=True)
    dot = (p * dp).sum(-1, keepdim=True)
    dS = p * (dp - dot) * (1.0 if mutant == 'no_scale_in_ds' else scale)
    EdS = dS.abs() * (rho + 4 * U) + p * scale * (ddp + ddot)
    dq = dS @ k
    if mutant == 'dq_summed':
        dq = dq.sum((0, 1), keepdim=True).expand_as(dq)
    out['dq'] = (dq, EdS @ k.abs() + (Lk + 1) * U * (dS.abs() @ k.abs()), US * (dS.abs() @ k.abs()))
    n = c.P * Lq if c.pass_loop else Lq
    dk = dS.transpose(-1, -2) @ q
    bk = EdS.transpose(-1, -2) @ q.abs() + (n + 1) * U * (dS.abs().transpose(-1, -2) @ q.abs())
    dv = pf.transpose(-1, -2) @ dO
    bv = (pf * (rho + U)).transpose(-1, -2) @ dO.abs() + (n + 1) * U * (pf.transpose(-1, -2) @ dO.abs())
    bk16, bv16 = US * (dS.abs().transpose(-1, -2) @ q.abs()), UP * (pf.transpose(-1, -2) @ dO.abs())
    res = {}
    for name, (val, b, b16) in out.items():
        res[name] = (_rows(val, c), C_TREE * _rows(b, c) + _rows(b16, c))
    for name, val, b, b16, old in (('dk', dk, bk, bk16, t['dk_old']), ('dv', dv, bv, bv16, t['dv_old'])):
        if c.pass_loop:
            val = val[-1:] if mutant == 'pass_loop_last_only' else val.sum(0, keepdim=True)
            b, b16 = b.sum(0, keepdim=True), b16.sum(0, keepdim=True)
        val, b, b16 = (z.reshape(-1, *z.shape[2:]).permute(0, 2, 1, 3) for z in (val, b, b16))
        acc = (c.kv_accumulate and mutant != 'no_accumulate') or mutant == 'accumulate_unasked'
        if c.kv_accumulate:
            b = b + U * (old.double().abs() + val.abs())
        if acc:
            val = val + old.double()
        res[name] = (val, C_TREE * b + b16)
    if c.out16:
        res = {name: (val, b + U16 * val.abs()) for name, (val, b) in res.items()}
    return res


def mutants_of(c: AttnCase):
    """The mutants that mean something for a case."""
    m = []
    if c.Lk > 16:
        m.append('last_tile')
    if c.Lk > 1:                 # (one key: p = 1 and dS = 0 whatever the scale)
        m += ['last_key_padding', 'no_scale_in_ds']
    if c.dropout:
        if c.Lk > 1:
            m.append('no_drop_on_dp')
        if c.Lk % 32:
            m.append('drop_index_padded')
        if c.P > 1 and c.B * c.H * c.Lq * c.Lk >= 64:      # (over a handful of elements two sites can draw the same mask)
            m.append('site_of_pass0')
    if c.qmask and c.P > 1 and c.Lk > 2:         # (keys 0 and Lk - 1 are never masked)
        m.append('qmask_of_pass0')
    if c.kmask and c.P > 1 and c.Lk > 2:
        m.append('kmask_by_image')
    if c.kv_shared and c.P > 1:
        m.append('kv_shared_ignored')
    m.append('no_accumulate' if c.kv_accumulate else 'accumulate_unasked')
    if c.pass_loop:
        m.append('pass_loop_last_only')
    # one key: p = 1 whatever the scores, and an unrounded v or dO moves o and dv by 2^-9 of their size, which U16 allows for the rounding of p f
    if c.rounded and c.Lk > 1:
        m.append('not_rounded')
    # (a lone query is the tie row: without masks or dropout dS of key 0 is minus that of key Lk - 1 on equal key rows, dq = 0 in every image)
    if c.q_shared and (c.Lq > 1 or c.dropout or c.qmask or c.kmask):
        m.append('dq_summed')
    return m


def emulate_f32(c: AttnCase, t, shuffled: bool):
    """The route's algorithm in float32 torch with its rounding points (operands; e f before V; p f and dS before the backward's second
    products; exp2 of an fp32 argument on the bf16 routes, exp on the others); shuffled: keys and queries in a random order in every sum."""
    g = torch.Generator().manual_seed(11 + c.seed)
    pk = torch.randperm(c.Lk, generator=g) if shuffled else torch.arange(c.Lk)
    pq = torch.randperm(c.Lq, generator=g) if shuffled else torch.arange(c.Lq)
    rnd = bf16_round if c.rounded else (lambda x_: x_)
    kv_n = t['k'].shape[0]
    q, dO = _heads(rnd(t['q']), c, t['q'].shape[0])[..., pq, :], _heads(rnd(t['dO']), c, c.images)[..., pq, :]
    k, v = _heads(rnd(t['k']), c, kv_n)[..., pk, :], _heads(rnd(t['v']), c, kv_n)[..., pk, :]
    masked = _masked(c, t).expand(-1, -1, c.H, -1, -1)[..., pq, :][..., pk]
    f = _factors(c).float()[..., pq, :][..., pk]
    scale = torch.tensor(c.scale, dtype=torch.float32)
    s = q @ k.transpose(-1, -2)
    if c.rounded:
        s = s.masked_fill(masked, float('-inf'))
        e = torch.exp2((s - s.amax(-1, keepdim=True)) * (scale * torch.tensor(LOG2E, dtype=torch.float32)))
    else:
        s = (s * scale).masked_fill(masked, float('-inf'))
        e = torch.exp(s - s.amax(-1, keepdim=True))
    inv = 1.0 / e.sum(-1, keepdim=True)
    p = e * inv
    o = (rnd(e * f) @ v) * inv if c.rounded else (p * f) @ v
    dp = (dO @ v.transpose(-1, -2)) * f
    dS = p * (dp - (p * dp).sum(-1, keepdim=True)) * scale
    dq = rnd(dS) @ k
    dk = rnd(dS).transpose(-1, -2) @ q
    dv = rnd(p * f).transpose(-1, -2) @ dO
    iq, ik = torch.argsort(pq), torch.argsort(pk)
    out = {'o': _rows(o[..., iq, :], c), 'dq': _rows(dq[..., iq, :], c)}
    for name, val, old in (('dk', dk[..., ik, :], t['dk_old']), ('dv', dv[..., ik, :], t['dv_old'])):
        if c.pass_loop:
            val = val.flip(0).sum(0, keepdim=True) if shuffled else val.sum(0, keepdim=True)
        val = val.reshape(-1, *val.shape[2:]).permute(0, 2, 1, 3)
        out[name] = val + old if c.kv_accumulate else val
    if c.out16:
        out = {name: bf16_round(val) for name, val in out.items()}
    return out


def worst_ratio(got, want):
    """max over every output and element of |got - expected| / bound (a NaN anywhere gives inf)"""
    worst = 0.0
    for name, (v, b) in want.items():
        r = (got[name].double() - v).abs() / b.clamp_min(1e-300)
        r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
        worst = max(worst, float(r.max()))
    return worst


def _c(name, route, hd, Lq, Lk, **kw):
    return AttnCase(name=name, route=route, hd=hd, Lq=Lq, Lk=Lk, **kw)


def attn_cases():
    """The one list both test files parametrize over; B, H, P in 2..3."""
    cs = []
    # ---- train_attn_dec_bf16_kernel, KT = 2 (<= 32 keys): self-attention style, the passes in one launch, both masks, dropout off and on
    for L in (1, 7, 16, 17, 26, 32):
        for drop in (0.0, 0.1):
            cs.append(_c(f'dec2-L{L}-drop{drop:g}', 'dec_bf16', 32, L, L, B=3, H=2, P=3, bf16_ops=True, qmask=True, kmask=True, dropout=drop))
    cs.append(_c('dec2-L17-one-pass-plain', 'dec_bf16', 32, 17, 17, B=3, H=3, bf16_ops=True))
    # ---- KT = 8 (33..128 keys): cross-attention style, K / V shared by the passes, with and without the pass walk, accumulate, shared queries
    i = 0
    for Lq in (1, 17, 32):
        for Lk in (33, 48, 49, 64, 100, 127, 128):
            kw = dict(B=2, H=3, P=3, bf16_ops=True, kv_shared=True, pass_loop=i % 2 == 0, kv_accumulate=i % 4 < 2, q_shared=i % 5 == 0,
                      qmask=i % 3 == 0, kmask=i % 3 == 1, dropout=0.1 if i % 3 != 2 else 0.0)
            cs.append(_c(f'dec8-q{Lq}-k{Lk}' + ''.join(f'-{n}' for n, on in (('loop', kw['pass_loop']), ('acc', kw['kv_accumulate']), ('qshared', kw['q_shared'])) if on),
                         'dec_bf16', 32, Lq, Lk, **kw))
            i += 1
    cs.append(_c('dec8-q26-k128-own-kv', 'dec_bf16', 32, 26, 128, B=2, H=2, P=2, bf16_ops=True, qmask=True, kmask=True, dropout=0.1))
    # ---- train_attn_bf16_kernel: 128 x 128, head width 64
    cs.append(_c('enc16-f32-out', 'enc_bf16', 64, 128, 128, B=2, H=3, bf16_ops=True))
    cs.append(_c('enc16-f32-out-acc', 'enc_bf16', 64, 128, 128, B=2, H=2, bf16_ops=True, kv_accumulate=True))
    cs.append(_c('enc16-bf16-out', 'enc_bf16', 64, 128, 128, B=3, H=2, bf16_ops=True, out16=True))
    # ---- train_attn_kernel<*, 32> in the fp32 mode: the decoder shapes above, a second query block, many keys
    for i, L in enumerate((1, 7, 16, 17, 26, 32)):       # the self-attention shapes, one combination each
        cs.append(_c(f'hd32-L{L}-self', 'hd32', 32, L, L, B=2 + i % 2, H=3 - i % 2, P=2 + i % 2, qmask=i % 3 != 2, kmask=i % 3 != 1, dropout=0.1 if i % 2 == 0 else 0.0))
    i = 0
    for Lq in (1, 17, 32):                               # the cross-attention shapes, one combination each
        for Lk in (33, 48, 49, 64, 100, 127, 128):
            kw = dict(B=2, H=2 + i % 2, P=2 + i % 2, kv_shared=True, kv_accumulate=i % 4 == 1, q_shared=i % 5 == 2, qmask=i % 3 == 1, kmask=i % 3 == 2,
                      dropout=0.1 if i % 3 != 0 else 0.0)
            cs.append(_c(f'hd32-q{Lq}-k{Lk}-cross' + ''.join(f'-{n}' for n, on in (('acc', kw['kv_accumulate']), ('qshared', kw['q_shared'])) if on),
                         'hd32', 32, Lq, Lk, **kw))
            i += 1
    cs.append(_c('hd32-q33-k33-two-blocks', 'hd32', 32, 33, 33, B=2, H=2, P=2, qmask=True, kmask=True, dropout=0.1))
    cs.append(_c('hd32-q40-k26-two-blocks', 'hd32', 32, 40, 26, B=3, H=2, kv_accumulate=True))
    cs.append(_c('hd32-q64-k48-two-blocks', 'hd32', 32, 64, 48, B=2, H=2, P=2, kv_shared=True, dropout=0.1))
    cs.append(_c('hd32-q26-k196', 'hd32', 32, 26, 196, B=2, H=2, P=2, kv_shared=True, kmask=True, dropout=0.1))
    cs.append(_c('hd32-q32-largest-backward', 'hd32', 32, 32, largest_backward_keys(32, 32), B=2, H=2, qmask=True))
    # ... and in the bf16-operand mode past 32 queries: the decoder's bf16 kernel does not take the shape, the call falls through
    cs.append(_c('hd32-q33-bf16-mode-falls-through', 'hd32', 32, 33, 40, B=2, H=2, P=2, bf16_ops=True, qmask=True, dropout=0.1))
    # ---- train_attn_kernel<*, 64>: token counts that are no multiple of 32 / 16, or masks / dropout at head width 64
    for L in (1, 33, 100, 127):
        cs.append(_c(f'hd64-L{L}-masks-drop', 'hd64', 64, L, L, B=2, H=2, qmask=True, kmask=True, dropout=0.1, kv_accumulate=L == 33))
        cs.append(_c(f'hd64-L{L}-plain', 'hd64', 64, L, L, B=3 if L < 100 else 2, H=2))
    cs.append(_c('hd64-q32-k24-plain', 'hd64', 64, 32, 24, B=2, H=3))
    cs.append(_c('hd64-q32-k24-masks-drop', 'hd64', 64, 32, 24, B=2, H=2, qmask=True, kmask=True, dropout=0.1))
    # ---- train_attn_mfma_kernel: shared queries (admitted by the plan), and two query blocks
    cs.append(_c('mfma-q32-k64-qshared', 'mfma', 64, 32, 64, B=3, H=2, q_shared=True))
    cs.append(_c('mfma-q64-k48-acc', 'mfma', 64, 64, 48, B=2, H=2, kv_accumulate=True))
    # ---- the key-streaming kernels
    cs.append(_c('wide-L130', 'wide', 64, 130, 130, B=2, H=2))
    return [replace(c, seed=i) for i, c in enumerate(cs)]
