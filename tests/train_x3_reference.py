"""Float64 references of the training step's SPLIT-bf16 products (train_precision = 'bf16x3', train_gemm.h mfma_x3gemm_kernel), with
derived bounds on the device's error, on top of oracle/train_gemm_ref.py (cases, inputs, constants and riders are its own).

The kernel splits every fp32 operand element v on its way into LDS into hi = bf16_rne(v) and lo = bf16_rne(v - hi) (the subtraction is
exact in fp32) and adds up, per 32-deep k step and accumulator, al*bh, then ah*bl, then ah*bh on the bf16 matrix cores.  Two references:

  split   alpha * sum_k (ah*bh + ah*bl + al*bh) + riders in float64.  The three bf16 products are exact in fp32 (8-bit x 8-bit
          significands), so what the device adds to this is 3K fp32 additions and the epilogue:
              |device - split| <= C_TREE * (3K + e) * 2^-24 * S                                                              (1)
          S = |alpha| sum_k (|ah||bh| + |ah||bl| + |al||bh|) + |bias| + |R| + |C_old|: the magnitudes of the terms the route adds up
          (the S of oracle/train_gemm_ref.py on the operands as this route carries them); C_TREE = 2 and e = 4 as there.
  full    alpha * sum_k a*b + riders on the unsplit fp32 operands.  |v - hi - lo| <= 2^-16 |v| (lo is the rounding of a value below
          2^-8 |v| to 8 bits), |lo| <= 2^-8 (1 + 2^-8) |v|, and the dropped al*bl is below 2^-16 (1 + 2^-7) |a||b|:
              |device - full| <= (1) + 3 * 2^-16 * (1 + 2^-7) * |alpha| * sum_k |a||b|                                        (2)

The riders scale both exactly as in oracle/train_gemm_ref.py (gelu_pre: times |gelu'| plus the device's own gelu'; gelu_out: the
Lipschitz constant 1.13 plus gelu's own error); the row sums are sums of the fp32 values before any split, its bound unchanged.

Mutants (tests/test_train_x3_bound.py holds each outside (1) and (2) for every case): 'drop_al_bh', 'drop_ah_bl', 'plain_bf16' (both lo
terms lost), 'drop_chunk' (one split-K chunk, or without a split the last stage), 'lo_prev_stage' (one stage reads the A lo plane the
previous stage parked: the double-buffer mistake), 'lo_from_truncated_hi' (lo = bf16(v - trunc(v)) beside the rounded hi).  The inputs of
train_gemm_ref.make_inputs make a lost lo term add up coherently on the elements where two of the every-eighth positive rows meet: there
every lo equals +0.4375 bf16 ulp.  Two mutants need other values on those rows and get them from mutant_inputs(): a truncated hi differs
from the rounded one only where rounding goes UP (low 16 bits 0x9000 on those rows), and a lo plane of the previous stage differs from
the right one only if the two stages' lo differ (0x7000 in the stage before, 0x9000 in the mutated stage, which is scaled by a power of
two so that it carries at least half of S at any K — a single stage of 32 cannot leave a bound that grows like K^2 otherwise)."""
from __future__ import annotations

import math
from dataclasses import replace

import torch

from oracle import train_gemm_ref as G

X3 = 3                      # PARSEQ_BF16X3, the operand mode
SPLIT_REL = 3 * 2.0 ** -16 * (1 + 2.0 ** -7)
KERNELS_X3 = {13: 'x3_kk', 14: 'x3_kn', 15: 'x3_nk', 16: 'x3_nn'}      # parseq_gemm_kernel (include/parseq_hip.h)
CHARSET_94 = ("0123456789abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ"
              "!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~")      # the 94 characters of the training goldens
MUTANTS = ('drop_al_bh', 'drop_ah_bl', 'plain_bf16', 'drop_chunk', 'lo_prev_stage', 'lo_from_truncated_hi')


def split(x32):
    """fp32 -> (hi, lo) as float32 tensors holding bf16 values, in the device's arithmetic"""
    hi = G.bf16_round(x32)
    return hi, G.bf16_round(x32 - hi)


def bf16_truncate(x32):
    return (x32.view(torch.int32) & ~0xFFFF).view(torch.float32)


def x3_kernel_name(a_kc, b_kc):
    return f'x3_{"k" if a_kc else "n"}{"k" if b_kc else "n"}'


def x3_case(name, M, N, K, a_kc=True, b_kc=True, **kw):
    return G.GemmCase(name=name, M=M, N=N, K=K, kernel=x3_kernel_name(a_kc, b_kc), a_kc=a_kc, b_kc=b_kc, bf16_ops=X3, **kw)


def x3_cases():
    """The operator cases of tests/test_train_x3.py (tile 128 x 128, stage 32): smallest shapes that can still go wrong."""
    cs = []
    for akc in (True, False):
        for bkc in (True, False):
            o = x3_kernel_name(akc, bkc)
            cs.append(x3_case(f'{o}-16x16-one-stage', 16, 16, 32, akc, bkc))
            cs.append(x3_case(f'{o}-edge-tiles-three-stages', 144, 80, 96, akc, bkc, bias=1, asum=True))
            cs.append(x3_case(f'{o}-split-ragged', 144, 80, 1472, akc, bkc, asum=True, accumulate=True))
            cs.append(x3_case(f'{o}-small-scratch-no-split', 144, 80, 1472, akc, bkc, scratch=144 * 80 + 144 + 8, bias=1))      # room for one partial only: 46 stages in one workgroup
    riders = (('bias', dict(bias=1)), ('bias-unaligned', dict(bias=2)), ('resid', dict(rper=26)), ('alpha', dict(alpha=0.75)), ('accumulate', dict(accumulate=True)),
              ('asum-k', dict(asum=True)), ('asum-outer', dict(asum=True, a_kc=False)), ('gelu_pre', dict(gelu_pre='f32')), ('gelu_out', dict(gelu_out='f32')))
    for k, v in riders:
        cs.append(x3_case(f'x3-rider-{k}', 144, 80, 96, **v))
    cs.append(x3_case('x3-riders-all', 144, 80, 96, **G.ALL_RIDERS))
    cs.append(x3_case('x3-riders-all-whole-tiles', 256, 128, 96, **G.ALL_RIDERS))                 # the staged (16-byte) epilogue with everything
    cs.append(x3_case('x3-riders-all-split', 144, 80, 1472, **G.ALL_RIDERS))
    cs.append(x3_case('x3-riders-all-split-outer', 144, 80, 1472, a_kc=False, b_kc=False, **G.ALL_RIDERS))
    cs.append(x3_case('x3-two-stages', 144, 80, 64))
    # 608 tiles, more than two workgroups' worth per CU: the split staging path with the row sums riding on it, as every dW product of a step runs
    cs.append(x3_case('x3-co-resident-asum-k', 4096, 2432, 64, bias=1, asum=True, accumulate=True))
    cs.append(x3_case('x3-co-resident-asum-outer', 4096, 2432, 64, a_kc=False, b_kc=False, asum=True, accumulate=True))
    return [replace(c, seed=100 + i) for i, c in enumerate(cs)]


LO_PREV_STAGE = 1          # the stage 'lo_prev_stage' mutates: the second of the contraction (it exists when K >= 64)


def mutant_inputs(c, t, mutant):
    """The inputs a mutant is judged on (see the module's docstring): `t` itself for most."""
    if mutant not in ('lo_from_truncated_hi', 'lo_prev_stage'):
        return t
    t = dict(t)
    for key in ('A', 'B'):
        x = t[key].clone()
        rows = x[::8].view(torch.int32)
        if mutant == 'lo_from_truncated_hi':
            x[::8] = ((rows & ~0xFFFF) | 0x9000).view(torch.float32)          # rounds UP by 0.4375 ulp, every element alike
        else:
            s = LO_PREV_STAGE
            rows = rows.clone()
            rows[:, 32 * s:32 * s + 32] = (rows[:, 32 * s:32 * s + 32] & ~0xFFFF) | 0x9000      # lo = -0.4375 ulp in the mutated stage, +0.4375 before it
            x[::8] = rows.view(torch.float32)
            if key == 'A':
                x[:, 32 * s:32 * s + 32] *= 2.0 ** max(0, math.ceil(math.log2(c.K / 32)))          # the stage carries half of S or more
        t[key] = x
    return t


def mutants_of(c):
    m = ['drop_al_bh', 'drop_ah_bl', 'plain_bf16', 'drop_chunk', 'lo_from_truncated_hi']
    if c.K >= 64:
        m.append('lo_prev_stage')
    return m


def _products(c, t, mutant=''):
    """-> split product, S of its terms, full product, sum |a||b|: float64 [M, N]"""
    A, B = t['A'], t['B']
    ah, al = (x.double() for x in split(A))
    bh, bl = (x.double() for x in split(B))
    S = ah.abs() @ bh.abs().T + ah.abs() @ bl.abs().T + al.abs() @ bh.abs().T
    alm, blm = al, bl
    if mutant == 'lo_from_truncated_hi':
        alm, blm = G.bf16_round(A - bf16_truncate(A)).double(), G.bf16_round(B - bf16_truncate(B)).double()
    elif mutant == 'lo_prev_stage':
        s = LO_PREV_STAGE
        alm = al.clone()
        alm[:, 32 * s:32 * s + 32] = al[:, 32 * s - 32:32 * s]
    terms = [] if mutant == 'plain_bf16' else [(alm, bh), (ah, blm)]
    if mutant == 'drop_al_bh':
        terms = [(ah, blm)]
    elif mutant == 'drop_ah_bl':
        terms = [(alm, bh)]
    terms.append((ah, bh))
    k1 = c.K
    if mutant == 'drop_chunk':           # the last split's chunk, or without a split the last stage of the contraction
        splits, k_chunk = c.plan()
        k1 = (splits - 1) * k_chunk if splits > 1 else (c.K - 1) // c.bk * c.bk
    prod = sum(x[:, :k1] @ y[:, :k1].T for x, y in terms)
    return prod, S, A.double() @ B.double().T, A.double().abs() @ B.double().abs().T


def expected(c, t, mutant=''):
    """name -> ((split value, bound (1)), (full value, bound (2))) for every output of the case: 'C', 'gelu_out', 'asum' as far as they are on.
    With a mutant: the split value carries the deliberate error (the bounds and the full value are the unmutated ones)."""
    prod, S_terms, full, absfull = _products(c, t, mutant)
    u, ct = G.U, G.C_TREE
    out = {}
    refs = []
    for p, extra in ((prod, 0.0), (full, SPLIT_REL * abs(c.alpha) * absfull)):
        v, S = G._epilogue(c, t, p, S_terms, c.K)
        bound = ct * (3 * c.K + G.E_EPI) * u * S + extra
        if t['pre'] is not None:
            gp = G.gelu_grad64(t['pre'].double())
            v = v * gp
            bound = (ct * (3 * c.K + G.E_EPI + 1) * u * S + extra) * gp.abs() + ct * u * G.E_GELU * S
        refs.append((v, bound))
    if c.c32:
        out['C'] = tuple(refs)
    if c.gelu_out:
        out['gelu_out'] = tuple((G.gelu64(v), G.GELU_LIP * b + ct * G.E_GELU * u * v.abs()) for v, b in refs)
    if c.asum:
        A, old = t['A'].double(), t['asum_old'].double()
        ref = (old + A.sum(1), ct * (c.K + 1) * u * (A.abs().sum(1) + old.abs()))
        out['asum'] = (ref, ref)
    return out


def emulate_f32(c, t, shuffled):
    """The split product in float32 torch arithmetic, stage by stage in the kernel's term order; shuffled: the stages in a random order."""
    ah, al = split(t['A'])
    bh, bl = split(t['B'])
    starts = torch.arange(0, c.K, 32)
    if shuffled:
        starts = starts[torch.randperm(len(starts), generator=torch.Generator().manual_seed(7 + c.seed))]
    prod = torch.zeros(c.M, c.N)
    for k0 in starts.tolist():
        k = slice(k0, k0 + 32)
        prod = ((prod + al[:, k] @ bh[:, k].T) + ah[:, k] @ bl[:, k].T) + ah[:, k] @ bh[:, k].T
    v = torch.tensor(c.alpha, dtype=torch.float32) * prod
    if t['bias'] is not None:
        v = v + t['bias']
    if t['R'] is not None:
        v = v + t['R'][torch.arange(c.M) % c.rper]
    if t['C_old'] is not None:
        v = v + t['C_old']
    if t['pre'] is not None:
        p = t['pre']
        v = v * (0.5 * (1.0 + torch.erf(p * math.sqrt(0.5))) + p * torch.exp(-0.5 * p * p) / math.sqrt(2.0 * math.pi))
    out = {}
    if c.c32:
        out['C'] = v
    if c.gelu_out:
        out['gelu_out'] = torch.nn.functional.gelu(v)
    if c.asum:
        out['asum'] = t['asum_old'] + t['A'].sum(1)
    return out


def ratios(got, want):
    """name -> (worst |got - split| / bound (1), worst |got - full| / bound (2)); a NaN anywhere gives inf"""
    out = {}
    for name, refs in want.items():
        r = []
        for v, b in refs:
            q = (got[name].double() - v).abs() / b.clamp_min(1e-300)
            r.append(float(torch.where(torch.isnan(q), torch.full_like(q, float('inf')), q).max()))
        out[name] = tuple(r)
    return out


def linear_expected(x, W, bias, R, rper, dy, dW0, db0, pre, want_gelu, want_dx):
    """lin_fwd / lin_bwd in the bf16x3 mode at one Linear (x [M, K], W [N, K], dy [M, N]): name -> ((split value, bound), (full value, bound))
    for 'y', 'gelu', 'dW', 'db', 'dx'.  Each product through `expected` above; the padded head contracts dX over N rounded up to 32 (zeros)."""
    M, K = x.shape
    N = W.shape[0]
    base = dict(bias=None, R=None, C_old=None, asum_old=None, pre=None)
    fwd = x3_case('y', M, N, K, bias=1, rper=rper, gelu_out='f32' if want_gelu else '')
    w = expected(fwd, dict(base, A=x, B=W, bias=bias, R=R))
    out = {'y': w['C']}
    if want_gelu:
        out['gelu'] = w['gelu_out']
    dw = x3_case('dW', N, K, M, accumulate=True)
    out['dW'] = expected(dw, dict(base, A=dy.T.contiguous(), B=x.T.contiguous(), C_old=dW0))['C']
    dbv = db0.double() + dy.double().sum(0)
    dbb = G.C_TREE * (M + 1) * G.U * (dy.double().abs().sum(0) + db0.double().abs())
    out['db'] = ((dbv, dbb), (dbv, dbb))
    if want_dx:
        Np = -(-N // 32) * 32
        pad = lambda v: torch.nn.functional.pad(v, (0, Np - N))      # noqa: E731
        dx = x3_case('dx', M, K, Np, gelu_pre='f32' if pre is not None else '')
        out['dx'] = expected(dx, dict(base, A=pad(dy), B=pad(W.T.contiguous()), pre=pre))['C']
    return out
