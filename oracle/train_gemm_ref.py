"""Float64 reference of the training step's products and row kernels, with a DERIVED bound on the device's error.

The operator tests (tests/test_train_gemm.py) drive `sgemm()`, `lin_fwd` / `lin_bwd`, `train_ln_fwd` / `ln_bwd` of lib_train.hip
through parseq_op_train_gemm / _linear / _layernorm and hold every stored element to

    |device - expected| <= C_TREE * (K + e) * 2^-24 * S                                           (1)

expected: the operation in float64 (exact erf) on the operands AS THE ROUTE ROUNDS THEM — untouched on the VALU and fp32 matrix-core
routes, torch.bfloat16 round-to-nearest-even of both operands in the bf16-operand mode (fp32 in memory or bf16 shadows alike).
S = |alpha| sum_k |a||b| + |bias| + |R| + |C_old| on those rounded operands: bf16 x bf16 products are exact in fp32 and fp32 x fp32
products round once, every addition of the fp32 accumulation rounds once, so ANY summation tree of the K products and the e epilogue
terms errs by at most (K + e) u S to first order, u = 2^-24 (Higham, Accuracy and Stability of Numerical Algorithms, section 4.2: the
bound does not depend on the order).  The split-K fold is part of that tree.

C_TREE = 2.  What the summation tree leaves open is not its shape but the rounding of the matrix core's internal additions, which the
ISA does not promise to be round-to-nearest: a truncating adder errs by up to one ulp (2 u) per addition instead of half of one.  The
factor also swallows the second-order terms of (1) at K <= 6144 (K u < 4e-4).  It was chosen from this reasoning before any device
output was looked at and is not fitted.

The riders:
  * gelu_pre: the stored value is v * gelu'(pre); (1) is scaled by |gelu'(pre)| and C_TREE * E_GELU * u * S is added for the device's
    gelu' itself (Abramowitz & Stegun 7.1.26 erf, |error| <= 1.5e-7 = 2.5 u, halved by the cdf's 0.5, a five-term Horner chain and one
    v_exp_f32 in fp32: under 6 u absolute in all; E_GELU = 8);
  * gelu_out: gelu(v) with |gelu'| <= 1.13: 1.13 * (1) + C_TREE * E_GELU * u * |v|  (gelu_erf: |error| <= 0.5 |v| 1.2e-7 + its fp32 evaluation);
  * a bf16 output (c16, gelu_out16): + 2^-8 |value|;
  * asum: the row sums of A — of the bf16 values when A is a shadow, of the UNROUNDED fp32 values otherwise — with S = sum_k |a| + |old|.
The same construction bounds the column sums (`rows` terms) and LayerNorm (sums over E, then over the rows).

Inputs: Gaussian, except that every eighth row of A and of B (outer index % 8 == 0) is POSITIVE with the low mantissa bits set so that
bf16 rounding moves every element the same way (down, by ~0.5 bf16 ulp), and so that a second rounding of 0.75 x or -1.5 x moves every
element the same way too (up, by a quarter of an ulp; see _operand).  On the elements where two such rows meet, an operand that was
not rounded (or a row sum that was taken from rounded values) shifts the result coherently, by ~2^-9 S — far outside (1) at every K used —
where on Gaussian data the shift would grow like sqrt(K) and hide inside a bound that grows like K.  The other 63 of 64 elements see
cancellation as real gradients do.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, replace

import torch

U = 2.0 ** -24
C_TREE = 2
E_EPI = 4          # alpha, bias + residual, old C, the final fma
E_GELU = 8
GELU_LIP = 1.13    # max |gelu'|

# tile geometry of lib_train.hip / train_gemm.h (the plan below mirrors gemm_plan(); the GPU test compares it with the reported route)
MG_BM = MG_BN = 128
MG_BK, BG_BK, BH_BK, SG_BK = 16, 32, 64, 16
SPLIT_TARGET = 512
STEP_SCRATCH = 16 << 20          # floats: the training step's scratch
LNB_ROWS = 4

# parseq_gemm_kernel (include/parseq_hip.h)
KERNELS = ('valu', 'mfma_f32', 'bf16_kk', 'bf16_kn', 'bf16_nk', 'bf16_nn', 'b16_kk', 'b16_kn', 'b16_nk', 'b16_nn', 'a16_nn', 'both16_k', 'both16_t')
HAS_WHOLE = ('both16_k', 'both16_t')


@dataclass(frozen=True)
class GemmCase:
    name: str
    M: int
    N: int
    K: int
    kernel: str                  # the route the case is written for (KERNELS)
    a_kc: bool = True            # A contiguous along the contraction (else along m)
    b_kc: bool = True
    a16: bool = False            # bf16 shadow in memory
    b16: bool = False
    bf16_ops: bool = False
    bias: int = 0                # 0: none, 1: given, 2: given at a pointer offset by one float (not 16-byte aligned)
    rper: int = 0                # 0: no residual; else R has max(rper, 1) rows, row m reads R[m % rper]
    alpha: float = 1.0
    accumulate: bool = False
    asum: bool = False
    gelu_pre: str = ''           # '', 'f32', 'b16'
    gelu_out: str = ''           # '', 'f32', 'b16'
    c32: bool = True
    c16: bool = False
    scratch: int = STEP_SCRATCH  # floats; 0: no scratch at all
    whole: bool = False
    seed: int = 0

    @property
    def rounded(self):
        return self.kernel not in ('valu', 'mfma_f32')

    @property
    def bk(self):
        return {'valu': SG_BK, 'mfma_f32': MG_BK, 'both16_k': BH_BK, 'both16_t': BH_BK}.get(self.kernel, BG_BK)

    def plan(self):
        """(splits, k_chunk) as gemm_plan() of lib_train.hip decides them; the VALU kernel never splits."""
        if self.kernel == 'valu':
            return 1, self.K
        M, N, K, bk = self.M, self.N, self.K, self.bk
        tiles = -(-M // MG_BM) * -(-N // MG_BN)
        splits = 1
        if tiles < 256:
            splits = min(-(-SPLIT_TARGET // tiles), K // (4 * min(bk, BG_BK)))
            splits = max(min(max(splits, 1), self.scratch // (M * N + M)), 1)
        k_chunk = -(-(-(-K // splits)) // bk) * bk
        return -(-K // k_chunk), k_chunk


def bf16_round(t):
    return t.to(torch.bfloat16).to(t.dtype)


def _operand(g, rows, K, shadow):
    x = torch.randn(rows, K, generator=g, dtype=torch.float32)
    coh = (torch.rand(rows // 8 + 1, K, generator=g, dtype=torch.float32) * 0.3 + 0.68)[: x[::8].shape[0]]
    # low 16 bits 0x7000: bf16 round-to-nearest moves the value DOWN by 0.44 of a bf16 ulp, every element alike.  The two bits above them
    # are 01 and the value lies in [0.67, 1): the bf16 significand is 4 q + 1 >= 171, so that 0.75 x (or -1.5 x) needs two more bits,
    # stays in a binade of the same spacing and a SECOND rounding to bf16 moves every element up by a quarter of an ulp, again alike
    bits = (coh.view(torch.int32) & ~0x3FFFF) | 0x17000
    x[::8] = bits.view(torch.float32)
    return bf16_round(x) if shadow else x


def make_inputs(c: GemmCase):
    """The logical tensors of a case, float32 on the CPU: A [M, K], B [N, K], and the riders (None where off)."""
    g = torch.Generator().manual_seed(1000 + c.seed)
    t = {'A': _operand(g, c.M, c.K, c.a16), 'B': _operand(g, c.N, c.K, c.b16)}
    scale = math.sqrt(c.K)
    t['bias'] = torch.randn(c.N, generator=g) * scale if c.bias else None
    t['R'] = torch.randn(max(c.rper, 1), c.N, generator=g) * scale if c.rper else None
    t['C_old'] = torch.randn(c.M, c.N, generator=g) * scale if c.accumulate else None
    t['asum_old'] = torch.randn(c.M, generator=g) * scale if c.asum else None
    pre = torch.randn(c.M, c.N, generator=g) * 1.5 if c.gelu_pre else None
    t['pre'] = bf16_round(pre) if c.gelu_pre == 'b16' else pre
    return t


def gelu64(v):
    return 0.5 * v * (1.0 + torch.erf(v * math.sqrt(0.5)))


def gelu_grad64(v):
    return 0.5 * (1.0 + torch.erf(v * math.sqrt(0.5))) + v * torch.exp(-0.5 * v * v) / math.sqrt(2.0 * math.pi)


def _epilogue(c, t, prod, absprod, K, R_rows=None):
    """prod, absprod: sum_k a b and sum_k |a||b| in float64 -> (v, S) before the GELU riders"""
    M = prod.shape[0]
    v = c.alpha * prod
    S = abs(c.alpha) * absprod
    if t['bias'] is not None:
        v = v + t['bias'].double()
        S = S + t['bias'].double().abs()
    if t['R'] is not None:
        rows = torch.arange(M) % c.rper if R_rows is None else R_rows
        v = v + t['R'].double()[rows]
        S = S + t['R'].double()[rows].abs()
    if t['C_old'] is not None:
        v = v + t['C_old'].double()
        S = S + t['C_old'].double().abs()
    return v, S


def expected(c: GemmCase, t, mutant: str = ''):
    """name -> (expected float64, bound float64) for every output of the case: 'C', 'c16', 'gelu_out', 'asum' as far as they are on.
    mutant: one deliberate error in the REFERENCE (tests/test_train_gemm_bound.py: each must leave the bound, which proves that the
    device test can fail): 'drop_chunk', 'last_row', 'not_rounded', 'rounded_twice', 'rper_ignored', 'no_accumulate', 'asum_rounded'."""
    A, B = t['A'].double(), t['B'].double()
    rnd = c.rounded
    Ar, Br = (bf16_round(A), bf16_round(B)) if rnd else (A, B)
    absprod = Ar.abs() @ Br.abs().T
    Am, Bm = Ar, Br
    if mutant == 'not_rounded':
        Am, Bm = A, B
    elif mutant == 'rounded_twice':      # alpha folded into the operand and the scaled operand rounded again
        Am = bf16_round(c.alpha * Ar) / c.alpha
    prod = Am @ Bm.T
    if mutant == 'drop_chunk':           # the last split's chunk, or without a split the last stage of the contraction
        splits, k_chunk = c.plan()
        k0 = (splits - 1) * k_chunk if splits > 1 else (c.K - 1) // c.bk * c.bk
        prod = prod - Ar[:, k0:] @ Br[:, k0:].T
    R_rows = torch.arange(c.M).clamp(max=max(c.rper, 1) - 1) if mutant == 'rper_ignored' else None
    tm = dict(t, C_old=None) if mutant == 'no_accumulate' else t
    v, _ = _epilogue(c, tm, prod, absprod, c.K, R_rows)
    _, S = _epilogue(c, t, prod, absprod, c.K)
    bound = C_TREE * (c.K + E_EPI) * U * S
    if t['pre'] is not None:
        gp = gelu_grad64(t['pre'].double())
        v = v * gp
        bound = C_TREE * U * ((c.K + E_EPI + 1) * S * gp.abs() + E_GELU * S)
    if mutant == 'last_row':             # the last row of the last M-tile written from its neighbour
        v = v.clone()
        v[-1] = v[-2]
    out = {}
    if c.c32:
        out['C'] = (v, bound)
    if c.c16:
        out['c16'] = (v, bound + 2.0 ** -8 * v.abs())
    if c.gelu_out:
        gv = gelu64(v)
        gb = GELU_LIP * bound + C_TREE * E_GELU * U * v.abs()
        out['gelu_out'] = (gv, gb + (2.0 ** -8 * gv.abs() if c.gelu_out == 'b16' else 0.0))
    if c.asum:
        src = Ar if (c.a16 or mutant == 'asum_rounded') else A
        base = A if not c.a16 else Ar
        old = t['asum_old'].double()
        out['asum'] = (old + src.sum(1), C_TREE * (c.K + 1) * U * (base.abs().sum(1) + old.abs()))
    return out


def mutants_of(c: GemmCase):
    """The mutants that mean something for a case (a rounding mutant needs an operand that is rounded on the way in, ...)."""
    m = ['drop_chunk', 'last_row']
    if c.rounded and not (c.a16 and c.b16):
        m.append('not_rounded')
    # a second rounding needs an alpha that is not a power of two (else alpha x is a bf16 value already)
    if c.rounded and math.frexp(c.alpha)[0] != 0.5:
        m.append('rounded_twice')
    if c.rper and c.rper < c.M:
        m.append('rper_ignored')
    if c.accumulate:
        m.append('no_accumulate')
    if c.asum and c.rounded and not c.a16:
        m.append('asum_rounded')
    return m


def emulate_f32(c: GemmCase, t, shuffled: bool):
    """The case in float32 torch arithmetic (any summation order is allowed by (1)); shuffled: the contraction in chunks of 32 taken in a
    random order and folded one by one."""
    A, B = t['A'], t['B']
    Ar, Br = (bf16_round(A), bf16_round(B)) if c.rounded else (A, B)
    if shuffled:
        g = torch.Generator().manual_seed(7 + c.seed)
        prod = torch.zeros(c.M, c.N)
        starts = torch.arange(0, c.K, 32)[torch.randperm(-(-c.K // 32), generator=g)]
        for k0 in starts.tolist():
            prod = prod + Ar[:, k0:k0 + 32] @ Br[:, k0:k0 + 32].T
    else:
        prod = Ar @ Br.T
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
    if c.c16:
        out['c16'] = bf16_round(v)
    if c.gelu_out:
        gv = torch.nn.functional.gelu(v)
        out['gelu_out'] = bf16_round(gv) if c.gelu_out == 'b16' else gv
    if c.asum:
        out['asum'] = t['asum_old'] + (Ar if c.a16 else A).sum(1)
    return out


def worst_ratio(got, want):
    """max over every output and element of |got - expected| / bound (a NaN anywhere gives inf)"""
    worst = 0.0
    for name, (v, b) in want.items():
        r = ((got[name].double() - v).abs() / b.clamp_min(1e-300))
        r = torch.where(torch.isnan(r), torch.full_like(r, float('inf')), r)
        worst = max(worst, float(r.max()))
    return worst


def _c(name, M, N, K, kernel, **kw):
    return GemmCase(name=name, M=M, N=N, K=K, kernel=kernel, **kw)


ALL_F32_OPTS = dict(bias=1, rper=7, alpha=0.75, accumulate=True)
ALL_RIDERS = dict(bias=1, rper=26, alpha=0.75, accumulate=True, asum=True, gelu_pre='f32', gelu_out='f32')


def gemm_cases():
    cs = []
    # ---- VALU kernel: nothing aligned, both orientations of each operand, every fp32 option, no scratch
    for akc in (True, False):
        for bkc in (True, False):
            o = 'k' if akc else 'm', 'k' if bkc else 'n'
            cs.append(_c(f'valu-{o[0]}{o[1]}', 67, 95, 26, 'valu', a_kc=akc, b_kc=bkc, scratch=0))
            cs.append(_c(f'valu-{o[0]}{o[1]}-all', 130, 95, 26, 'valu', a_kc=akc, b_kc=bkc, scratch=0, **ALL_F32_OPTS))
    cs.append(_c('valu-bf16mode-unaligned', 67, 95, 26, 'valu', bf16_ops=True, bias=1))              # K % 32 != 0: the bf16 mode falls through
    cs.append(_c('valu-rper-ge-M', 33, 17, 100, 'valu', rper=40, bias=1))
    # ---- fp32 matrix cores
    for akc in (True, False):
        for bkc in (True, False):
            o = 'k' if akc else 'm', 'k' if bkc else 'n'
            cs.append(_c(f'mfma32-{o[0]}{o[1]}-one-tile', 128, 128, 48, 'mfma_f32', a_kc=akc, b_kc=bkc))                 # K / 64 = 0 splits -> 1: direct
            cs.append(_c(f'mfma32-{o[0]}{o[1]}-split-short', 256, 384, 1000 - 8, 'mfma_f32', a_kc=akc, b_kc=bkc))        # 6 tiles, K = 992 in 13 splits of 80: the last is 32
    cs.append(_c('mfma32-many-tiles-direct', 2048, 2048, 64, 'mfma_f32', **ALL_F32_OPTS))                                # 256 tiles: never split
    cs.append(_c('mfma32-direct-all-rper-ge-M', 128, 256, 48, 'mfma_f32', bias=1, rper=128, alpha=-1.5, accumulate=True))
    cs.append(_c('mfma32-split-all', 256, 128, 1488, 'mfma_f32', **ALL_F32_OPTS))
    cs.append(_c('mfma32-split-all-rper-ge-M', 256, 128, 1488, 'mfma_f32', bias=1, rper=300, alpha=-1.5, accumulate=True))
    cs.append(_c('mfma32-small-scratch', 256, 256, 2048, 'mfma_f32', scratch=3 * (256 * 256 + 256) + 5, bias=1))         # 3 splits of 688 (the last 672) where the step's scratch gives 32
    cs.append(_c('mfma32-deep', 128, 128, 6144, 'mfma_f32', a_kc=False, b_kc=False))
    # ---- bf16-operand mode, fp32 operands in memory: the four orientation forms, edge tiles, both epilogues, every rider
    for akc in (True, False):
        for bkc in (True, False):
            kern = f'bf16_{"k" if akc else "n"}{"k" if bkc else "n"}'
            M = 130 if akc else 132                     # an outer-contiguous operand is read in groups of four
            cs.append(_c(f'{kern}-edge-both', M, 95 if bkc else 96, 160, kern, a_kc=akc, b_kc=bkc, bf16_ops=True, bias=1, asum=True))     # direct (splits = 1: K / 128 = 1)
            cs.append(_c(f'{kern}-split-asum', 256, 128, 1504, kern, a_kc=akc, b_kc=bkc, bf16_ops=True, asum=True, accumulate=True))      # staged partials, K = 1504 in 10 splits of 160: the last is 64
            cs.append(_c(f'{kern}-staged-all', 384, 256, 96, kern, a_kc=akc, b_kc=bkc, bf16_ops=True, **ALL_RIDERS))                      # splits = 0 -> 1: the staged epilogue with everything
    cs.append(_c('bf16_kk-edge-M', 130, 128, 64, 'bf16_kk', bf16_ops=True, rper=26))
    cs.append(_c('bf16_kk-edge-N96', 128, 96, 64, 'bf16_kk', bf16_ops=True, bias=1, gelu_out='f32'))
    cs.append(_c('bf16_kk-edge-N95-all', 130, 95, 64, 'bf16_kk', bf16_ops=True, **ALL_RIDERS))
    cs.append(_c('bf16_kk-direct-bias-offset', 128, 128, 64, 'bf16_kk', bf16_ops=True, bias=2, rper=128))
    cs.append(_c('bf16_kk-split-all', 130, 95, 1504, 'bf16_kk', bf16_ops=True, **ALL_RIDERS))
    for k, v in (('bias', dict(bias=1)), ('resid', dict(rper=26)), ('alpha', dict(alpha=0.75)), ('accumulate', dict(accumulate=True)), ('asum', dict(asum=True)),
                 ('gelu_pre', dict(gelu_pre='f32')), ('gelu_out', dict(gelu_out='f32')), ('c16', dict(c16=True))):
        cs.append(_c(f'bf16_kk-staged-{k}', 256, 128, 96, 'bf16_kk', bf16_ops=True, **v))
    cs.append(_c('bf16_kk-head-shape', 9984, 96, 384, 'bf16_kk', bf16_ops=True, bias=1))                                 # 78 x 1 tiles, 3 splits
    cs.append(_c('bf16_kn-wide-output', 4096, 1536, 384, 'bf16_kn', b_kc=False, bf16_ops=True, bias=1, gelu_out='f32'))  # 384 tiles: never split
    cs.append(_c('bf16_nn-deep', 128, 256, 6144, 'bf16_nn', a_kc=False, b_kc=False, bf16_ops=True, asum=True, accumulate=True))
    # ---- shadows
    for akc in (True, False):
        for bkc in (True, False):
            kern = f'b16_{"k" if akc else "n"}{"k" if bkc else "n"}'
            cs.append(_c(f'{kern}-shadowB', 132, 136, 160, kern, a_kc=akc, b_kc=bkc, b16=True, bf16_ops=True, bias=1, asum=True))
            cs.append(_c(f'{kern}-shadowB-split', 256, 128, 1504, kern, a_kc=akc, b_kc=bkc, b16=True, bf16_ops=True, accumulate=True))
    cs.append(_c('a16_nn-K96', 132, 136, 96, 'a16_nn', a_kc=False, b_kc=False, a16=True, b16=True, bf16_ops=True, asum=True, accumulate=True))
    cs.append(_c('a16_nn-K1504-split', 256, 128, 1504, 'a16_nn', a_kc=False, b_kc=False, a16=True, b16=True, bf16_ops=True, asum=True, accumulate=True))
    cs.append(_c('both16_k-edge', 136, 104, 128, 'both16_k', a16=True, b16=True, bf16_ops=True, bias=1, rper=26, c16=True))
    cs.append(_c('both16_k-edge-split', 136, 104, 1472, 'both16_k', a16=True, b16=True, bf16_ops=True, bias=1, gelu_out='b16'))
    cs.append(_c('both16_k-edge-split-even', 136, 104, 1536, 'both16_k', a16=True, b16=True, bf16_ops=True, bias=1, gelu_out='b16'))   # 12 x 128 at either depth: compared with its fp32 twin
    cs.append(_c('both16_k-whole', 256, 384, 128, 'both16_k', a16=True, b16=True, bf16_ops=True, whole=True, bias=1, c32=False, c16=True, gelu_out='b16'))
    cs.append(_c('both16_k-whole-split', 256, 384, 1472, 'both16_k', a16=True, b16=True, bf16_ops=True, whole=True, gelu_pre='b16', c16=True))
    cs.append(_c('both16_k-whole-c16-only', 512, 256, 384, 'both16_k', a16=True, b16=True, bf16_ops=True, whole=True, c32=False, c16=True, gelu_pre='b16'))
    cs.append(_c('both16_t-edge', 132, 136, 128, 'both16_t', a_kc=False, b_kc=False, a16=True, b16=True, bf16_ops=True, asum=True, accumulate=True))
    cs.append(_c('both16_t-edge-split', 132, 136, 1472, 'both16_t', a_kc=False, b_kc=False, a16=True, b16=True, bf16_ops=True, asum=True, accumulate=True))
    cs.append(_c('both16_t-whole', 384, 256, 128, 'both16_t', a_kc=False, b_kc=False, a16=True, b16=True, bf16_ops=True, whole=True, asum=True))
    cs.append(_c('both16_t-whole-split', 384, 256, 6144, 'both16_t', a_kc=False, b_kc=False, a16=True, b16=True, bf16_ops=True, whole=True, asum=True, accumulate=True))
    return [replace(c, seed=i) for i, c in enumerate(cs)]


# ---- the row kernels -------------------------------------------------------------------------------------------------
def colsum_bound(x64, old64=None):
    """column sums over `rows` terms (+ an old value accumulated into): value, bound"""
    rows = x64.shape[0]
    v, S = x64.sum(0), x64.abs().sum(0)
    if old64 is not None:
        v, S = v + old64, S + old64.abs()
    return v, C_TREE * (rows + 1) * U * S


def layernorm_reference(x, gamma, beta, eps, dy=None, add=None, dgamma_old=None, dbeta_old=None):
    """LayerNorm forward and backward by float64 autograd of torch.nn.functional.layer_norm, with bounds built as (1): a row's sums run
    over E terms; xhat carries the relative error of mean and rstd, (E + e) u each, amplified by |x - mean| / |x| cancellation which the
    bound takes from sum |x| / E against the row's standard deviation; dgamma / dbeta then sum `rows` terms.
    Returns name -> (value, bound): 'y' and, with dy, 'dx', 'dgamma', 'dbeta'."""
    E = x.shape[1]
    x64 = x.double().requires_grad_(dy is not None)
    g64, b64 = gamma.double().requires_grad_(dy is not None), beta.double().requires_grad_(dy is not None)
    y = torch.nn.functional.layer_norm(x64, (E,), g64, b64, eps)
    xd = x64.detach()
    mean = xd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(xd.var(1, unbiased=False, keepdim=True) + eps)
    xhat = (xd - mean) * rstd
    # |d xhat| <= rstd * (u |x| + |d mean|) + |xhat| |d rstd| / rstd:  |d mean| <= (E + 1) u mean|x|;  d rstd / rstd <= (E + 4) u + rstd * 2 |d mean| * mean|x - mean| * rstd
    mabs = xd.abs().mean(1, keepdim=True)
    dmean = (E + 1) * U * mabs
    drel = (E + 4) * U + 2.0 * rstd * rstd * dmean * (xd - mean).abs().mean(1, keepdim=True)
    dxhat = C_TREE * (rstd * (U * xd.abs() + dmean) + xhat.abs() * drel + 2 * U * xhat.abs())
    out = {'y': (y.detach(), dxhat * g64.detach().abs() + C_TREE * 2 * U * (xhat.abs() * g64.detach().abs() + b64.detach().abs()))}
    if dy is None:
        return out
    dy64 = dy.double()
    dx, dg, db = torch.autograd.grad(y, (x64, g64, b64), dy64)
    gam = g64.detach()
    gv = dy64 * gam
    m1abs, m2abs = gv.abs().mean(1, keepdim=True), (gv * xhat).abs().mean(1, keepdim=True)
    m2 = (gv * xhat).mean(1, keepdim=True)
    # dx = rstd (g - m1 - xhat m2) + add: every term's own rounding, the sums' (E + 2) u, and the error of xhat and rstd carried through
    inner = gv.abs() + m1abs + xhat.abs() * m2abs
    dm2 = (gv.abs() * dxhat).mean(1, keepdim=True)
    bdx = rstd * (C_TREE * (E + 6) * U * inner + dxhat * m2.abs() + xhat.abs() * dm2) + drel * C_TREE * (rstd * inner)
    if add is not None:
        dx = dx + add.double()
        bdx = bdx + C_TREE * U * (add.double().abs() + dx.abs())
    out['dx'] = (dx, bdx)
    rows = x.shape[0]
    for name, val, terms, err_terms, old in (('dgamma', dg, dy64 * xhat, dy64.abs() * dxhat, dgamma_old), ('dbeta', db, dy64, None, dbeta_old)):
        S = terms.abs().sum(0)
        b = C_TREE * (rows + 4) * U * S
        if err_terms is not None:
            b = b + err_terms.sum(0)
        if old is not None:
            val, b = val + old.double(), b + C_TREE * (rows + 4) * U * old.double().abs()
        out[name] = (val, b)
    return out


# ---- the optimiser step ------------------------------------------------------------------------------------------------
def _f32(x):
    return float(torch.tensor(x, dtype=torch.float32))


def adamw_reference(p, g, m, v, decay, lr, beta1, beta2, eps, weight_decay, step, norm=None, max_norm=0.0, mutant=''):
    """One torch.optim.AdamW step in float64 on flat float32 tensors (decay: bool per element), with the gradient scaled by
    min(1, max_norm / (norm + 1e-6)) when `norm` is given (torch.nn.utils.clip_grad_norm_).  The hyper-parameters cross the C ABI as
    float, so their float32 values are what the reference takes.  Returns name -> (value, bound) for 'p', 'm', 'v'.

    The bound follows the update through fp32 operation by operation, u per rounding:
      grad = g coef                           relative rg = 4 u (the sum, the quotient and the minimum of coef, the product)
      m'   = m + (grad - m)(1 - beta1)        1 - beta is exact for beta in [0.5, 1]; absolute dm below
      v'   = beta2 v + (1 - beta2) grad^2     all terms positive: relative rv = 4 u + 2 rg
      bc1  = 1 - beta1^step, bc2 likewise     a float power is good to one ulp (2 u) and the subtraction cancels: relative 2 u beta^step / bc + u —
                                              334 u on sqrt(bc2) at step 3 with beta2 = 0.999; this term is the conditioning of the
                                              bias correction in fp32, not slack
      p'   = p (1 - lr wd) - (lr / bc1) m' / (sqrt(v') / sqrt(bc2) + eps)
    times C_TREE for the second-order terms and for a divide or a square root that is good to one ulp instead of half of one.
    mutant: one deliberate error (tests/test_train_gemm_bound.py)."""
    lr, beta1, beta2, eps, weight_decay = (_f32(x) for x in (lr, beta1, beta2, eps, weight_decay))
    p, g, m, v = (t.double() for t in (p, g, m, v))
    coef, rg = 1.0, 0.0
    if norm is not None and mutant != 'no_clip':
        coef, rg = min(_f32(max_norm) / (_f32(norm) + _f32(1e-6)), 1.0), 4 * U
    grad = g * coef
    wd = torch.where(decay, weight_decay, 0.0).double()
    if mutant == 'no_decay':
        wd = torch.zeros_like(wd)
    elif mutant == 'decay_everywhere':
        wd = torch.full_like(wd, weight_decay)
    p1 = p * (1.0 - lr * wd)
    t1 = grad - m
    t2 = t1 * (1.0 - beta1)
    mi = m + t2
    dm = U * mi.abs() + U * t2.abs() + (1.0 - beta1) * (U * t1.abs() + rg * grad.abs())
    vi = beta2 * v + (1.0 - beta2) * grad * grad
    rv = 4 * U + 2 * rg
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    r_bc1 = 2 * U * beta1 ** step / bc1 + U
    r_bc2s = 0.5 * (2 * U * beta2 ** step / bc2 + U) + U
    if mutant == 'no_bias_correction':
        bc1 = bc2 = 1.0
    q = vi.sqrt() / math.sqrt(bc2)
    denom = q + eps
    r_den = q / denom * (0.5 * rv + U + r_bc2s + U) + U
    r = mi / denom
    dr = dm / denom + r.abs() * (r_den + U)
    upd = lr / bc1 * r
    dupd = lr / bc1 * dr + upd.abs() * (r_bc1 + 2 * U)
    pn = p1 - upd
    dp = 3 * U * p.abs() + dupd + U * pn.abs()
    return {'p': (pn, C_TREE * dp), 'm': (mi, C_TREE * dm), 'v': (vi, C_TREE * rv * vi)}


def adamw_inputs(numels, seed):
    """Flat p, g, m, v of a model in the middle of training (moments not zero) and a per-tensor decay flag that alternates in runs of
    one and two, so that the flat buffer is cut into many launches: -> p, g, m, v, flags (list of int), decay (bool per element)"""
    gen = torch.Generator().manual_seed(seed)
    n = sum(numels)
    p, g = torch.randn(n, generator=gen) * 0.5, torch.randn(n, generator=gen) * 0.3
    m, v = torch.randn(n, generator=gen) * 0.1, torch.rand(n, generator=gen) * 0.05 + 1e-6
    flags = [int(i % 3 != 1) for i in range(len(numels))]
    decay = torch.cat([torch.full((k,), bool(f)) for k, f in zip(numels, flags)])
    return p, g, m, v, flags, decay


def grad_norm_bound(n, want):
    """parseq_grad_norm reduces through 1024 partial sums of an even share of the elements each (its workspace is 1024 floats): a square
    passes through at most ceil(n / 1024) additions into its partial and 1024 more into the total, whatever the order — and never through
    more than n, adding zero being exact — one rounding each and one for the square itself.  All terms are positive, so that is relative
    on the sum of squares; the root halves it and rounds once.  (2.4e-4 at n = 3 Mi: a lost block of 256 elements is 8e-5 of the
    sum and hides, which is why the test also runs each size with a heavy tail.)"""
    return C_TREE * (0.5 * (min(n, -(-n // 1024) + 1024) + 1) + 1) * U * want
