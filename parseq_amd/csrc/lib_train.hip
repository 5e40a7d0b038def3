// libparseq_hip.so — the training step.
#include "lib_internal.h"

#include "train_gemm.h"
#include "train_rows.h"
#include "train_attn.h"
#include "train_attn_wide.h"
#include "train_vitstr.h"

// -------------------------------------------------------------------------------------------------------------------
// training step, decoder side: loss of system.py:168-199 and its gradients, fp32
// -------------------------------------------------------------------------------------------------------------------
// Scratch shared by the split-K partials of the MFMA GEMM and the partial column sums; part of the caller's workspace.
constexpr size_t TRAIN_SCRATCH_FLOATS = (size_t)16 << 20;
// LayerNorm backward parks rows / LNB_ROWS partial rows of 2E floats at the END of the scratch and folds them through 128 E floats at its start,
// so a layout whose LayerNorms see more than ~87 k rows (E = 384) takes a larger scratch instead of failing.
static size_t train_scratch_floats(size_t ln_rows, size_t E) {
    return std::max(TRAIN_SCRATCH_FLOATS, ((ln_rows + LNB_ROWS - 1) / LNB_ROWS * 2 * E + 128 * E + 63) / 64 * 64);
}
struct TrainCtx {
    hipStream_t s;
    float* scratch;      // scratch_floats floats (train_scratch_floats)
    int ops = PARSEQ_F32;       // the operand mode of the products (parseq_model_set_train_precision): PARSEQ_F32 exact, PARSEQ_BF16 GEMM operands
                                // rounded to bf16, PARSEQ_BF16X3 split into bf16 (hi, lo) pairs; fp32 accumulate and everything else in all three
    size_t scratch_floats = TRAIN_SCRATCH_FLOATS;      // what of `scratch` the split-K partials / column sums may use (lin_bwd carves its padded copies off the end)
    bool bf16_ops() const { return ops == PARSEQ_BF16; }
    bool x3_ops() const { return ops == PARSEQ_BF16X3; }
};
static bool train_ops_ok(int ops) { return ops == PARSEQ_F32 || ops == PARSEQ_BF16 || ops == PARSEQ_BF16X3; }

static bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
constexpr int SPLIT_TARGET = 512;      // split-K: how many workgroups a product with few output tiles is cut into along the contraction

// A product C[M, N] = A B is described by its parts, each of which carries its element type:
// Operand: where an input matrix lives, its stride along the product's outer axis (m for A, n for B) and along the contraction, both in
// ELEMENTS of its own type, and whether that type is fp32 or bf16 — constructible from a typed pointer only, so bf16 bytes cannot reach a
// loader of floats by a cast at a call site.  bf16 operands are the SHADOWS of the bf16-operand mode (train_gemm.h SgemmArgs a16 / b16).
struct Operand {
    const void* p; long so, sk; bool bf16;
    Operand(const float* q, long outer, long k) : p(q), so(outer), sk(k), bf16(false) {}
    Operand(const bf16_t* q, long outer, long k) : p(q), so(outer), sk(k), bf16(true) {}
};
// An [M, N] tensor the epilogue writes (Out) or reads (In), dense rows: as fp32, as bf16, or both
template <typename F, typename H>
struct Dual {
    F* f32 = nullptr; H* b16 = nullptr;
    Dual() = default;
    Dual(F* p) : f32(p) {}
    Dual(H* q) : b16(q) {}
    Dual(F* p, H* q) : f32(p), b16(q) {}
    template <typename F2, typename H2> Dual(const Dual<F2, H2>& o) : f32(o.f32), b16(o.b16) {}      // an Out read back as an In
    explicit operator bool() const { return f32 || b16; }
};
using Out = Dual<float, bf16_t>;
using In = Dual<const float, const bf16_t>;
// The optional parts of a product: C (+)= alpha * A B + bias + R[m % rper], and what may ride on its epilogue
struct GemmOpts {
    const float* bias = nullptr;                          // [N]
    const float* R = nullptr; long ldr = 0; int rper = 0; // residual rows
    float alpha = 1.f; bool accumulate = false;
    float* asum = nullptr;       // [M] += row sums of A over k (the bias gradient riding on a dW product)
    In gelu_pre;                 // C is multiplied by gelu'(gelu_pre) (the GELU backward riding on a dX product)
    Out gelu_out;                // gelu(C) as a second output
};
// Which of the optional epilogues the kernel sgemm chose has folded into the product; the caller launches the others itself
struct GemmFolded { bool asum = false, gelu_pre = false, gelu_out = false; };

// The matrix-core loaders read 16-byte pieces along the contraction (4 floats, 8 bf16) or, of an operand contiguous along its outer axis
// (`outer` = M or N elements), whole groups of four
static bool mc_readable(const Operand& x, int outer) {
    return aligned16(x.p) && (x.sk == 1 ? x.so % (x.bf16 ? 8 : 4) == 0 : (x.so == 1 && x.sk % 4 == 0 && outer % 4 == 0));
}
// split-K: a product with few output tiles is cut along the contraction into `splits` workgroups per tile, k_chunk (whole stages of bk) each.
// The 64-deep kernels of the bf16 shadows ask for as many splits as the 32-deep ones do; k_chunk is then rounded up to whole stages of the
// kernel's own depth.  Where K / splits rounds to the same chunk at 32 and at 64 the shadow path is
// bit-identical to the fp32-in-memory one; elsewhere (K = 1472: 8 x 192 against 10 x 160) the two sum in a different order.
struct GemmPlan { int gm, gn, tiles, bk, splits, k_chunk; };
static GemmPlan gemm_plan(int M, int N, int K, int bk, size_t scratch_floats) {
    GemmPlan p; p.gm = (M + MG_BM - 1) / MG_BM; p.gn = (N + MG_BN - 1) / MG_BN; p.tiles = p.gm * p.gn; p.bk = bk;
    int splits = 1;
    if (p.tiles < 256) {
        splits = std::min((SPLIT_TARGET + p.tiles - 1) / p.tiles, K / (4 * std::min(bk, BG_BK)));
        splits = (int)std::min<size_t>((size_t)std::max(splits, 1), scratch_floats / ((size_t)M * N + (size_t)M));      // + the row-sum slots
        splits = std::max(splits, 1);
    }
    p.k_chunk = ((K + splits - 1) / splits + bk - 1) / bk * bk;
    p.splits = (K + p.k_chunk - 1) / p.k_chunk;
    return p;
}
// The matrix-core kernel of the bf16-operand mode for a product's operand types and contiguous axes (akf / bkf: contiguous along the
// contraction); all of them take a one-dimensional tile index (they order the tiles XCD-aware) and the split in grid z.
// whole: the four-workgroups-per-CU forms of the all-bf16 kernels; deep_t: both operands bf16, outer-contiguous, whole 64-deep stages
// Each entry carries its name in the route report (parseq_gemm_kernel; parseq_op_train_gemm hands it to the operator tests).
using BgemmKernel = void (*)(const SgemmArgs, int, float*, int, int);
struct BgemmChoice { BgemmKernel fn; int id; };
static BgemmChoice bgemm_kernel(bool a16, bool b16, bool akf, bool bkf, bool whole, bool deep_t) {
    if (a16 && akf) return {whole ? mfma_bgemm16_kernel<true> : mfma_bgemm16_kernel<false>, PARSEQ_GEMM_BOTH16_K};
    if (a16 && deep_t) return {whole ? mfma_bgemm16t_kernel<true> : mfma_bgemm16t_kernel<false>, PARSEQ_GEMM_BOTH16_T};
    if (a16) return {mfma_bgemm_kernel<false, false, true, true>, PARSEQ_GEMM_A16_NN};
    if (b16) return akf ? (bkf ? BgemmChoice{mfma_bgemm_kernel<true, true, true>, PARSEQ_GEMM_B16_KK} : BgemmChoice{mfma_bgemm_kernel<true, false, true>, PARSEQ_GEMM_B16_KN})
                        : (bkf ? BgemmChoice{mfma_bgemm_kernel<false, true, true>, PARSEQ_GEMM_B16_NK} : BgemmChoice{mfma_bgemm_kernel<false, false, true>, PARSEQ_GEMM_B16_NN});
    return akf ? (bkf ? BgemmChoice{mfma_bgemm_kernel<true, true>, PARSEQ_GEMM_BF16_KK} : BgemmChoice{mfma_bgemm_kernel<true, false>, PARSEQ_GEMM_BF16_KN})
               : (bkf ? BgemmChoice{mfma_bgemm_kernel<false, true>, PARSEQ_GEMM_BF16_NK} : BgemmChoice{mfma_bgemm_kernel<false, false>, PARSEQ_GEMM_BF16_NN});
}
// The split-bf16 kernel of the bf16x3 mode (fp32 operands in memory only): same arguments, same grid
static BgemmChoice x3gemm_kernel(bool akf, bool bkf) {
    return akf ? (bkf ? BgemmChoice{mfma_x3gemm_kernel<true, true>, PARSEQ_GEMM_X3_KK} : BgemmChoice{mfma_x3gemm_kernel<true, false>, PARSEQ_GEMM_X3_KN})
               : (bkf ? BgemmChoice{mfma_x3gemm_kernel<false, true>, PARSEQ_GEMM_X3_NK} : BgemmChoice{mfma_x3gemm_kernel<false, false>, PARSEQ_GEMM_X3_NN});
}
// Routes, first match wins.  The bf16x3 mode's split-bf16 kernel takes what the bf16-operand mode's fp32-in-memory kernels take and
// falls through to the fp32 routes otherwise.  The bf16-operand mode's matrix-core kernels: edge tiles allowed (the 95-class head, the 96-wide patch
// rows), every optional epilogue folded; a product with a bf16 part MUST take them — one that cannot is an error, never a silent fp32
// read of bf16 data.  The fp32 matrix-core kernel: whole 128 x 128 tiles and 16-deep stages.  The VALU kernel: everything else.
static int sgemm(const TrainCtx& cx, const Operand& A, const Operand& B, const Out& C, int M, int N, int K, const GemmOpts& o = GemmOpts(),
                 GemmFolded* folded = nullptr, parseq_gemm_route* route = nullptr) {
    hipStream_t s = cx.s;
    if (M <= 0 || N <= 0 || K <= 0) return fail(PARSEQ_E_INVALID, "sgemm: bad shape %d x %d x %d", M, N, K);
    const bool shadow = A.bf16 || B.bf16 || C.b16 || o.gelu_out.b16 || o.gelu_pre.b16;
    if (shadow && (!cx.bf16_ops() || !cx.scratch || M < 16 || N < 16)) return fail(PARSEQ_E_STATE, "sgemm: bf16 shadow operands outside the bf16-operand mode");
    if (!C) return fail(PARSEQ_E_INVALID, "sgemm: no output");
    const bool akf = A.sk == 1, bkf = B.sk == 1, readable = mc_readable(A, M) && mc_readable(B, N);
    const bool both = A.bf16 && B.bf16 && akf && bkf;                     // the 64-deep kernel
    const bool both_t = A.bf16 && B.bf16 && A.so == 1 && B.so == 1;       // dW with a bf16 dY: both operands outer-contiguous
    const bool deep_t = both_t && K % BH_BK == 0;                         // ... at 64 rows of the contraction per stage
    const int bk16 = (both || deep_t) ? BH_BK : BG_BK;
    if (shadow && (!readable || K % bk16 != 0 || (A.bf16 && !both && !both_t)))
        return fail(PARSEQ_E_INVALID, "sgemm: shadow operands of a %d x %d x %d product are not laid out for the matrix-core kernels", M, N, K);
    if (shadow && o.asum && both) return fail(PARSEQ_E_INVALID, "sgemm: row sums of a bf16 shadow");
    const bool mc16 = K % BG_BK == 0 && readable && cx.scratch && M >= 16 && N >= 16;      // what the fp32-in-memory bf16 kernels take
    const bool x3 = cx.x3_ops() && mc16;
    const bool bf16 = shadow || (cx.bf16_ops() && mc16);
    const bool mfma32 = !bf16 && !x3 && M % MG_BM == 0 && N % MG_BN == 0 && K % MG_BK == 0 && readable && cx.scratch;

    SgemmArgs a{};      // the one place where a typed operand becomes the kernels' pointer + flag
    a.A = static_cast<const float*>(A.p); a.sam = A.so; a.sak = A.sk; a.a16 = A.bf16;
    a.B = static_cast<const float*>(B.p); a.sbk = B.sk; a.sbn = B.so; a.b16 = B.bf16;
    a.bias = o.bias; a.R = o.R; a.ldr = o.ldr; a.rper = o.rper > 0 ? o.rper : 1;
    a.C = C.f32; a.c16 = C.b16; a.ldc = N; a.M = M; a.N = N; a.K = K; a.alpha = o.alpha; a.accumulate = o.accumulate ? 1 : 0;
    if (bf16 || x3) { a.asum = o.asum; a.gelu_pre = o.gelu_pre.f32; a.gelu_pre16 = o.gelu_pre.b16; a.gelu_out = o.gelu_out.f32; a.gelu_out16 = o.gelu_out.b16; }
    if (folded) folded->asum = folded->gelu_pre = folded->gelu_out = bf16 || x3;
    if (!bf16 && !x3 && !mfma32) {
        if (route) { route->kernel = PARSEQ_GEMM_VALU; route->whole = 0; route->splits = 1; route->k_chunk = K; }
        return launch(sgemm_kernel, dim3((N + SG_BN - 1) / SG_BN, (M + SG_BM - 1) / SG_BM), dim3(256), 0, s, a);
    }
    const GemmPlan p = gemm_plan(M, N, K, (bf16 || x3) ? bk16 : MG_BK, cx.scratch_floats);
    if (x3) {
        const BgemmChoice k = x3gemm_kernel(akf, bkf);
        if (route) { route->kernel = k.id; route->whole = 0; route->splits = p.splits; route->k_chunk = p.k_chunk; }
        hipLaunchKernelGGL(k.fn, dim3((unsigned)p.tiles, 1, p.splits), dim3(256), 0, s, a, p.k_chunk, cx.scratch, p.gn, p.gm);
        HIPCHK(hipGetLastError());
    } else if (bf16) {
        // whole 128 x 128 tiles (every product of the PARSeq-S / ViTSTR encoders); the buffer loads' 32-bit byte offsets cover both operands
        // with room to spare at any batch that fits the workspace
        const bool whole = M % MG_BM == 0 && N % MG_BN == 0 &&
                           (size_t)M * (size_t)std::max(A.so, A.sk) < ((size_t)1 << 29) && (size_t)N * (size_t)std::max(B.so, B.sk) < ((size_t)1 << 29) &&
                           (size_t)K * (size_t)std::max(A.sk, B.sk) < ((size_t)1 << 29);
        const BgemmChoice k = bgemm_kernel(A.bf16, B.bf16, akf, bkf, whole, deep_t);
        if (route) { route->kernel = k.id; route->whole = (whole && (k.id == PARSEQ_GEMM_BOTH16_K || k.id == PARSEQ_GEMM_BOTH16_T)) ? 1 : 0; route->splits = p.splits; route->k_chunk = p.k_chunk; }
        hipLaunchKernelGGL(k.fn, dim3((unsigned)p.tiles, 1, p.splits), dim3(256), 0, s, a, p.k_chunk, cx.scratch, p.gn, p.gm);
        HIPCHK(hipGetLastError());
    } else {
        if (route) { route->kernel = PARSEQ_GEMM_MFMA_F32; route->whole = 0; route->splits = p.splits; route->k_chunk = p.k_chunk; }
        CHK(launch(mfma_sgemm_kernel, dim3(p.gn, p.gm, p.splits), dim3(256), 0, s, a, p.k_chunk, cx.scratch));
    }
    if (p.splits > 1)
        CHK(launch(splitk_reduce_kernel, dim3((unsigned)(((size_t)M * N + (a.asum ? (size_t)M : 0) + 255) / 256)), dim3(256), 0, s, a, cx.scratch, p.splits));
    return 0;
}
static int colsum(const TrainCtx& cx, const float* A, long lda, int M, int N, float* out, bool accumulate) {
    hipStream_t s = cx.s;
    constexpr int CHUNKS = 64;
    if (M >= 2048 && cx.scratch && (size_t)CHUNKS * N <= cx.scratch_floats) {
        const int rows_per = (M + CHUNKS - 1) / CHUNKS;
        CHK(launch(colsum_kernel, dim3((N + 63) / 64, CHUNKS), dim3(1024), 0, s, A, lda, M, N, cx.scratch, 0, rows_per, (float*)nullptr, 0));
        return launch(colsum_kernel, dim3((N + 63) / 64, 1), dim3(1024), 0, s, cx.scratch, (long)N, CHUNKS, N, out, accumulate ? 1 : 0, CHUNKS, (float*)nullptr, 0);
    }
    return launch(colsum_kernel, dim3((N + 63) / 64, 1), dim3(1024), 0, s, A, lda, M, N, out, accumulate ? 1 : 0, M, (float*)nullptr, 0);
}
// A dense row-major [rows, ld] tensor as a product's operand, in the type it is stored in (the bf16 shadow where there is one)
static Operand rows_operand(In t, long ld) { return t.b16 ? Operand(t.b16, ld, 1) : Operand(t.f32, ld, 1); }
// y[M, N] = x[M, K] W[N, K]^T + bias + R[m % rper], x and W both fp32 or both bf16 shadows (x16 [M, K], W16 [N, K]; y as fp32, bf16 or both)
// gelu_out (optional, [M, N]): gelu(y) as a second output — from the product's epilogue on the bf16 matrix-core kernels, by gelu_fwd_kernel otherwise
static int lin_fwd(const TrainCtx& cx, In x, In W, const float* bias, const float* R, int rper, Out y, int M, int N, int K, Out gelu_out = Out()) {
    GemmOpts g; g.bias = bias; g.R = R; g.ldr = N; g.rper = rper; g.gelu_out = gelu_out;
    GemmFolded f;
    CHK(sgemm(cx, rows_operand(x, K), rows_operand(W, K), y, M, N, K, g, &f));
    if (gelu_out && !f.gelu_out)
        CHK(launch(gelu_fwd_kernel, dim3((unsigned)(((size_t)M * N + 1023) / 1024)), dim3(256), 0, cx.s, y.f32, gelu_out.f32, (size_t)M * N));
    return 0;
}
static int gelu_bwd(const TrainCtx& cx, const float* pre, float* d, size_t n) {      // d *= gelu'(pre)
    return launch(gelu_bwd_kernel, dim3((unsigned)((n + 1023) / 1024)), dim3(256), 0, cx.s, pre, d, d, n);
}
// dW[N, K] += dy[M, N]^T x[M, K];  db[N] += column sums of dy;  dx[M, K] = dy W   (dx may be null)
// dx_gelu_pre (optional, [M, K]): dx is additionally multiplied by gelu'(dx_gelu_pre) — the GELU backward of the layer below, folded
// into the dX product's epilogue when it takes the bf16 matrix-core kernel and run as gelu_bwd_kernel otherwise
static int lin_bwd(const TrainCtx& cx, const float* x, const float* W, const float* dy, float* dW, float* db, float* dx, int M, int N, int K,
                   const float* dx_gelu_pre = nullptr) {
    // bf16-operand mode, output width not a multiple of 4 (the 95-class head): rows of dy are not 16-byte aligned and N is no multiple of
    // the 32-deep k-step, so both products would fall to the VALU kernel (10 % of the step).  Instead dy and W are copied into zero-padded
    // [M, Np] / [Np, K] buffers (Np = N rounded up to 32) carved off the end of the scratch, both products run on the matrix cores, and the
    // first N rows of the padded dW are added to the gradient.
    const int Np = (N + 31) / 32 * 32;
    const size_t reserve = (size_t)M * Np + 2 * (size_t)Np * K;
    if ((cx.bf16_ops() || cx.x3_ops()) && N % 4 != 0 && cx.scratch && M % 4 == 0 && K % 4 == 0 && reserve + ((size_t)4 << 20) <= cx.scratch_floats) {
        hipStream_t s = cx.s;
        TrainCtx c2 = cx; c2.scratch_floats = cx.scratch_floats - reserve;
        float* dyp = cx.scratch + c2.scratch_floats; float* Wp = dyp + (size_t)M * Np; float* dWp = Wp + (size_t)Np * K;
        CHK(launch(pad_copy_kernel, dim3((unsigned)(((size_t)M * Np + 255) / 256)), dim3(256), 0, s, dy, M, N, dyp, M, Np));
        CHK(launch(pad_copy_kernel, dim3((unsigned)(((size_t)Np * K + 255) / 256)), dim3(256), 0, s, W, N, K, Wp, Np, K));
        CHK(sgemm(c2, Operand(dyp, 1, Np), Operand(x, 1, K), dWp, Np, K, M));
        CHK(launch(add_into_kernel, dim3((unsigned)(((size_t)N * K + 255) / 256)), dim3(256), 0, s, dWp, dW, (size_t)N * K));
        CHK(colsum(c2, dy, N, M, N, db, true));
        if (dx) CHK(sgemm(c2, Operand(dyp, Np, 1), Operand(Wp, 1, K), dx, M, K, Np));
        if (dx && dx_gelu_pre) CHK(gelu_bwd(cx, dx_gelu_pre, dx, (size_t)M * K));
        return 0;
    }
    // dW += dY^T X; the bias gradient (column sums of dY = row sums of the product's A operand) rides on it in the bf16-operand mode
    GemmOpts gw; gw.accumulate = true; gw.asum = db;
    GemmFolded f;
    CHK(sgemm(cx, Operand(dy, 1, N), Operand(x, 1, K), dW, N, K, M, gw, &f));
    if (!f.asum) CHK(colsum(cx, dy, N, M, N, db, true));
    if (dx) {
        GemmOpts gx; gx.gelu_pre = dx_gelu_pre;
        CHK(sgemm(cx, Operand(dy, N, 1), Operand(W, 1, K), dx, M, K, N, gx, &f));
        if (dx_gelu_pre && !f.gelu_pre) CHK(gelu_bwd(cx, dx_gelu_pre, dx, (size_t)M * K));
    }
    return 0;
}
// The two backward products on bf16 SHADOW operands (encoder, bf16-operand mode; train_gemm.h SgemmArgs): x16 [M, K] and the transposed weight
// shadow Wt16 [K, N] are bfloat16 in memory; dy is read as fp32 where it exists (the bias gradient is then summed from the unrounded values) and
// through its shadow dy16 otherwise — the dX product prefers the shadow; dx16: the result again as bf16 for the next product; dx_gelu_pre16: the
// pre-activation as bf16.  Bit-identical to lin_bwd on the fp32 copies: the rounding moved, nothing else.
static int lin_bwd16_dw(const TrainCtx& cx, const bf16_t* x16, In dy, float* dW, float* db, int M, int N, int K) {
    if (!dy) return fail(PARSEQ_E_INVALID, "lin_bwd16: no gradient");
    GemmOpts g; g.accumulate = true; g.asum = db;
    return sgemm(cx, dy.f32 ? Operand(dy.f32, 1, N) : Operand(dy.b16, 1, N), Operand(x16, 1, K), dW, N, K, M, g);
}
static int lin_bwd16_dx(const TrainCtx& cx, const bf16_t* Wt16, In dy, Out dx, int M, int N, int K, In dx_gelu_pre = In()) {
    if (!dy) return fail(PARSEQ_E_INVALID, "lin_bwd16: no gradient");
    if (!dx) return 0;
    GemmOpts g; g.gelu_pre = dx_gelu_pre;
    return sgemm(cx, rows_operand(dy, N), Operand(Wt16, N, 1), dx, M, K, N, g);
}
// dx = add + LayerNorm backward; dgamma += column sums of dy * xhat; dbeta += column sums of dy.
// dx16 (optional): dx again as bf16, the operand shadow of the dX product that follows.
static int ln_bwd(const TrainCtx& cx, const float* x, const float* gamma, const float* dy, const float* add, float* dx, float* dgamma, float* dbeta,
                  int rows, int E, float eps, bf16_t* dx16 = nullptr) {
    hipStream_t s = cx.s;
    if (E > 768) return fail(PARSEQ_E_INVALID, "layernorm backward: E=%d > 768", E);
    // per-chunk partial sums of dy * xhat and dy land in the scratch ([chunks][2E]); two small column sums fold them
    const int chunks = (rows + LNB_ROWS - 1) / LNB_ROWS;
    if (!cx.scratch || (size_t)chunks * 2 * E + (size_t)64 * E > cx.scratch_floats) return fail(PARSEQ_E_INVALID, "layernorm backward: %d rows do not fit the scratch", rows);
    float* part = cx.scratch + (cx.scratch_floats - (size_t)chunks * 2 * E);      // the END of the scratch: colsum's own partials use its start
    TrainCtx c2 = cx; c2.scratch_floats = cx.scratch_floats - (size_t)chunks * 2 * E;
    CHK(launch(ln_bwd_kernel, dim3(chunks), dim3(256), 0, s, x, gamma, dy, add, dx, part, rows, E, eps, dx16));
    // both column sums in one pair of launches: [chunks][2E] -> 64 row chunks -> dgamma (columns < E) and dbeta (the rest)
    constexpr int CHUNKS = 64;
    if (chunks >= 2048 && (size_t)CHUNKS * 2 * E <= c2.scratch_floats) {
        const int rows_per = (chunks + CHUNKS - 1) / CHUNKS;
        CHK(launch(colsum_kernel, dim3((2 * E + 63) / 64, CHUNKS), dim3(1024), 0, s, part, 2L * E, chunks, 2 * E, c2.scratch, 0, rows_per, (float*)nullptr, 0));
        return launch(colsum_kernel, dim3((2 * E + 63) / 64, 1), dim3(1024), 0, s, c2.scratch, 2L * E, CHUNKS, 2 * E, dgamma, 1, CHUNKS, dbeta, E);
    }
    return launch(colsum_kernel, dim3((2 * E + 63) / 64, 1), dim3(1024), 0, s, part, 2L * E, chunks, 2 * E, dgamma, 1, chunks, dbeta, E);
}
// ---- attention -------------------------------------------------------------------------------------------------------------------------
// Which kernel a training attention call runs and how it is launched.  Routes, first match wins: the two bf16-operand kernels (decoder
// shapes, the 128-token encoder), the fp32 matrix-core kernel (head width 64, up to 128 keys), the key-streaming kernels past 128
// tokens (train_attn_wide.h), the VALU kernels; TA_NONE: no kernel.
enum TrainAttnRoute { TA_DEC_BF16, TA_ENC_BF16, TA_MFMA, TA_WIDE, TA_HD32, TA_HD64, TA_NONE };
struct TrainAttnPlan { TrainAttnRoute route; dim3 grid; int threads; size_t lds; };
constexpr size_t TA_LDS_CAP = 150 * 1024;      // what the fp32 kernels may be given of a CU's 160 KiB
// the shapes train_attn_dec_bf16_kernel takes (bf16-operand mode, head width 32, <= TD_Q queries, <= TD_K keys); train_dec_route asks
// the same of the cross-attention before there are operands to plan with
static bool train_attn_dec_bf16_shape(bool bf16_ops, int hd, int Lq, int Lk) { return bf16_ops && hd == TD_HD && Lq <= TD_Q && Lk <= TD_K; }
// ... and the instantiation by key tiles: up to 128 keys, or for the self-attention the 32-key one (a quarter of the LDS, a third of the registers)
static int train_attn_dec_kt(const TrainAttnArgs& a) { return a.Lk > 32 ? 8 : 2; }
// The plan of one call: under each route's match stands everything its kernel asks of the arguments — a field the kernel does not read
// is refused, not ignored (lse / dsum excepted: the slots of the key-streaming route, which the others leave untouched) — and its
// capacity, then its grid and LDS bytes (from the function beside the kernel).  out->route is written even when the call is refused.
static int train_attn_plan(const TrainCtx& cx, const TrainAttnArgs& a, int hd, int B, bool backward, TrainAttnPlan* out) {
    const bool rows4 = a.ldq % 4 == 0 && a.ldkv % 4 == 0 && a.ldo % 4 == 0 && (!backward || (a.lddq % 4 == 0 && a.lddkv % 4 == 0 && aligned16(a.dk) && aligned16(a.dv)));
    const bool plain = !a.qmask && !a.kmask && !a.drop.thresh;      // no masks, no dropout
    // what a route answers whose kernel walks one pass per launch / writes fp32 only / keeps all keys resident
    auto no_pass_loop = [&] { return a.pass_loop > 1 ? fail(PARSEQ_E_INVALID, "training attention: pass_loop is train_attn_dec_bf16_kernel's alone") : 0; };
    auto one_pass = [&] {
        CHK(no_pass_loop());
        return a.pass_B ? fail(PARSEQ_E_INVALID, "training attention: several passes per launch only at the decoder's head width") : 0;
    };
    auto fp32_out = [&] { return (a.o16 || a.dq16 || a.dk16 || a.dv16) ? fail(PARSEQ_E_INVALID, "training attention: a bf16 output is only written by the encoder-shaped bf16 kernel") : 0; };
    auto fits = [&](size_t lds, bool regs) { return (lds > TA_LDS_CAP || !regs) ? fail(PARSEQ_E_INVALID, "training attention: %d keys of width %d do not fit (LDS %zu bytes)", a.Lk, hd, lds) : 0; };
    TrainAttnPlan& p = *out;
    p = TrainAttnPlan{TA_NONE, dim3((unsigned)(B * a.H)), 256, 0};      // one workgroup of four waves per (image, head) unless the route says otherwise
    if (train_attn_dec_bf16_shape(cx.bf16_ops(), hd, a.Lq, a.Lk) && rows4 && a.q_bstride % 4 == 0) {
        // masks, dropout, shared queries, pass_B with or without kv_shared; pass_loop: one workgroup per (image, head) walks the passes
        p.route = TA_DEC_BF16;
        if (a.pass_loop > 1 && !(a.pass_B > 0 && a.kv_shared && B == a.pass_B * a.pass_loop))
            return fail(PARSEQ_E_INVALID, "training attention: pass_loop needs pass_B, shared K / V and a batch of pass_B * pass_loop images");
        CHK(fp32_out());
        p.grid = dim3((unsigned)((a.pass_loop > 1 ? a.pass_B : B) * a.H)); p.threads = 128; p.lds = train_attn_dec_lds(backward, train_attn_dec_kt(a));
    } else if (cx.bf16_ops() && hd == TB_HD && a.Lq == TB_N && a.Lk == TB_N && plain && a.q_bstride == (long)a.Lq * a.ldq && rows4) {
        // per-image queries; o16 / dq16 / dk16 / dv16 in place of the fp32 outputs, dk16 and dv16 together and never accumulated into
        p.route = TA_ENC_BF16;
        CHK(one_pass());
        if (!a.dk16 != !a.dv16 || (a.dk16 && a.kv_accumulate)) return fail(PARSEQ_E_INVALID, "training attention: bf16 dK / dV come as a pair and are stored, not accumulated");
        p.lds = train_attn_bf16_lds(backward);
    } else if (hd == TM_HD && a.Lq % TM_QB == 0 && a.Lk % 16 == 0 && a.Lk <= TM_K && plain) {
        // shared or per-image queries
        p.route = TA_MFMA;
        CHK(one_pass()); CHK(fp32_out());
        p.lds = train_attn_mfma_lds(a.Lk, backward);
        CHK(fits(p.lds, true));
    } else if (hd == TW_HD && a.Lk > 128 && a.Lk <= TW_MAXN && a.Lq == a.Lk && plain && !a.pass_B && !a.pass_loop && a.q_bstride == (long)a.Lq * a.ldq) {
        // per-image queries, one pass; the shapes no resident kernel takes (train_attn_kernel<*, 64> holds at most 128 keys)
        p.route = TA_WIDE;
        CHK(fp32_out());
        if (!a.lse || (backward && !a.dsum)) return fail(PARSEQ_E_INVALID, "training attention over %d tokens: no log-sum-exp / row-sum slot", a.Lk);
        bool ok = a.ldq % 4 == 0 && a.ldkv % 4 == 0 && a.ldo % 4 == 0 && a.q_bstride % 4 == 0 && aligned16(a.q) && aligned16(a.k) && aligned16(a.v) && aligned16(a.o);
        if (backward) ok = ok && a.d_o && a.dq && a.dk && a.dv && aligned16(a.d_o);
        if (!ok) return fail(PARSEQ_E_INVALID, "training attention over %d tokens: operands not laid out in 16-byte rows", a.Lk);
        p.grid = dim3((unsigned)((a.Lk + TW_BLK - 1) / TW_BLK), (unsigned)(B * a.H));
    } else if (hd == 32 || hd == 64) {
        // any strides, masks, dropout; pass_B with or without kv_shared at the decoder's head width
        p.route = hd == 32 ? TA_HD32 : TA_HD64;
        CHK(hd == TD_HD ? no_pass_loop() : one_pass()); CHK(fp32_out());
        p.lds = train_attn_lds_floats(a.Lq, a.Lk, hd, backward) * sizeof(float);
        CHK(fits(p.lds, (size_t)a.Lk * hd <= (size_t)TA_NACC * 256));
    } else return fail(PARSEQ_E_INVALID, "training attention: head width %d not in {32, 64}", hd);
    return 0;
}
// One launch of a pair of kernels, forward or backward, both allowed `cap_f` / `cap_b` bytes of dynamic LDS once per device (one LdsAttr
// pair per pair of kernels): the one place that raises the attribute
using AttnKernel = void (*)(const TrainAttnArgs);
template <AttnKernel FWD, AttnKernel BWD>
static int attn_launch(const TrainCtx& cx, const TrainAttnArgs& a, bool backward, const TrainAttnPlan& p, size_t cap_f, size_t cap_b) {
    static LdsAttr attr_f, attr_b;
    HIPCHK(attr_f.ensure(reinterpret_cast<const void*>(FWD), cap_f));
    HIPCHK(attr_b.ensure(reinterpret_cast<const void*>(BWD), cap_b));
    hipLaunchKernelGGL(backward ? BWD : FWD, p.grid, dim3(p.threads), p.lds, cx.s, a);
    HIPCHK(hipGetLastError());
    return 0;
}
template <int KT>
static int attn_launch_dec(const TrainCtx& cx, const TrainAttnArgs& a, bool backward, const TrainAttnPlan& p) {
    return attn_launch<train_attn_dec_bf16_kernel<false, KT>, train_attn_dec_bf16_kernel<true, KT>>(cx, a, backward, p, train_attn_dec_lds(false, KT), train_attn_dec_lds(true, KT));
}
// Plan, then launch; `took`: the route, also of a call that was refused
static int train_attn(const TrainCtx& cx, const TrainAttnArgs& a, int B, bool backward, int hd, TrainAttnRoute* took = nullptr) {
    TrainAttnPlan p;
    const int rc = train_attn_plan(cx, a, hd, B, backward, &p);
    if (took) *took = p.route;
    CHK(rc);
    switch (p.route) {
        case TA_DEC_BF16: return train_attn_dec_kt(a) == 8 ? attn_launch_dec<8>(cx, a, backward, p) : attn_launch_dec<2>(cx, a, backward, p);
        case TA_ENC_BF16: return attn_launch<train_attn_bf16_kernel<false>, train_attn_bf16_kernel<true>>(cx, a, backward, p, train_attn_bf16_lds(false), train_attn_bf16_lds(true));
        case TA_MFMA: return attn_launch<train_attn_mfma_kernel<false>, train_attn_mfma_kernel<true>>(cx, a, backward, p, TA_LDS_CAP, TA_LDS_CAP);
        case TA_HD32: return attn_launch<train_attn_kernel<false, 32>, train_attn_kernel<true, 32>>(cx, a, backward, p, TA_LDS_CAP, TA_LDS_CAP);
        case TA_HD64: return attn_launch<train_attn_kernel<false, 64>, train_attn_kernel<true, 64>>(cx, a, backward, p, TA_LDS_CAP, TA_LDS_CAP);
        default: break;      // TA_WIDE: static LDS, and the backward is two launches (dQ writes the row sums that dK / dV read)
    }
    if (!backward) return launch(train_attn_wide_fwd_kernel, p.grid, dim3(p.threads), 0, cx.s, a);
    CHK(launch(train_attn_wide_dq_kernel, p.grid, dim3(p.threads), 0, cx.s, a));
    return launch(train_attn_wide_dkv_kernel, p.grid, dim3(p.threads), 0, cx.s, a);
}

// The dropout of a step as its kernels take it: keep an element iff its hash >= dropout_p * 2^32, kept elements times 1 / (1 - dropout_p)
static DropSpec drop_spec(float dropout_p, uint64_t seed) {
    DropSpec drop{(unsigned)(seed & 0xFFFFFFFFull), (unsigned)(seed >> 32), 0u, 1.0f};
    if (dropout_p > 0.f) { drop.thresh = (unsigned)((double)dropout_p * 4294967296.0); drop.scale = 1.0f / (1.0f - dropout_p); }
    return drop;
}
static bool dropout_p_ok(float dropout_p) { return dropout_p >= 0.f && dropout_p < 1.f; }

// One call of train_attn() from a descriptor (the kernels' unit test, tests/test_train_attn.py): the descriptor is TrainAttnArgs field
// by field plus what the step takes from its context (head width, operand mode, dropout as probability and seed).
static_assert((int)PARSEQ_TRAIN_ATTN_DEC_BF16 == TA_DEC_BF16 && (int)PARSEQ_TRAIN_ATTN_ENC_BF16 == TA_ENC_BF16 && (int)PARSEQ_TRAIN_ATTN_MFMA == TA_MFMA &&
              (int)PARSEQ_TRAIN_ATTN_WIDE == TA_WIDE && (int)PARSEQ_TRAIN_ATTN_HD32 == TA_HD32 && (int)PARSEQ_TRAIN_ATTN_HD64 == TA_HD64 &&
              (int)PARSEQ_TRAIN_ATTN_NONE == TA_NONE, "the public route enum restates TrainAttnRoute");
extern "C" int parseq_op_train_attention_desc(const parseq_train_attn_desc* d, int batch, int backward, int32_t* route, void* stream) {
    if (route) *route = TA_NONE;
    CHK(check_arch());
    if (!d || !d->q || !d->k || !d->v || batch <= 0 || d->Lq <= 0 || d->Lk <= 0 || d->H <= 0 || d->pass_B < 0 || d->pass_loop < 0 ||
        (backward ? (!d->d_o || !(d->dq || d->dq16) || !((d->dk && d->dv) || d->dk16 || d->dv16)) : !(d->o || d->o16)))
        return fail(PARSEQ_E_INVALID, "bad argument");
    if (!train_ops_ok(d->bf16_ops)) return fail(PARSEQ_E_INVALID, "operand mode %d", d->bf16_ops);
    if (!dropout_p_ok(d->dropout_p)) return fail(PARSEQ_E_INVALID, "dropout_p %g outside [0, 1)", d->dropout_p);
    TrainAttnArgs a{};
    a.q = d->q; a.q_bstride = (long)d->q_bstride; a.ldq = d->ldq; a.k = d->k; a.v = d->v; a.ldkv = d->ldkv;
    a.qmask = d->qmask; a.kmask = d->kmask; a.ldkm = d->ldkm;
    a.o = d->o; a.ldo = d->ldo; a.o16 = static_cast<bf16_t*>(d->o16);
    a.dq16 = static_cast<bf16_t*>(d->dq16); a.dk16 = static_cast<bf16_t*>(d->dk16); a.dv16 = static_cast<bf16_t*>(d->dv16);
    a.d_o = d->d_o; a.dq = d->dq; a.lddq = d->lddq; a.dk = d->dk; a.dv = d->dv; a.lddkv = d->lddkv; a.kv_accumulate = d->kv_accumulate;
    a.Lq = d->Lq; a.Lk = d->Lk; a.H = d->H; a.scale = d->scale; a.drop = drop_spec(d->dropout_p, d->seed); a.drop_site = d->drop_site;
    a.pass_B = d->pass_B; a.qmask_pstride = (long)d->qmask_pstride; a.site_pstride = d->site_pstride; a.kv_shared = d->kv_shared;
    a.pass_loop = d->pass_loop; a.lse = d->lse; a.dsum = d->dsum;
    const TrainCtx cx{(hipStream_t)stream, nullptr, d->bf16_ops, 0};
    TrainAttnRoute took = TA_NONE;
    const int rc = train_attn(cx, a, batch, backward != 0, d->head_dim, &took);
    if (route) *route = (int32_t)took;
    return rc;
}

// The training step's encoder attention on its own: the self-attention of `tokens` tokens, `heads` heads of 64, q | k | v interleaved in
// qkv [batch * tokens, 3 E] (E = 64 heads), o [batch * tokens, E], fp32, exact products.  A caller of the descriptor hook.
extern "C" int parseq_op_train_attention(const float* qkv, float* o, float* lse, const float* d_o, float* dqkv, float* dsum, int batch, int tokens,
                                         int heads, int backward, int* route, void* stream) {
    CHK(check_arch());
    if (!qkv || !o || batch <= 0 || tokens <= 0 || heads <= 0 || (backward && (!d_o || !dqkv))) return fail(PARSEQ_E_INVALID, "bad argument");
    const int E = heads * TW_HD;
    parseq_train_attn_desc d{};
    d.q = qkv; d.q_bstride = (int64_t)tokens * 3 * E; d.ldq = 3 * E; d.k = qkv + E; d.v = qkv + 2 * E; d.ldkv = 3 * E;
    d.o = o; d.ldo = E; d.d_o = d_o; d.dq = dqkv; d.lddq = 3 * E; d.dk = dqkv ? dqkv + E : nullptr; d.dv = dqkv ? dqkv + 2 * E : nullptr;
    d.lddkv = 3 * E; d.Lq = tokens; d.Lk = tokens; d.H = heads; d.scale = 1.0f / sqrtf((float)TW_HD); d.lse = lse; d.dsum = dsum;
    d.head_dim = TW_HD; d.bf16_ops = PARSEQ_F32;
    int32_t took = TA_NONE;
    const int rc = parseq_op_train_attention_desc(&d, batch, backward, &took, stream);
    if (route) *route = took == TA_WIDE ? 1 : 0;
    return rc;
}


// The step's products and row kernels one operator at a time (the kernels' unit tests): each hook builds the step's context from its
// arguments and calls the function the step calls.
static bool gemm_dtype_ok(int dtype) { return dtype == PARSEQ_F32 || dtype == PARSEQ_BF16; }
static Operand gemm_operand(const parseq_gemm_operand& x) {
    return x.dtype == PARSEQ_BF16 ? Operand(static_cast<const bf16_t*>(x.data), (long)x.outer_stride, (long)x.k_stride)
                                  : Operand(static_cast<const float*>(x.data), (long)x.outer_stride, (long)x.k_stride);
}
extern "C" int parseq_op_train_gemm(const parseq_train_gemm_desc* d, parseq_gemm_route* route, void* stream) {
    if (route) *route = parseq_gemm_route{PARSEQ_GEMM_NONE, 0, 0, 0, 0, 0, 0};
    CHK(check_arch());
    if (!d || !d->A.data || !d->B.data || !gemm_dtype_ok(d->A.dtype) || !gemm_dtype_ok(d->B.dtype)) return fail(PARSEQ_E_INVALID, "bad argument");
    if (!train_ops_ok(d->bf16_ops)) return fail(PARSEQ_E_INVALID, "operand mode %d", d->bf16_ops);
    const TrainCtx cx{(hipStream_t)stream, d->scratch, d->bf16_ops, d->scratch_floats};
    GemmOpts g;
    g.bias = d->bias; g.R = d->R; g.ldr = (long)d->ldr; g.rper = d->rper; g.alpha = d->alpha; g.accumulate = d->accumulate != 0; g.asum = d->asum;
    g.gelu_pre = In(d->gelu_pre, static_cast<const bf16_t*>(d->gelu_pre16));
    g.gelu_out = Out(d->gelu_out, static_cast<bf16_t*>(d->gelu_out16));
    GemmFolded f;
    parseq_gemm_route r{PARSEQ_GEMM_NONE, 0, 0, 0, 0, 0, 0};
    const int rc = sgemm(cx, gemm_operand(d->A), gemm_operand(d->B), Out(d->C, static_cast<bf16_t*>(d->c16)), d->M, d->N, d->K, g, &f, &r);
    if (rc == 0) { r.folded_asum = f.asum; r.folded_gelu_pre = f.gelu_pre; r.folded_gelu_out = f.gelu_out; }
    if (route && rc == 0) *route = r;
    return rc;
}
extern "C" int parseq_op_train_linear(const float* x, const float* W, const float* bias, const float* R, int rper, float* y, float* gelu_out,
                                      const float* dy, float* dW, float* db, float* dx, const float* dx_gelu_pre, int M, int N, int K, int backward,
                                      int bf16_ops, float* scratch, size_t scratch_floats, void* stream) {
    CHK(check_arch());
    if (!x || !W || M <= 0 || N <= 0 || K <= 0 || (backward ? (!dy || !dW || !db) : !y)) return fail(PARSEQ_E_INVALID, "bad argument");
    if (!train_ops_ok(bf16_ops)) return fail(PARSEQ_E_INVALID, "operand mode %d", bf16_ops);
    const TrainCtx cx{(hipStream_t)stream, scratch, bf16_ops, scratch_floats};
    if (backward) return lin_bwd(cx, x, W, dy, dW, db, dx, M, N, K, dx_gelu_pre);
    return lin_fwd(cx, x, W, bias, R, rper, y, M, N, K, Out(gelu_out));
}

// ---- what the step's entry points share ---------------------------------------------------------------------------------------------
// Workspace layouts hand out their buffers in order, each on a 64-float boundary
struct Take {
    size_t off = 0;
    size_t operator()(size_t n) { const size_t at = off; off += (n + 63) / 64 * 64; return at; }
};
static int require_params_set(const parseq_model* m) {
    for (const ParamSpec& ps : m->params) if (!ps.set) return fail(PARSEQ_E_STATE, "parameter %s was never set", ps.key.c_str());
    return 0;
}
// A parameter resolved once per call (on the stack: the caller's gradient buffer may change between calls): where it lies in the master
// (`at`, in floats) and its slot in the flat gradient buffer, which is laid out like the master (null where the call writes no gradients)
struct ParamRef { const float* p; float* g; size_t at; };
static ParamRef param_ref(const parseq_model* m, const std::string& key, float* grads) {
    const size_t at = m->params[m->index.at(key)].offset;
    return ParamRef{m->master + at, grads ? grads + at : nullptr, at};
}
template <int N> struct ParamSet {      // indexed by the enum of its key table: W(k) the parameter, W.g(k) its gradient
    ParamRef v[N];
    const float* operator()(int k) const { return v[k].p; }
    float* g(int k) const { return v[k].g; }
};
// Cross-entropy of `passes` passes of M rows each over C classes (ignore_index = pad): each pass's own mean into loss[q] (system.py:189-190;
// rows summed in the order its own launch would) with its kept targets in count[q], then logits <- d loss / d logits at 1 / total_targets per row
static int ce_loss_and_grad(hipStream_t s, float* logits, const int32_t* tgt, int passes, int M, int C, int pad, float* row_loss, float* loss, int* count,
                            int total_targets) {
    const int R = passes * M;
    CHK(launch(ce_rows_kernel, dim3((R + 3) / 4), dim3(256), 0, s, logits, tgt, R, C, pad, row_loss));
    for (int q = 0; q < passes; ++q)
        CHK(launch(ce_reduce_kernel, dim3(1), dim3(256), 0, s, row_loss + (size_t)q * M, tgt + (size_t)q * M, M, pad, loss + q, count + q));
    return launch(ce_bwd_kernel, dim3((R + 3) / 4), dim3(256), 0, s, logits, tgt, R, C, pad, 1.0f / (float)total_targets);
}

// ---- decoder side ---------------------------------------------------------------------------------------------------------------------
// The K permutation passes of a step share every weight and differ in their masks, dropout sites and (after two passes) targets only
// (system.py:175-196), so the decoder runs them as ONE batch of KP * B images (KP = K by default): every Linear product, LayerNorm,
// attention launch and column sum once per step instead of once per pass — 6 x the rows per launch, a sixth of the launches and of the
// split-K folds, the dW products contracted over all passes at once.  PARSEQ_TRAIN_PERM_GROUP=g runs the passes g at a time (1 = one after
// the other, the arrangement of rounds 1-2: same masks, same per-pass losses, gradients equal up to fp32 summation order).
// ca_loop: the cross-attention walks the passes of a batch inside one workgroup (train_attn_dec_bf16_kernel's pass_loop: bf16-operand mode,
// head width 32, <= TD_Q queries, <= TD_K memory tokens), so no pass keeps its own d K | d V of the memory; PARSEQ_TRAIN_NO_PASS_LOOP=1
// turns it off.  Decided here, once per call, for the layout (which then has no per-pass copies) and for parseq_train_decoder alike.
struct TrainDecRoute { int KP; bool ca_loop; };
static TrainDecRoute train_dec_route(const parseq_model* m, int L, int K) {
    TrainDecRoute r;
    int g = K;
    if (const char* e = getenv("PARSEQ_TRAIN_PERM_GROUP")) { const int v = atoi(e); if (v >= 1) g = v; }
    r.KP = std::min(std::max(g, 1), K);
    const int E = m->cfg.embed_dim;
    // the shape question only (rows of E = dec_heads * 32 floats are 16-byte rows); parseq_train_decoder asks the plan itself once the operands exist
    r.ca_loop = r.KP > 1 && E == m->cfg.dec_heads * TD_HD && train_attn_dec_bf16_shape(m->train_precision == PARSEQ_BF16, TD_HD, L, m->tokens) &&
                !getenv("PARSEQ_TRAIN_NO_PASS_LOOP");
    return r;
}

// The decoder's workspace: offsets in floats into the caller's buffer, one member and one row of kDecBufs per buffer.  A row names the
// buffer (parseq_train_decoder_workspace_offset answers by that name), its rows and its width; the layout hands the buffers out in table order.
struct TrainDecoderLayout {
    size_t content0, content, cn, kvc, qd, qn, qsa, kvm, sa_o, t1, n1, q2, ca_o, t2, n2, hpre, hact, t3, out, logits;
    size_t d_a, d_b, d_c, d_h, pm, d_kvc, d_kvm, d_kvm_p, d_content, d_pq, d_qb, row_loss, tgt_all, losses, counts, scratch, total;
    size_t scratch_floats;
};
enum DecRows { ROWS_PASSES, ROWS_ONCE, ROWS_MEMORY, ROWS_MEMORY_PASSES, ROWS_POS, ROWS_PERMS, ROWS_PERMS_1, ROWS_SCRATCH };
enum DecWidth { W_E, W_2E, W_F, W_C, W_1 };
struct DecBuf { const char* name; size_t TrainDecoderLayout::* at; DecRows rows; DecWidth width; };
#define DEC_BUF(member, rows, width) {#member, &TrainDecoderLayout::member, rows, width}
static const DecBuf kDecBufs[] = {
    DEC_BUF(content0, ROWS_ONCE, W_E), DEC_BUF(content, ROWS_PASSES, W_E), DEC_BUF(cn, ROWS_PASSES, W_E), DEC_BUF(kvc, ROWS_PASSES, W_2E),
    DEC_BUF(qd, ROWS_PASSES, W_E), DEC_BUF(qn, ROWS_PASSES, W_E), DEC_BUF(qsa, ROWS_PASSES, W_E), DEC_BUF(kvm, ROWS_MEMORY, W_2E),
    DEC_BUF(sa_o, ROWS_PASSES, W_E), DEC_BUF(t1, ROWS_PASSES, W_E), DEC_BUF(n1, ROWS_PASSES, W_E), DEC_BUF(q2, ROWS_PASSES, W_E),
    DEC_BUF(ca_o, ROWS_PASSES, W_E), DEC_BUF(t2, ROWS_PASSES, W_E), DEC_BUF(n2, ROWS_PASSES, W_E), DEC_BUF(hpre, ROWS_PASSES, W_F),
    DEC_BUF(hact, ROWS_PASSES, W_F), DEC_BUF(t3, ROWS_PASSES, W_E), DEC_BUF(out, ROWS_PASSES, W_E),
    {"dlogits", &TrainDecoderLayout::logits, ROWS_PASSES, W_C},      // the logits, then their gradient in place: the name callers ask for
    DEC_BUF(d_a, ROWS_PASSES, W_E), DEC_BUF(d_b, ROWS_PASSES, W_E), DEC_BUF(d_c, ROWS_PASSES, W_E), DEC_BUF(d_h, ROWS_PASSES, W_F),
    DEC_BUF(pm, ROWS_PASSES, W_E), DEC_BUF(d_kvc, ROWS_PASSES, W_2E), DEC_BUF(d_kvm, ROWS_MEMORY, W_2E),
    // each pass's own d K | d V of the memory, folded into d_kvm after the batch — only where the cross-attention cannot walk the passes
    // itself; otherwise the name stands for d_kvm
    DEC_BUF(d_kvm_p, ROWS_MEMORY_PASSES, W_2E),
    DEC_BUF(d_content, ROWS_ONCE, W_E), DEC_BUF(d_pq, ROWS_POS, W_E), DEC_BUF(d_qb, ROWS_PASSES, W_E), DEC_BUF(row_loss, ROWS_PASSES, W_1),
    DEC_BUF(tgt_all, ROWS_PERMS, W_1), DEC_BUF(losses, ROWS_PERMS_1, W_1), DEC_BUF(counts, ROWS_PERMS_1, W_1), DEC_BUF(scratch, ROWS_SCRATCH, W_1)};
#undef DEC_BUF
static TrainDecoderLayout train_decoder_layout(const parseq_model* m, int B, int L, int K, const TrainDecRoute& r) {
    const size_t E = m->cfg.embed_dim, M = (size_t)B * L, MS = (size_t)B * m->tokens, P = (size_t)r.KP;
    TrainDecoderLayout o;
    o.scratch_floats = train_scratch_floats(P * M, E);
    // DecRows: a row per token of every pass of a batch / of one pass / per memory token / per memory token and pass / per position /
    // per token of all K permutations / K + 1 scalars / the scratch
    const size_t rows[] = {P * M, M, MS, P * MS, (size_t)L, (size_t)K * M, (size_t)K + 1, o.scratch_floats};
    const size_t width[] = {E, 2 * E, E * m->cfg.dec_mlp_ratio, (size_t)m->classes, 1};
    Take take;
    for (const DecBuf& b : kDecBufs) {
        const bool alias = b.at == &TrainDecoderLayout::d_kvm_p && !(r.KP > 1 && !r.ca_loop);
        o.*b.at = alias ? o.d_kvm : take(rows[b.rows] * width[b.width]);
    }
    o.total = take.off;
    return o;
}

// The decoder's parameters and their gradient slots, resolved once per call; the training step has depth-1 decoder kernels only
enum TrainDecParam { D_NORM_C_W, D_NORM_C_B, D_NORM_Q_W, D_NORM_Q_B, D_NORM1_W, D_NORM1_B, D_NORM2_W, D_NORM2_B, D_SA_IN_W, D_SA_IN_B, D_SA_OUT_W, D_SA_OUT_B,
                     D_CA_IN_W, D_CA_IN_B, D_CA_OUT_W, D_CA_OUT_B, D_LIN1_W, D_LIN1_B, D_LIN2_W, D_LIN2_B, D_LAYER_PARAMS,
                     D_NORM_W = D_LAYER_PARAMS, D_NORM_B, D_HEAD_W, D_HEAD_B, D_TEXT_EMBED, D_POS_QUERIES, D_PARAMS };
static const char* const kDecKeys[D_PARAMS] = {
    "norm_c.weight", "norm_c.bias", "norm_q.weight", "norm_q.bias", "norm1.weight", "norm1.bias", "norm2.weight", "norm2.bias",
    "self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
    "cross_attn.in_proj_weight", "cross_attn.in_proj_bias", "cross_attn.out_proj.weight", "cross_attn.out_proj.bias",
    "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias",
    "decoder.norm.weight", "decoder.norm.bias", "head.weight", "head.bias", "text_embed.embedding.weight", "pos_queries"};
static std::string train_dec_key(int k) { return k < D_LAYER_PARAMS ? std::string("decoder.layers.0.") + kDecKeys[k] : std::string(kDecKeys[k]); }
using TrainDecW = ParamSet<D_PARAMS>;
static TrainDecW train_dec_weights(const parseq_model* m, float* grads) {
    TrainDecW W;
    for (int k = 0; k < D_PARAMS; ++k) W.v[k] = param_ref(m, train_dec_key(k), grads);
    return W;
}

extern "C" int64_t parseq_model_param_offset(const parseq_model* m, int index) {
    if (!m || index < 0 || index >= (int)m->params.size()) return -1;
    return (int64_t)m->params[index].offset;
}
extern "C" int64_t parseq_model_grad_elems(const parseq_model* m) { return m ? (int64_t)m->master_elems : 0; }
extern "C" int parseq_model_set_train_precision(parseq_model* m, int precision) {
    if (!m) return fail(PARSEQ_E_INVALID, "null model");
    if (!train_ops_ok(precision)) return fail(PARSEQ_E_INVALID, "training precision %d (PARSEQ_F32, PARSEQ_BF16 or PARSEQ_BF16X3)", precision);
    m->train_precision = precision;
    return 0;
}

// Where a named buffer lives in the workspace, in floats — of a per-pass buffer, the slot of the LAST permutation; -1 if unknown.  For tests.
extern "C" int64_t parseq_train_decoder_workspace_offset(const parseq_model* m, int batch, int ctx_len, int num_perms, const char* name) {
    if (!m || !name || batch <= 0 || ctx_len <= 0 || num_perms <= 0) return -1;
    const TrainDecRoute r = train_dec_route(m, ctx_len, num_perms);
    const TrainDecoderLayout o = train_decoder_layout(m, batch, ctx_len, num_perms, r);
    const size_t E = m->cfg.embed_dim, M = (size_t)batch * ctx_len;
    const size_t width[] = {E, 2 * E, E * m->cfg.dec_mlp_ratio, (size_t)m->classes, 1};
    const size_t last = (size_t)((num_perms - 1) % r.KP);      // the last pass's slot in its batch of KP passes
    for (const DecBuf& b : kDecBufs)
        if (!strcmp(b.name, name)) return (int64_t)(o.*b.at + (b.rows == ROWS_PASSES ? last * M * width[b.width] : 0));
    return -1;
}

extern "C" size_t parseq_train_decoder_workspace_bytes(const parseq_model* m, int batch, int ctx_len, int num_perms) {
    if (!m || batch <= 0 || ctx_len <= 0 || num_perms <= 0) return 0;
    return train_decoder_layout(m, batch, ctx_len, num_perms, train_dec_route(m, ctx_len, num_perms)).total * sizeof(float);
}

// y = R + dropout(x) over `passes` passes of n_pass elements each (train_rows.h dropout_passes_kernel: R may be null, x == y allowed,
// x_shared: one pass of x read by every pass); with dropout off a plain add / copy
static int dropout_add(const TrainCtx& cx, const float* x, bool x_shared, const float* R, float* y, size_t n_pass, int passes, const DropSpec& d, unsigned site) {
    return launch(dropout_passes_kernel, dim3((unsigned)((n_pass + 255) / 256), (unsigned)passes), dim3(256), 0, cx.s, x, x_shared ? 1 : 0, R, y, n_pass, d, site);
}

extern "C" int parseq_train_decoder(parseq_model* m, const float* memory, const int32_t* tokens, const int32_t* targets, const uint8_t* key_padding_mask,
                                    const uint8_t* query_masks, int batch, int ctx_len, int num_perms, int total_targets, float dropout_p,
                                    uint64_t seed, float* loss_out, float* grads, float* dmemory, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || !memory || !tokens || !targets || !key_padding_mask || !query_masks || !loss_out || !grads || !dmemory || !workspace)
        return fail(PARSEQ_E_INVALID, "null argument");
    if (m->vitstr) return fail(PARSEQ_E_INVALID, "ViTSTR has no decoder");
    if (m->cfg.dec_depth != 1) return fail(PARSEQ_E_INVALID, "dec_depth=%d: the training step has depth-1 decoder kernels only", m->cfg.dec_depth);
    CHK(require_params_set(m));
    m->grad_events_valid = false;      // a new step starts writing the flat gradient buffer: the previous step's segment events say nothing about it
    DevGuard dg(m->device);
    const int B = batch, L = ctx_len, K = num_perms;
    if (B <= 0 || L < 2 || L > m->cfg.max_label_length + 1 || K <= 0 || total_targets <= 0)
        return fail(PARSEQ_E_INVALID, "bad shape: batch %d, ctx_len %d (2..%d), %d permutations, %d targets", B, L, m->cfg.max_label_length + 1, K, total_targets);
    if (!dropout_p_ok(dropout_p)) return fail(PARSEQ_E_INVALID, "dropout_p %g outside [0, 1)", dropout_p);
    const TrainDecRoute route = train_dec_route(m, L, K);
    const TrainDecoderLayout o = train_decoder_layout(m, B, L, K, route);
    if (workspace_bytes < o.total * sizeof(float)) return fail(PARSEQ_E_INVALID, "workspace: %zu bytes given, %zu needed", workspace_bytes, o.total * sizeof(float));
    hipStream_t s = (hipStream_t)stream;
    const int E = m->cfg.embed_dim, F = E * m->cfg.dec_mlp_ratio, S = m->tokens, C = m->classes, H = m->cfg.dec_heads, M = B * L, MS = B * S;
    const float eps = m->cfg.dec_ln_eps, scale = 1.0f / sqrtf(32.0f), sqrtE = sqrtf((float)E);
    const DropSpec drop = drop_spec(dropout_p, seed);
    float* w = reinterpret_cast<float*>(workspace);
    const TrainDecW W = train_dec_weights(m, grads);
    // the in-projections by their rows: [0, E) the queries, [E, 3E) k | v
    const float* sa_w = W(D_SA_IN_W); const float* sa_b = W(D_SA_IN_B); const float* ca_w = W(D_CA_IN_W); const float* ca_b = W(D_CA_IN_B);
    const float* pq = W(D_POS_QUERIES);
    int* tgt_all = reinterpret_cast<int*>(w + o.tgt_all); float* losses = w + o.losses; int* counts = reinterpret_cast<int*>(w + o.counts);
    const size_t ME = (size_t)M * E, MF = (size_t)M * F, EE = (size_t)E * E;
    const int KP = route.KP; const bool ca_loop = route.ca_loop;      // passes per batch; the pass-walking cross-attention
    const TrainCtx cx{s, w + o.scratch, m->train_precision, o.scratch_floats};

    // ---- shared by all permutations: the content rows before dropout, and the memory's K / V (model.py:95-98, modules.py:74) ----
    CHK(launch(train_content_kernel, dim3(M), dim3(256), 0, s, W(D_TEXT_EMBED), pq, tokens, L, L, E, sqrtE, w + o.content0));
    CHK(lin_fwd(cx, memory, ca_w + EE, ca_b + E, nullptr, 0, w + o.kvm, MS, 2 * E, E));
    if (KP == 1) HIPCHK(hipMemsetAsync(w + o.d_kvm, 0, (size_t)MS * 2 * E * sizeof(float), s));      // the passes accumulate into it one after the other
    HIPCHK(hipMemsetAsync(w + o.d_pq, 0, (size_t)L * E * sizeof(float), s));
    // the targets of pass i, one row per pass: <eos> targets are dropped after two permutations (system.py:191-195)
    for (int i = 0; i < K; ++i)
        HIPCHK(hipMemcpyAsync(tgt_all + (size_t)i * M, targets + (size_t)(i < 2 ? 0 : 1) * M, (size_t)M * sizeof(int), hipMemcpyDeviceToDevice, s));

    TrainAttnArgs sa{};      // self-attention of the query stream over the content stream (modules.py:70-72)
    sa.q = w + o.qsa; sa.q_bstride = (long)L * E; sa.ldq = E; sa.k = w + o.kvc; sa.v = w + o.kvc + E; sa.ldkv = 2 * E; sa.kmask = key_padding_mask; sa.ldkm = L;
    sa.o = w + o.sa_o; sa.ldo = E; sa.d_o = w + o.d_b; sa.dq = w + o.d_qb; sa.lddq = E; sa.dk = w + o.d_kvc; sa.dv = w + o.d_kvc + E; sa.lddkv = 2 * E;
    sa.Lq = L; sa.Lk = L; sa.H = H; sa.scale = scale; sa.kv_accumulate = 0; sa.drop = drop;
    sa.pass_B = B; sa.qmask_pstride = (long)L * L; sa.site_pstride = 8; sa.kv_shared = 0;
    TrainAttnArgs ca{};      // cross-attention over the encoder memory (modules.py:74-75)
    ca.q = w + o.q2; ca.q_bstride = (long)L * E; ca.ldq = E; ca.k = w + o.kvm; ca.v = w + o.kvm + E; ca.ldkv = 2 * E; ca.o = w + o.ca_o; ca.ldo = E;
    ca.d_o = w + o.d_c; ca.dq = w + o.d_a; ca.lddq = E; ca.lddkv = 2 * E; ca.Lq = L; ca.Lk = S; ca.H = H; ca.scale = scale;
    // d K | d V: KP == 1: d_kvm_p IS d_kvm and the passes accumulate; otherwise each pass of the batch writes its own copy — or, in the
    // bf16-operand mode, one workgroup per (image, head) walks the batch's passes (train_attn.h TrainAttnArgs::pass_loop): the memory's K | V are
    // staged once per batch instead of once per pass and d K | d V go straight into d_kvm (which d_kvm_p then names too), summed over the
    // passes in the accumulators
    ca.dk = w + o.d_kvm_p; ca.dv = w + o.d_kvm_p + E; ca.kv_accumulate = KP == 1 ? 1 : 0;
    ca.drop = drop;
    ca.pass_B = B; ca.qmask_pstride = 0; ca.site_pstride = 8; ca.kv_shared = 1;
    // the route (and with it the layout, which then has no per-pass copies) chose the pass-walking kernel; the kernel's own preconditions must agree
    TrainAttnPlan ca_plan;      // consulted for its route alone (pass_loop is set per batch below); a refusal by the plan is answered with the message here
    if (ca_loop && (train_attn_plan(cx, ca, 32, KP * B, true, &ca_plan) != 0 || ca_plan.route != TA_DEC_BF16)) return fail(PARSEQ_E_STATE, "training decoder: the workspace was laid out for the pass-walking cross-attention, which this call cannot run (its operands are not aligned for it)");
    // Both attentions are planned in both directions BEFORE the passes start (only the workspace has been written so far): the backward holds more in LDS than the forward
    // (train_attn_lds_floats: at 32 queries of width 32 the forward fits up to 256 keys, the backward up to 223), so without this a step in
    // the fp32 mode over 224..256 memory tokens would run its forward and be refused in the middle of its backward, gradients half written.
    // Planned as the arguments stand here: sa.qmask is still null and ca.pass_loop still 0 (both are set per batch below).  At head width 32 no
    // route asks whether a mask is present, and pass_loop only adds a condition on pass_B, kv_shared and the batch size that the per-batch
    // call meets by construction (pass_loop = kp, batch = kp * B) — a route that came to depend on either would have to be planned with them set.
    for (const TrainAttnArgs* at : {&sa, &ca})
        for (const bool bw : {false, true}) { TrainAttnPlan pl; CHK(train_attn_plan(cx, *at, 32, KP * B, bw, &pl)); }
    enum { S_CONTENT, S_QUERY, S_SA_PROB, S_SA_OUT, S_CA_PROB, S_CA_OUT, S_FF_HIDDEN, S_FF_OUT };      // dropout sites of one pass

    for (int i0 = 0; i0 < K; i0 += KP) {
        const int kp = std::min(KP, K - i0);       // passes i0 .. i0 + kp - 1 as one batch of kp * B images
        const int R = kp * M;                      // rows of this batch
        const size_t RF = (size_t)R * F;
        const int32_t* tgt = tgt_all + (size_t)i0 * M;
        auto site = [&](int k) { return (unsigned)(8 * i0 + k); };      // of the batch's first pass; pass p draws site + 8 p
        // ---- forward: model.decode (model.py:86-103) — the embeddings and the queries are dropped afresh in every pass -----------
        CHK(dropout_add(cx, w + o.content0, true, nullptr, w + o.content, ME, kp, drop, site(S_CONTENT)));
        CHK((run_layernorm<float>(s, w + o.content, W(D_NORM_C_W), W(D_NORM_C_B), w + o.cn, nullptr, R, E, eps)));
        CHK(lin_fwd(cx, w + o.cn, sa_w + EE, sa_b + E, nullptr, 0, w + o.kvc, R, 2 * E, E));
        CHK(launch(dropout_rows_passes_kernel, dim3((unsigned)((ME + 255) / 256), (unsigned)kp), dim3(256), 0, s, pq, L, E, w + o.qd, ME, drop, site(S_QUERY)));
        CHK((run_layernorm<float>(s, w + o.qd, W(D_NORM_Q_W), W(D_NORM_Q_B), w + o.qn, nullptr, R, E, eps)));
        CHK(lin_fwd(cx, w + o.qn, sa_w, sa_b, nullptr, 0, w + o.qsa, R, E, E));
        // ---- DecoderLayer.forward_stream (modules.py:55-79), Decoder.norm (:124), head (model.py:63) -----------------------------
        sa.qmask = query_masks + (size_t)i0 * L * L; sa.drop_site = site(S_SA_PROB);
        CHK(train_attn(cx, sa, kp * B, false, 32));
        CHK(lin_fwd(cx, w + o.sa_o, W(D_SA_OUT_W), W(D_SA_OUT_B), nullptr, 0, w + o.pm, R, E, E));
        CHK(dropout_add(cx, w + o.pm, false, w + o.qd, w + o.t1, ME, kp, drop, site(S_SA_OUT)));
        CHK((run_layernorm<float>(s, w + o.t1, W(D_NORM1_W), W(D_NORM1_B), w + o.n1, nullptr, R, E, eps)));
        CHK(lin_fwd(cx, w + o.n1, ca_w, ca_b, nullptr, 0, w + o.q2, R, E, E));
        ca.drop_site = site(S_CA_PROB);
        if (ca_loop) { ca.pass_loop = kp; ca.kv_accumulate = i0 > 0 ? 1 : 0; }
        CHK(train_attn(cx, ca, kp * B, false, 32));
        CHK(lin_fwd(cx, w + o.ca_o, W(D_CA_OUT_W), W(D_CA_OUT_B), nullptr, 0, w + o.pm, R, E, E));
        CHK(dropout_add(cx, w + o.pm, false, w + o.t1, w + o.t2, ME, kp, drop, site(S_CA_OUT)));
        CHK((run_layernorm<float>(s, w + o.t2, W(D_NORM2_W), W(D_NORM2_B), w + o.n2, nullptr, R, E, eps)));
        CHK(lin_fwd(cx, w + o.n2, W(D_LIN1_W), W(D_LIN1_B), nullptr, 0, w + o.hpre, R, F, E, w + o.hact));      // hact = gelu(hpre): the product's epilogue (bf16-operand mode) or gelu_fwd_kernel
        if (drop.thresh) CHK(dropout_add(cx, w + o.hact, false, nullptr, w + o.hact, MF, kp, drop, site(S_FF_HIDDEN)));
        CHK(lin_fwd(cx, w + o.hact, W(D_LIN2_W), W(D_LIN2_B), nullptr, 0, w + o.pm, R, E, F));
        CHK(dropout_add(cx, w + o.pm, false, w + o.t2, w + o.t3, ME, kp, drop, site(S_FF_OUT)));
        CHK((run_layernorm<float>(s, w + o.t3, W(D_NORM_W), W(D_NORM_B), w + o.out, nullptr, R, E, eps)));
        CHK(lin_fwd(cx, w + o.out, W(D_HEAD_W), W(D_HEAD_B), nullptr, 0, w + o.logits, R, C, E));
        CHK(ce_loss_and_grad(s, w + o.logits, tgt, kp, M, C, m->cfg.pad_id, w + o.row_loss, losses + i0, counts + i0, total_targets));
        // ---- backward (o.logits now holds d logits) ------------------------------------------------------------------------------
        CHK(lin_bwd(cx, w + o.out, W(D_HEAD_W), w + o.logits, W.g(D_HEAD_W), W.g(D_HEAD_B), w + o.d_a, R, C, E));                              // d_a = d out
        CHK(ln_bwd(cx, w + o.t3, W(D_NORM_W), w + o.d_a, nullptr, w + o.d_b, W.g(D_NORM_W), W.g(D_NORM_B), R, E, eps));                        // d_b = d t3
        CHK(dropout_add(cx, w + o.d_b, false, nullptr, w + o.pm, ME, kp, drop, site(S_FF_OUT)));
        CHK(lin_bwd(cx, w + o.hact, W(D_LIN2_W), w + o.pm, W.g(D_LIN2_W), W.g(D_LIN2_B), w + o.d_h, R, E, F));                                 // d_h = d hact
        if (drop.thresh && MF % 4 == 0)            // d_h = d hpre: the MLP's inner dropout and the GELU backward in one pass
            CHK(launch(gelu_bwd_drop_passes_kernel, dim3((unsigned)((MF + 1023) / 1024), (unsigned)kp), dim3(256), 0, s, w + o.hpre, w + o.d_h, w + o.d_h, MF, drop, site(S_FF_HIDDEN)));
        else {
            if (drop.thresh) CHK(dropout_add(cx, w + o.d_h, false, nullptr, w + o.d_h, MF, kp, drop, site(S_FF_HIDDEN)));
            CHK(gelu_bwd(cx, w + o.hpre, w + o.d_h, RF));
        }
        CHK(lin_bwd(cx, w + o.n2, W(D_LIN1_W), w + o.d_h, W.g(D_LIN1_W), W.g(D_LIN1_B), w + o.d_a, R, F, E));                                  // d_a = d n2
        CHK(ln_bwd(cx, w + o.t2, W(D_NORM2_W), w + o.d_a, w + o.d_b, w + o.d_b, W.g(D_NORM2_W), W.g(D_NORM2_B), R, E, eps));                   // d_b = d t2
        CHK(dropout_add(cx, w + o.d_b, false, nullptr, w + o.pm, ME, kp, drop, site(S_CA_OUT)));
        CHK(lin_bwd(cx, w + o.ca_o, W(D_CA_OUT_W), w + o.pm, W.g(D_CA_OUT_W), W.g(D_CA_OUT_B), w + o.d_c, R, E, E));                           // d_c = d ca_o
        CHK(train_attn(cx, ca, kp * B, true, 32));                                                                                              // d_a = d q2; d_kvm_p[pass] = (KP == 1: d_kvm +=)
        if (KP > 1 && !ca_loop)                    // d_kvm (+)= the batch's passes, in ascending order
            CHK(launch(sum_passes_kernel, dim3((unsigned)(((size_t)MS * 2 * E / 4 + 255) / 256)), dim3(256), 0, s, w + o.d_kvm_p, w + o.d_kvm, (size_t)MS * 2 * E, kp,
                       i0 > 0 ? 1 : 0));
        CHK(lin_bwd(cx, w + o.n1, ca_w, w + o.d_a, W.g(D_CA_IN_W), W.g(D_CA_IN_B), w + o.d_c, R, E, E));                                        // d_c = d n1
        CHK(ln_bwd(cx, w + o.t1, W(D_NORM1_W), w + o.d_c, w + o.d_b, w + o.d_a, W.g(D_NORM1_W), W.g(D_NORM1_B), R, E, eps));                   // d_a = d t1
        CHK(dropout_add(cx, w + o.d_a, false, nullptr, w + o.pm, ME, kp, drop, site(S_SA_OUT)));
        CHK(lin_bwd(cx, w + o.sa_o, W(D_SA_OUT_W), w + o.pm, W.g(D_SA_OUT_W), W.g(D_SA_OUT_B), w + o.d_b, R, E, E));                           // d_b = d sa_o
        CHK(train_attn(cx, sa, kp * B, true, 32));                                                                                              // d_qb = d q; d_kvc =
        CHK(lin_bwd(cx, w + o.qn, sa_w, w + o.d_qb, W.g(D_SA_IN_W), W.g(D_SA_IN_B), w + o.d_c, R, E, E));                                       // d_c = d qn
        CHK(ln_bwd(cx, w + o.qd, W(D_NORM_Q_W), w + o.d_c, w + o.d_a, w + o.d_b, W.g(D_NORM_Q_W), W.g(D_NORM_Q_B), R, E, eps));                // d_b = d qd
        CHK(dropout_add(cx, w + o.d_b, false, nullptr, w + o.d_b, ME, kp, drop, site(S_QUERY)));
        CHK(colsum(cx, w + o.d_b, (long)L * E, kp * B, L * E, w + o.d_pq, true));               // every image's query rows are pos_queries[l]
        CHK(lin_bwd(cx, w + o.cn, sa_w + EE, w + o.d_kvc, W.g(D_SA_IN_W) + EE, W.g(D_SA_IN_B) + E, w + o.d_c, R, 2 * E, E));                    // d_c = d cn
        CHK(ln_bwd(cx, w + o.content, W(D_NORM_C_W), w + o.d_c, nullptr, w + o.d_b, W.g(D_NORM_C_W), W.g(D_NORM_C_B), R, E, eps));             // d_b = d content
        // d_content (+)= every pass's d content through that pass's mask (the passes in ascending order)
        CHK(launch(dropout_sum_passes_kernel, dim3((unsigned)((ME + 255) / 256)), dim3(256), 0, s, w + o.d_b, w + o.d_content, ME, kp, drop, site(S_CONTENT), i0 > 0 ? 1 : 0));
    }
    CHK(launch(loss_combine_kernel, dim3(1), dim3(64), 0, s, losses, counts, K, losses + K));
    HIPCHK(hipMemcpyAsync(loss_out, losses + K, sizeof(float), hipMemcpyDeviceToDevice, s));
    HIPCHK(hipMemcpyAsync(loss_out + 1, losses, (size_t)K * sizeof(float), hipMemcpyDeviceToDevice, s));

    // ---- what every permutation shares, once ---------------------------------------------------------------------------------------
    if (L > 1) CHK(colsum(cx, w + o.d_content + E, (long)L * E, B, (L - 1) * E, w + o.d_pq, true));       // content row j carries pos_queries[j - 1]
    {   // token-embedding gradient: the B * L rows in chunks of 768, one workgroup per (token id, chunk), then the chunks folded in order
        const int rows_per = 768, chunks = (M + rows_per - 1) / rows_per;
        if (chunks > 1 && (size_t)m->cfg.num_tokens * chunks * E <= cx.scratch_floats) {
            CHK(launch(embed_bwd_kernel, dim3(m->cfg.num_tokens, chunks), dim3(256), 0, s, w + o.d_content, tokens, L, B, L, E, sqrtE, W.g(D_TEXT_EMBED), cx.scratch, rows_per));
            CHK(launch(embed_bwd_fold_kernel, dim3(m->cfg.num_tokens), dim3(256), 0, s, cx.scratch, chunks, E, sqrtE, W.g(D_TEXT_EMBED)));
        } else {
            CHK(launch(embed_bwd_kernel, dim3(m->cfg.num_tokens, 1), dim3(256), 0, s, w + o.d_content, tokens, L, B, L, E, sqrtE, W.g(D_TEXT_EMBED), (float*)nullptr, M));
        }
    }
    CHK(lin_bwd(cx, memory, ca_w + EE, w + o.d_kvm, W.g(D_CA_IN_W) + EE, W.g(D_CA_IN_B) + E, dmemory, MS, 2 * E, E));
    return launch(add_kernel, dim3((unsigned)(((size_t)L * E + 255) / 256)), dim3(256), 0, s, W.g(D_POS_QUERIES), w + o.d_pq, W.g(D_POS_QUERIES), (size_t)L * E);
}

// ---- training step, encoder side: forward that keeps what the backward needs, and the backward ------------------------------
struct TrainEncoderLayout {          // offsets in floats
    size_t patches, layer0, layer_stride, x_last, d_x, d_a, d_h, dqkv, tmp, scratch, scratch2, scratch_floats, total;      // scratch2: the backward's second stream
    size_t w16, w16_layer, d_x16, d_h16;      // bf16 shadows (TrainEncRoute::shadows): the Linear weights and their transposes ([layer][qkv, proj, fc1, fc2][W16 | Wt16]),
                                              // the residual-stream gradient and the fc1-output gradient
    size_t x(int i) const { return layer0 + i * layer_stride; }
    size_t lse = 0, dsum = 0;        // past 128 tokens only (train_attn_wide.h): the attention's log-sum-exp [B, H, tokens] inside each layer's
                                     // record, and the backward's D = rowsum(dO o O) [B, H, tokens] (one slot)
    size_t qkv, ao, x_mid, hpre, hact_l, n1, n2;     // offsets inside one layer's record (x at 0); hact_l, n1, n2: the GELU output and the two
                                             // LayerNorm outputs, kept for the backward (round 3: they used to be recomputed there — a 600 MB and two
                                             // 150 MB passes per block; the record grows from 10 E to 16 E floats per token per block)
};
// How a training encoder call runs, decided once per call (on every call: the switches may change between two steps of one process):
//   shadows      bf16 shadow operands for the encoder's products (train_gemm.h SgemmArgs): the bf16-operand mode at the shapes the bf16
//                attention kernel and the 64-deep GEMM take.  The record's n1 / n2 / ao / hact_l slots then hold bf16 (in the first half of
//                the fp32 slot).  PARSEQ_TRAIN_NO_SHADOWS=1 keeps every operand fp32 in memory (the A/B and the bit-identity test).
//   bf16_only    level 2 (the default with shadows on): tensors that exist ONLY to be rounded to bf16 by their consumers or to feed a GELU
//                derivative are stored as bf16 and nothing else — the fc1 pre-activation (its GELU derivative is taken at the bf16 value),
//                the gradient of the fc1 output and the gradient of q | k | v (the dW products read them as bf16 too; the bias gradients are
//                sums of the bf16 values) — and the fc2 / proj dW products read the residual-stream gradient through its bf16 shadow (the
//                fp32 copy stays: LayerNorm backward adds to it).  That is what bf16-mixed autocast keeps of these tensors (BASELINE
//                configs[4]); it is no longer bit-identical to the fp32-in-memory path — the oracle gates of the bf16-operand mode hold
//                it.  PARSEQ_TRAIN_SHADOW_LEVEL=1: shadows beside the fp32 copies only (bit-identical).
//   one_launch   the forward as one launch: the bf16-only record at the geometry encoder_blocks.h is written for (E = 384, six 64-wide
//                heads, 128 tokens, hidden = 4 E) with a block's record inside one 32-bit buffer descriptor.  PARSEQ_TRAIN_ENC_PER_OP=1:
//                the per-operation launches (the A/B; also what every other geometry and record mode runs).
//   two_streams  the backward's weight-gradient products on a side stream (enc_block_bwd_shadow); PARSEQ_TRAIN_ONE_STREAM=1 and level 1: one stream.
//   wide         more than 128 tokens: the key-streaming attention (train_attn_wide.h) with its lse / dsum slots; the record at 128 tokens
//                stays as it was, slot for slot.
// The layout's sizes depend on `wide` (the lse / dsum slots; train_enc_wide, which the route repeats) and on whether a second stream can
// exist at all (scratch2: the precision, not the switch, so a workspace serves either setting) — facts of the model alone; everything
// else of the route needs the layout's record stride first.
struct TrainEncRoute {
    bool shadows, bf16_only, one_launch, two_streams, wide;
    EncRecordMode record() const { return bf16_only ? REC_BF16_ONLY : shadows ? REC_SHADOWS : REC_F32; }      // what the record's slots hold
};
static bool train_enc_wide(const parseq_model* m) { return m->tokens > 128; }
static TrainEncRoute train_enc_route(const parseq_model* m, const TrainEncoderLayout& o) {
    const int E = m->cfg.embed_dim, F = E * m->cfg.enc_mlp_ratio;
    TrainEncRoute r;
    r.wide = train_enc_wide(m);
    r.shadows = m->train_precision == PARSEQ_BF16 && E % 64 == 0 && F % 64 == 0 && m->tokens == TB_N && E == m->cfg.enc_heads * TB_HD &&
                !getenv("PARSEQ_TRAIN_NO_SHADOWS");
    const char* lv = getenv("PARSEQ_TRAIN_SHADOW_LEVEL");
    r.bf16_only = r.shadows && !(lv && lv[0] == '1');
    r.one_launch = r.bf16_only && E == 384 && m->cfg.enc_mlp_ratio == 4 && m->tokens == 128 && o.layer_stride * sizeof(float) < ((size_t)1 << 32) &&
                   !getenv("PARSEQ_TRAIN_ENC_PER_OP");
    r.two_streams = r.bf16_only && !getenv("PARSEQ_TRAIN_ONE_STREAM");
    return r;
}
static TrainEncoderLayout train_encoder_layout(const parseq_model* m, int B) {
    const size_t E = m->cfg.embed_dim, F = E * m->cfg.enc_mlp_ratio, MS = (size_t)B * m->tokens, PK = m->patch_k;
    TrainEncoderLayout o;
    Take take;
    o.patches = take(MS * PK);
    o.layer0 = take.off;
    auto slot = [&](size_t n) { return take(n) - o.layer0; };      // inside the first block's record; every block's is laid out alike
    slot(MS * E); o.qkv = slot(MS * 3 * E); o.ao = slot(MS * E); o.x_mid = slot(MS * E); o.hpre = slot(MS * F); o.hact_l = slot(MS * F);
    o.n1 = slot(MS * E); o.n2 = slot(MS * E);
    if (train_enc_wide(m)) o.lse = slot(MS * m->cfg.enc_heads);
    o.layer_stride = take.off - o.layer0;
    take.off = o.layer0 + o.layer_stride * (size_t)m->cfg.enc_depth;
    o.x_last = take(MS * E); o.d_x = take(MS * E); o.d_a = take(MS * E); o.d_h = take(MS * F);
    o.dqkv = take(MS * 3 * E); o.tmp = take(MS * E);
    if (train_enc_wide(m)) o.dsum = take(MS * m->cfg.enc_heads);
    o.scratch_floats = train_scratch_floats(MS, E); o.scratch = take(o.scratch_floats);
    // the second scratch belongs to the backward's second stream, which only the bf16-operand mode has (the fp32 mode carves nothing for it)
    o.scratch2 = m->train_precision == PARSEQ_BF16 ? take(o.scratch_floats) : o.scratch;
    o.w16_layer = 4 * E * E + 2 * E * F;      // floats = 2 bf16 each: W16 and Wt16 of the block's four Linear weights
    o.w16 = take(o.w16_layer * (size_t)m->cfg.enc_depth); o.d_x16 = take(MS * E / 2 + 8); o.d_h16 = take(MS * F / 2 + 8);
    o.total = take.off;
    return o;
}

extern "C" size_t parseq_train_encoder_workspace_bytes(const parseq_model* m, int batch) {
    if (!m || batch <= 0) return 0;
    return train_encoder_layout(m, batch).total * sizeof(float);
}

static int train_encoder_check(const parseq_model* m, int batch, const void* workspace, size_t workspace_bytes) {
    if (!m || !workspace) return fail(PARSEQ_E_INVALID, "null argument");
    if (batch <= 0) return fail(PARSEQ_E_INVALID, "batch %d", batch);
    CHK(require_params_set(m));
    const size_t need = train_encoder_layout(m, batch).total * sizeof(float);
    if (workspace_bytes < need) return fail(PARSEQ_E_INVALID, "workspace: %zu bytes given, %zu needed", workspace_bytes, need);
    return 0;
}

// LayerNorm of the training encoder, written in the type its consumer reads: fp32, or the bf16 shadow
static int train_ln_fwd(hipStream_t s, const float* x, const float* w, const float* b, Out out, int rows, int E, float eps) {
    if (E > 768 || E % 2) return fail(PARSEQ_E_INVALID, "training layernorm: E=%d", E);
    if (out.b16) return launch(ln_fwd_kernel<bf16_t>, dim3((rows + 3) / 4), dim3(256), 0, s, x, w, b, out.b16, rows, E, eps);
    return launch(ln_fwd_kernel<float>, dim3((rows + 3) / 4), dim3(256), 0, s, x, w, b, out.f32, rows, E, eps);
}
extern "C" int parseq_op_train_layernorm(const float* x, const float* gamma, const float* beta, void* y, int y_dtype, const float* dy, const float* add,
                                         float* dx, void* dx16, float* dgamma, float* dbeta, int rows, int E, float eps, int backward, float* scratch,
                                         size_t scratch_floats, void* stream) {
    CHK(check_arch());
    if (!x || !gamma || rows <= 0 || E <= 0) return fail(PARSEQ_E_INVALID, "bad argument");
    if (backward) {
        if (!dy || !dx || !dgamma || !dbeta) return fail(PARSEQ_E_INVALID, "bad argument");
        const TrainCtx cx{(hipStream_t)stream, scratch, PARSEQ_F32, scratch_floats};
        return ln_bwd(cx, x, gamma, dy, add, dx, dgamma, dbeta, rows, E, eps, static_cast<bf16_t*>(dx16));
    }
    if (!beta || !y || !gemm_dtype_ok(y_dtype)) return fail(PARSEQ_E_INVALID, "bad argument");
    return train_ln_fwd((hipStream_t)stream, x, gamma, beta, y_dtype == PARSEQ_BF16 ? Out(static_cast<bf16_t*>(y)) : Out(static_cast<float*>(y)), rows, E, eps);
}

// A block's twelve parameters with their gradient slots, its four Linear weights' bf16 shadows in the workspace (W16 [N, K] and the
// transpose Wt16 [K, N] behind it; `at`: where W16 starts, in bf16 elements from the shadows' base ws + o.w16) and the forward's weight
// operands in the route's type, resolved once per call for all blocks
enum EncBlockParam { E_LN1_W, E_LN1_B, E_QKV_W, E_QKV_B, E_PROJ_W, E_PROJ_B, E_LN2_W, E_LN2_B, E_FC1_W, E_FC1_B, E_FC2_W, E_FC2_B, E_PARAMS };
static const char* const kEncBlockKeys[E_PARAMS] = {"norm1.weight", "norm1.bias", "attn.qkv.weight", "attn.qkv.bias", "attn.proj.weight", "attn.proj.bias",
                                                    "norm2.weight", "norm2.bias", "mlp.fc1.weight", "mlp.fc1.bias", "mlp.fc2.weight", "mlp.fc2.bias"};
static std::string enc_block_key(const parseq_model* m, int i, int k) { return m->enc + "blocks." + std::to_string(i) + "." + kEncBlockKeys[k]; }
enum EncLinear { LIN_QKV, LIN_PROJ, LIN_FC1, LIN_FC2, ENC_LINEARS };      // [3E, E], [E, E], [F, E], [E, F]
static const EncBlockParam kEncLinearW[ENC_LINEARS] = {E_QKV_W, E_PROJ_W, E_FC1_W, E_FC2_W};
struct EncShadowW { bf16_t* w; bf16_t* wt; size_t at; int n, k; };      // n, k: the weight's shape [n, k]
struct EncBlockW : ParamSet<E_PARAMS> {
    EncShadowW s16[ENC_LINEARS];
    In lin[ENC_LINEARS];      // the forward's weight operand: the W16 shadow on the shadow route, the master's fp32 otherwise
};
// grads, ws: null where the caller wants the offsets alone (the device tables below)
static std::vector<EncBlockW> enc_block_weights(const parseq_model* m, const TrainEncoderLayout& o, bool shadows, float* grads, float* ws) {
    const int E = m->cfg.embed_dim, F = E * m->cfg.enc_mlp_ratio;
    const int wn[ENC_LINEARS] = {3 * E, E, F, E}, wk[ENC_LINEARS] = {E, E, E, F};
    bf16_t* base = ws ? reinterpret_cast<bf16_t*>(ws + o.w16) : nullptr;
    std::vector<EncBlockW> W(m->cfg.enc_depth);
    for (int i = 0; i < m->cfg.enc_depth; ++i) {
        for (int k = 0; k < E_PARAMS; ++k) W[i].v[k] = param_ref(m, enc_block_key(m, i, k), grads);
        size_t at = 2 * o.w16_layer * (size_t)i;
        for (int j = 0; j < ENC_LINEARS; ++j) {
            const size_t nk = (size_t)wn[j] * wk[j];
            W[i].s16[j] = EncShadowW{base ? base + at : nullptr, base ? base + at + nk : nullptr, at, wn[j], wk[j]};
            W[i].lin[j] = shadows ? In(W[i].s16[j].w) : In(W[i](kEncLinearW[j]));
            at += 2 * nk;
        }
    }
    return W;
}

// Two device tables, model constants built on first use (offsets only, relative to the master weights and to the shadows' base, so any
// workspace of the same layout serves); each is published only when valid: a failed upload must not leave a non-null table of garbage
// offsets behind for the next call
template <typename T>
static int upload_table(const std::vector<T>& tab, const char* what, T** out) {
    void* dev = nullptr;
    HIPCHK(hipMalloc(&dev, tab.size() * sizeof(T)));
    if (hipMemcpy(dev, tab.data(), tab.size() * sizeof(T), hipMemcpyHostToDevice) != hipSuccess) {
        (void)hipFree(dev);
        return fail(PARSEQ_E_HIP, "upload of the %s table failed: %s", what, hipGetErrorString(hipGetLastError()));
    }
    *out = static_cast<T*>(dev);
    return 0;
}
// weight_shadows_kernel's table: the 4 * depth Linear weights, where each lies in the master and where its W16 | Wt16 pair goes
static int enc_shadow_table(parseq_model* m, const TrainEncoderLayout& o) {
    if (m->shadow_tab_dev) return 0;
    std::vector<ShadowEntry> tab;
    unsigned tile = 0;
    for (const EncBlockW& W : enc_block_weights(m, o, true, nullptr, nullptr))
        for (int j = 0; j < ENC_LINEARS; ++j) {
            const EncShadowW& sh = W.s16[j];
            tab.push_back(ShadowEntry{(unsigned)W.v[kEncLinearW[j]].at, (unsigned)sh.n, (unsigned)sh.k, tile, (unsigned long long)sh.at});
            tile += (unsigned)((sh.n / 32) * (sh.k / 32));
        }
    ShadowEntry* dev = nullptr;
    CHK(upload_table(tab, "weight-shadow", &dev));
    m->shadow_tiles = (int)tile;
    m->shadow_tab_dev = dev;
    return 0;
}
// the one-launch forward's table: per block, the parameters' offsets into the master and the four W16 shadows' (bf16 elements from the shadows' base)
static int enc_block_table(parseq_model* m, const TrainEncoderLayout& o) {
    if (m->train_blocks_dev) return 0;
    std::vector<EncBlockParams> tab;
    for (const EncBlockW& W : enc_block_weights(m, o, true, nullptr, nullptr)) {
        auto off = [&](int k) { return (unsigned)W.v[k].at; };
        auto w16 = [&](int j) { return (unsigned)W.s16[j].at; };
        EncBlockParams e{};
        e.ln1_w = off(E_LN1_W); e.ln1_b = off(E_LN1_B); e.bqkv = off(E_QKV_B); e.bproj = off(E_PROJ_B);
        e.ln2_w = off(E_LN2_W); e.ln2_b = off(E_LN2_B); e.b1 = off(E_FC1_B); e.b2 = off(E_FC2_B);
        e.wqkv = w16(LIN_QKV); e.wproj = w16(LIN_PROJ); e.w1 = w16(LIN_FC1); e.w2 = w16(LIN_FC2);
        tab.push_back(e);
    }
    return upload_table(tab, "training block", &m->train_blocks_dev);
}

// A block's record, slot by slot in the type the route stores it in — the one place where a record slot is read as bf16.  On the shadow
// route n1 / n2 / the attention output / the GELU output hold bf16 in the first half of their slots, at level 2 the fc1 pre-activation too.
//   x, qkv, x_mid, x_out   the block's input, q | k | v, the residual stream after the attention branch, the block's output: fp32 always
//   ao, ao_v               the attention output's slot as the attention kernels address it (rows of E floats, whatever it holds), and its values
//   lse                    past 128 tokens only
struct EncBlockRec { float *x, *qkv, *x_mid, *x_out, *ao, *lse; Out n1, n2, ao_v, hpre, hact; };
static EncBlockRec enc_block_rec(const TrainEncoderLayout& o, float* w, int i, int depth, const TrainEncRoute& r) {
    float* x = w + o.x(i);
    auto slot = [&](size_t at, bool bf16) { return bf16 ? Out(reinterpret_cast<bf16_t*>(x + at)) : Out(x + at); };
    EncBlockRec c;
    c.x = x; c.qkv = x + o.qkv; c.x_mid = x + o.x_mid; c.x_out = w + (i + 1 < depth ? o.x(i + 1) : o.x_last);
    c.ao = x + o.ao; c.lse = r.wide ? x + o.lse : nullptr;
    c.n1 = slot(o.n1, r.shadows); c.n2 = slot(o.n2, r.shadows); c.ao_v = slot(o.ao, r.shadows); c.hact = slot(o.hact_l, r.shadows);
    c.hpre = slot(o.hpre, r.bf16_only);
    return c;
}

static TrainAttnArgs enc_attn_args(const parseq_model* m, float* qkv, float* ao, const float* d_ao, float* dqkv, float* lse = nullptr, float* dsum = nullptr) {
    const int E = m->cfg.embed_dim, S = m->tokens;
    TrainAttnArgs a{};
    a.q = qkv; a.q_bstride = (long)S * 3 * E; a.ldq = 3 * E; a.k = qkv + E; a.v = qkv + 2 * E; a.ldkv = 3 * E;
    a.o = ao; a.ldo = E; a.d_o = d_ao; a.dq = dqkv; a.lddq = 3 * E; a.dk = dqkv ? dqkv + E : nullptr; a.dv = dqkv ? dqkv + 2 * E : nullptr;
    a.lddkv = 3 * E; a.kv_accumulate = 0; a.Lq = S; a.Lk = S; a.H = m->cfg.enc_heads; a.scale = 1.0f / sqrtf((float)ATT_HD);
    a.lse = lse; a.dsum = dsum;
    return a;
}

// One block of the per-operation forward: x_mid = x + proj(attention(qkv(norm1(x)))), x_out = x_mid + fc2(gelu(fc1(norm2(x_mid)))), every
// intermediate into the record.  The operands carry their type: the same seven operations run on fp32 slots and weights or on bf16 shadows.
static int enc_block_fwd(const TrainCtx& cx, const parseq_model* m, int batch, const EncBlockRec& rec, const EncBlockW& W) {
    const int E = m->cfg.embed_dim, F = E * m->cfg.enc_mlp_ratio, MS = batch * m->tokens;
    const float eps = m->cfg.enc_ln_eps;
    CHK(train_ln_fwd(cx.s, rec.x, W(E_LN1_W), W(E_LN1_B), rec.n1, MS, E, eps));
    CHK(lin_fwd(cx, rec.n1, W.lin[LIN_QKV], W(E_QKV_B), nullptr, 0, rec.qkv, MS, 3 * E, E));
    TrainAttnArgs aa = enc_attn_args(m, rec.qkv, rec.ao, nullptr, nullptr, rec.lse);
    aa.o16 = rec.ao_v.b16;
    CHK(train_attn(cx, aa, batch, false, ATT_HD));
    CHK(lin_fwd(cx, rec.ao_v, W.lin[LIN_PROJ], W(E_PROJ_B), rec.x, MS, rec.x_mid, MS, E, E));
    CHK(train_ln_fwd(cx.s, rec.x_mid, W(E_LN2_W), W(E_LN2_B), rec.n2, MS, E, eps));
    CHK(lin_fwd(cx, rec.n2, W.lin[LIN_FC1], W(E_FC1_B), nullptr, 0, rec.hpre, MS, F, E, rec.hact));      // hpre and gelu(hpre), one epilogue
    return lin_fwd(cx, rec.hact, W.lin[LIN_FC2], W(E_FC2_B), rec.x_mid, MS, rec.x_out, MS, E, F);
}

// The patch rows of `rows` patches into `out`: fp32 images through patches_kernel, raw uint8 pixels through patches_u8_kernel
static int train_patches(const parseq_model* m, hipStream_t s, const void* images, int images_dtype, const float* u8_table, int rows, float* out) {
    const int H = m->cfg.img_h, W = m->cfg.img_w, ph = m->cfg.patch_h, pw = m->cfg.patch_w;
    if (images_dtype == PARSEQ_F32) return launch(patches_kernel, dim3(rows), dim3(256), 0, s, static_cast<const float*>(images), H, W, ph, pw, out);
    const uint8_t* img = static_cast<const uint8_t*>(images);
    const size_t segments = (size_t)rows * 3 * ph;
    const dim3 grid((unsigned)((segments + 255) / 256));
    const bool aligned = reinterpret_cast<uintptr_t>(img) % (uintptr_t)pw == 0;
    if (pw == 8 && aligned) return launch(patches_u8_kernel<8>, grid, dim3(256), 0, s, img, u8_table, H, W, ph, pw, segments, out);
    if (pw == 16 && aligned) return launch(patches_u8_kernel<16>, grid, dim3(256), 0, s, img, u8_table, H, W, ph, pw, segments, out);
    return launch(patches_u8_kernel<0>, grid, dim3(256), 0, s, img, u8_table, H, W, ph, pw, segments, out);
}

static int train_encoder_forward(parseq_model* m, const void* images, int images_dtype, const float* u8_table, int batch, float* memory_out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!images || !memory_out) return fail(PARSEQ_E_INVALID, "null argument");
    if (images_dtype != PARSEQ_F32 && images_dtype != PARSEQ_U8)
        return fail(PARSEQ_E_INVALID, "images_dtype %d: the training encoder takes PARSEQ_F32 or PARSEQ_U8 images", images_dtype);
    CHK(train_encoder_check(m, batch, workspace, workspace_bytes));
    DevGuard dg(m->device);
    const TrainEncoderLayout o = train_encoder_layout(m, batch);
    const TrainEncRoute r = train_enc_route(m, o);
    hipStream_t s = (hipStream_t)stream;
    const int E = m->cfg.embed_dim, S = m->tokens, MS = batch * S, PK = m->patch_k, depth = m->cfg.enc_depth;
    const float eps = m->cfg.enc_ln_eps;
    float* w = reinterpret_cast<float*>(workspace);
    auto P = [&](const char* key) { return m->p(m->enc + key); };
    const TrainCtx cx{s, w + o.scratch, m->train_precision, o.scratch_floats};
    if (m->vitstr) {
        // S - 1 patch rows per image, S token rows: the class token in front (timm _pos_embed), assembled from the patch product in `tmp`
        const int MP = batch * (S - 1);
        CHK(train_patches(m, s, images, images_dtype, u8_table, MP, w + o.patches));
        CHK(lin_fwd(cx, w + o.patches, P("patch_embed.proj.weight"), P("patch_embed.proj.bias"), nullptr, 0, w + o.tmp, MP, E, PK));
        CHK(launch(vitstr_tokens_kernel, dim3(MS), dim3(256), 0, s, w + o.tmp, P("cls_token"), P("pos_embed"), w + o.x(0), S, E));
    } else {
        CHK(train_patches(m, s, images, images_dtype, u8_table, MS, w + o.patches));
        CHK(lin_fwd(cx, w + o.patches, P("patch_embed.proj.weight"), P("patch_embed.proj.bias"), P("pos_embed"), S, w + o.x(0), MS, E, PK));
    }
    m->enc_record_mode = r.record();      // what the record's slots hold; the backward entry must read them the same way
    m->enc_record_ws = workspace;
    if (r.shadows) {
        // this step's weights as bf16, both ways round (the backward entry reads the transposes from the same workspace): one launch over
        // the 4 * depth matrices (it was one launch per matrix: 48 launches of 2 - 7 us)
        CHK(enc_shadow_table(m, o));
        CHK(launch(weight_shadows_kernel, dim3(m->shadow_tiles), dim3(256), 0, s, m->master, reinterpret_cast<const ShadowEntry*>(m->shadow_tab_dev), 4 * depth,
                   reinterpret_cast<bf16_t*>(w + o.w16)));
    }
    if (r.one_launch) {
        // The twelve blocks as ONE launch (encoder_blocks.h record mode): the inference throughput kernel's walk — x resident in the
        // accumulators, the weights streamed from this step's bf16 shadows — writing the record on the way; 48 GEMM, 24 LayerNorm and
        // 12 attention launches and every re-read of an activation disappear, what is left is the record's own bytes.
        CHK(enc_block_table(m, o));
        const EncRecordParams rec{w + o.layer0, o.layer_stride, (unsigned)(o.layer_stride * sizeof(float)), (unsigned)(o.qkv * 4), (unsigned)(o.ao * 4),
                                  (unsigned)(o.x_mid * 4), (unsigned)(o.hpre * 4), (unsigned)(o.hact_l * 4), (unsigned)(o.n1 * 4), (unsigned)(o.n2 * 4)};
        HIPCHK((launch_enc_blocks_record<384>(s, w + o.x_last, reinterpret_cast<const bf16_t*>(w + o.w16), o.w16_layer * (size_t)depth * sizeof(float),
                                              m->master, m->train_blocks_dev, depth, eps, MS, rec)));
    } else {
        const std::vector<EncBlockW> W = enc_block_weights(m, o, r.shadows, nullptr, w);
        for (int i = 0; i < depth; ++i) CHK(enc_block_fwd(cx, m, batch, enc_block_rec(o, w, i, depth, r), W[i]));
    }
    return run_layernorm<float>(s, w + o.x_last, P("norm.weight"), P("norm.bias"), memory_out, nullptr, MS, E, eps);
}
extern "C" int parseq_train_encoder_forward(parseq_model* m, const float* images, int batch, float* memory_out, void* workspace,
                                            size_t workspace_bytes, void* stream) {
    return train_encoder_forward(m, images, PARSEQ_F32, nullptr, batch, memory_out, workspace, workspace_bytes, stream);
}
extern "C" int parseq_train_encoder_forward_ex(parseq_model* m, const void* images, int images_dtype, const float* u8_table, int batch,
                                               float* memory_out, void* workspace, size_t workspace_bytes, void* stream) {
    return train_encoder_forward(m, images, images_dtype, u8_table, batch, memory_out, workspace, workspace_bytes, stream);
}

// ---- gradient segments: the hook for overlapping the data-parallel all-reduce with the encoder's backward -----------------------------
// The reference trains under Lightning's DDP strategy (train.py:65-71): gradient buckets are all-reduced while the backward is still
// running.  Here the gradients live in ONE flat buffer laid out like the master weights — pos_queries | encoder.pos_embed, patch_embed |
// blocks 0 .. depth-1 | encoder.norm | decoder.*, head.*, text_embed.* — and become final in this order: the decoder's part (and
// pos_queries) before the encoder's backward starts, then encoder.norm and the blocks from the last to the first, then pos_embed /
// patch_embed.  Segment k (completion order) is a contiguous range of the buffer; parseq_train_encoder_backward records event k on its
// stream right after the last kernel that writes into it:
//   0: [decoder begin, end)            1: [block depth-1 begin, decoder begin)  (with encoder.norm)
//   1 + j: block depth-1-j, j = 1 .. depth-2          depth: [0, block 0 end)   (pos_queries, pos_embed, patch_embed, block 0)
static int64_t grad_block_begin(const parseq_model* m, int i) { return (int64_t)m->params[m->index.at(enc_block_key(m, i, E_LN1_W))].offset; }
static int grad_segment_range(const parseq_model* m, int k, int64_t* begin, int64_t* end) {
    const int depth = m->cfg.enc_depth;
    if (m->vitstr || depth < 2) return fail(PARSEQ_E_INVALID, "gradient segments are defined for the PARSeq training step (depth >= 2)");
    if (k < 0 || k > depth) return fail(PARSEQ_E_INVALID, "gradient segment %d outside [0, %d]", k, depth);
    const int64_t dec = (int64_t)m->params[m->index.at(train_dec_key(D_SA_IN_W))].offset;
    if (k == 0) { *begin = dec; *end = (int64_t)m->master_elems; }
    else if (k == 1) { *begin = grad_block_begin(m, depth - 1); *end = dec; }
    else if (k < depth) { *begin = grad_block_begin(m, depth - k); *end = grad_block_begin(m, depth - k + 1); }
    else { *begin = 0; *end = grad_block_begin(m, 1); }
    return 0;
}
static int grad_event_record(parseq_model* m, int k, hipStream_t s) {
    while ((int)m->grad_events.size() <= m->cfg.enc_depth) {
        hipEvent_t e;
        HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        m->grad_events.push_back(e);
    }
    HIPCHK(hipEventRecord(m->grad_events[k], s));
    return 0;
}
extern "C" int parseq_train_grad_segments(const parseq_model* m) { return (m && !m->vitstr && m->cfg.enc_depth >= 2) ? m->cfg.enc_depth + 1 : 0; }
extern "C" int parseq_train_grad_segment(parseq_model* m, int index, int64_t* begin, int64_t* end, void** event) {
    if (!m || !begin || !end) return fail(PARSEQ_E_INVALID, "null argument");
    CHK(grad_segment_range(m, index, begin, end));
    if (event) {
        if ((int)m->grad_events.size() <= index || !m->grad_events_valid)
            return fail(PARSEQ_E_STATE, "gradient segment %d: its event does not belong to this step (no parseq_train_encoder_backward has run to its end since the last parseq_train_decoder)", index);
        *event = (void*)m->grad_events[index];
    }
    return 0;
}
extern "C" int parseq_stream_wait_event(void* stream, void* event) {
    if (!event) return fail(PARSEQ_E_INVALID, "null event");
    HIPCHK(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
    return 0;
}

// The backward's gradient buffers in the type the route keeps them in.  Level 2 keeps the gradient of the fc1 output and of q | k | v as
// bf16 alone, and its dW products read the residual-stream gradient through the shadow d_x16 (the fp32 d_x stays: LayerNorm backward adds to it).
//   d_x, d_x16    the residual-stream gradient and its shadow (shadow route); d_x_dy: ... as the dY of a product
//   d_h           the gradient of the fc1 output, then of its pre-activation
//   dqkv, dqkv16  the gradient of q | k | v as the attention kernels address it, and where level 2 has them write bf16; dqkv_dy: as a dY
//   dsum          past 128 tokens only
struct EncBwdBufs { float *d_x, *d_a, *dqkv, *dsum; bf16_t *d_x16, *dqkv16; In d_x_dy, dqkv_dy; Out d_h; };
static EncBwdBufs enc_bwd_bufs(const TrainEncoderLayout& o, float* w, const TrainEncRoute& r) {
    EncBwdBufs g;
    g.d_x = w + o.d_x; g.d_a = w + o.d_a; g.dqkv = w + o.dqkv; g.dsum = r.wide ? w + o.dsum : nullptr;
    g.d_x16 = r.shadows ? reinterpret_cast<bf16_t*>(w + o.d_x16) : nullptr; g.dqkv16 = r.bf16_only ? reinterpret_cast<bf16_t*>(g.dqkv) : nullptr;
    g.d_x_dy = In(r.bf16_only ? nullptr : g.d_x, g.d_x16); g.dqkv_dy = In(r.bf16_only ? nullptr : g.dqkv, g.dqkv16);
    g.d_h = Out(r.bf16_only ? nullptr : w + o.d_h, r.shadows ? reinterpret_cast<bf16_t*>(w + o.d_h16) : nullptr);
    return g;
}

// The caller stream's own side stream and events, created on first use (a step split into micro-batches runs several backwards at once,
// each on its own stream), and the three ways the shadow block orders the two; with `on` false everything runs on the caller's stream
struct SideFork {
    bool on = false; hipStream_t s = nullptr, side = nullptr; hipEvent_t* ev = nullptr;
    int fork(int e) const { if (on) { HIPCHK(hipEventRecord(ev[e], s)); HIPCHK(hipStreamWaitEvent(side, ev[e], 0)); } return 0; }      // the side stream waits for the main one
    int mark(int e) const { if (on) HIPCHK(hipEventRecord(ev[e], side)); return 0; }                                                  // a point on the side stream ...
    int join(int e) const { if (on) HIPCHK(hipStreamWaitEvent(s, ev[e], 0)); return 0; }                                              // ... that the main stream waits for
};
static int train_side_for(parseq_model* m, hipStream_t s, SideFork* out) {
    size_t slot = 0;
    while (slot < m->train_sides.size() && m->train_sides[slot].key != s) ++slot;
    if (slot == m->train_sides.size()) {
        if (slot >= 8) return fail(PARSEQ_E_STATE, "training encoder backward: more than 8 distinct caller streams on one model");
        parseq_model::TrainSide ts;
        ts.key = s;
        HIPCHK(hipStreamCreateWithFlags(&ts.side, hipStreamNonBlocking));
        for (hipEvent_t& e : ts.ev) HIPCHK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        m->train_sides.push_back(ts);
    }
    out->on = true; out->s = s; out->side = m->train_sides[slot].side; out->ev = m->train_sides[slot].ev;
    return 0;
}

// One block of the backward on bf16 shadow operands.  The block's four weight-gradient products run on the side context `cxs`, beside the
// chain dX -> LayerNorm / attention backward -> dX that needs them for nothing.  With two streams each starts when its dY exists (an event
// of the main stream) and is waited for only where the main stream is about to overwrite that dY (the residual-stream gradient's shadow
// d_x16) or closes the block; with one stream (PARSEQ_TRAIN_ONE_STREAM=1, and always at level 1) the side context is the main one and the
// events are skipped.  Same kernels, same operands, same order inside every buffer either way: bit-identical.  The level decides only which
// gradients also exist in fp32 (level 1) and which exist as bf16 only (level 2: the fc1 pre-activation, d q | k | v, and d_x as the dY of
// the dW products).  An error return must not leave weight-gradient kernels running on the side stream behind the caller's back: the
// caller joins the side stream before it reports a failure of this function.
static int enc_block_bwd_shadow(const TrainCtx& cx, const TrainCtx& cxs, const SideFork& fk, const parseq_model* m, int batch, const EncBlockRec& rec,
                                const EncBlockW& W, const EncBwdBufs& g) {
    const int E = m->cfg.embed_dim, F = E * m->cfg.enc_mlp_ratio, MS = batch * m->tokens;
    const float eps = m->cfg.enc_ln_eps;
    CHK(fk.fork(0));                                                                                    // d_x16 of this block exists
    CHK(lin_bwd16_dw(cxs, rec.hact.b16, g.d_x_dy, W.g(E_FC2_W), W.g(E_FC2_B), MS, E, F));
    CHK(fk.mark(4));
    CHK(lin_bwd16_dx(cx, W.s16[LIN_FC2].wt, g.d_x_dy, g.d_h, MS, E, F, rec.hpre));
    CHK(fk.fork(1));                                                                                    // d_h16 exists
    CHK(lin_bwd16_dw(cxs, rec.n2.b16, g.d_h, W.g(E_FC1_W), W.g(E_FC1_B), MS, F, E));
    CHK(lin_bwd16_dx(cx, W.s16[LIN_FC1].wt, g.d_h, g.d_a, MS, F, E));
    CHK(fk.join(4));                                                                                    // fc2's dW has read d_x16
    CHK(ln_bwd(cx, rec.x_mid, W(E_LN2_W), g.d_a, g.d_x, g.d_x, W.g(E_LN2_W), W.g(E_LN2_B), MS, E, eps, g.d_x16));
    CHK(fk.fork(2));                                                                                    // the new d_x16 exists
    CHK(lin_bwd16_dw(cxs, rec.ao_v.b16, g.d_x_dy, W.g(E_PROJ_W), W.g(E_PROJ_B), MS, E, E));
    CHK(fk.mark(5));
    CHK(lin_bwd16_dx(cx, W.s16[LIN_PROJ].wt, g.d_x_dy, g.d_a, MS, E, E));
    TrainAttnArgs ab = enc_attn_args(m, rec.qkv, rec.ao, g.d_a, g.dqkv);
    if (g.dqkv16) { ab.dq16 = g.dqkv16; ab.dk16 = g.dqkv16 + E; ab.dv16 = g.dqkv16 + 2 * E; }
    CHK(train_attn(cx, ab, batch, true, ATT_HD));
    CHK(fk.fork(3));                                                                                    // d q | k | v exists
    CHK(lin_bwd16_dw(cxs, rec.n1.b16, g.dqkv_dy, W.g(E_QKV_W), W.g(E_QKV_B), MS, 3 * E, E));
    CHK(fk.mark(6));
    CHK(lin_bwd16_dx(cx, W.s16[LIN_QKV].wt, g.dqkv_dy, g.d_a, MS, 3 * E, E));
    CHK(fk.join(5));                                                                                    // proj's dW has read d_x16
    CHK(ln_bwd(cx, rec.x, W(E_LN1_W), g.d_a, g.d_x, g.d_x, W.g(E_LN1_W), W.g(E_LN1_B), MS, E, eps, g.d_x16));
    return fk.join(6);        // the block's gradients are final on the main stream too (the segment event that follows covers them)
}
// One block of the backward with every operand fp32 in memory (lin_bwd: its padded path and folded epilogues), one stream
static int enc_block_bwd_f32(const TrainCtx& cx, const parseq_model* m, int batch, const EncBlockRec& rec, const EncBlockW& W, const EncBwdBufs& g) {
    const int E = m->cfg.embed_dim, F = E * m->cfg.enc_mlp_ratio, MS = batch * m->tokens;
    const float eps = m->cfg.enc_ln_eps;
    // x_out = x_mid + fc2(gelu(fc1(norm2(x_mid))))        d_x = d x_out
    CHK(lin_bwd(cx, rec.hact.f32, W(E_FC2_W), g.d_x, W.g(E_FC2_W), W.g(E_FC2_B), g.d_h.f32, MS, E, F, rec.hpre.f32));      // d_h = d hpre (GELU backward folded in)
    CHK(lin_bwd(cx, rec.n2.f32, W(E_FC1_W), g.d_h.f32, W.g(E_FC1_W), W.g(E_FC1_B), g.d_a, MS, F, E));
    CHK(ln_bwd(cx, rec.x_mid, W(E_LN2_W), g.d_a, g.d_x, g.d_x, W.g(E_LN2_W), W.g(E_LN2_B), MS, E, eps));                   // d_x = d x_mid
    // x_mid = x + proj(attention(qkv(norm1(x))))
    CHK(lin_bwd(cx, rec.ao_v.f32, W(E_PROJ_W), g.d_x, W.g(E_PROJ_W), W.g(E_PROJ_B), g.d_a, MS, E, E));                     // d_a = d ao
    CHK(train_attn(cx, enc_attn_args(m, rec.qkv, rec.ao, g.d_a, g.dqkv, rec.lse, rec.lse ? g.dsum : nullptr), batch, true, ATT_HD));
    CHK(lin_bwd(cx, rec.n1.f32, W(E_QKV_W), g.dqkv, W.g(E_QKV_W), W.g(E_QKV_B), g.d_a, MS, 3 * E, E));
    return ln_bwd(cx, rec.x, W(E_LN1_W), g.d_a, g.d_x, g.d_x, W.g(E_LN1_W), W.g(E_LN1_B), MS, E, eps);                     // d_x = d x
}

extern "C" int parseq_train_encoder_backward(parseq_model* m, const float* dmemory, int batch, float* grads, void* workspace, size_t workspace_bytes,
                                             void* stream) {
    if (!dmemory || !grads) return fail(PARSEQ_E_INVALID, "null argument");
    CHK(train_encoder_check(m, batch, workspace, workspace_bytes));
    DevGuard dg(m->device);
    const TrainEncoderLayout o = train_encoder_layout(m, batch);
    const TrainEncRoute r = train_enc_route(m, o);
    if (m->enc_record_ws == workspace && m->enc_record_mode != r.record())
        return fail(PARSEQ_E_STATE, "training encoder backward: the record in this workspace was written in mode %d, this call would read it in mode %d "
                    "(PARSEQ_TRAIN_NO_SHADOWS / PARSEQ_TRAIN_SHADOW_LEVEL / train precision changed between forward and backward)", (int)m->enc_record_mode,
                    (int)r.record());
    hipStream_t s = (hipStream_t)stream;
    const int E = m->cfg.embed_dim, S = m->tokens, MS = batch * S, PK = m->patch_k, depth = m->cfg.enc_depth;
    const float eps = m->cfg.enc_ln_eps;
    float* w = reinterpret_cast<float*>(workspace);
    auto top = [&](const char* key) { return param_ref(m, m->enc + key, grads); };      // the encoder's parameters outside the blocks
    const TrainCtx cx{s, w + o.scratch, m->train_precision, o.scratch_floats};
    const EncBwdBufs g = enc_bwd_bufs(o, w, r);
    const bool segs = !m->vitstr && depth >= 2;
    SideFork fk;
    if (r.two_streams) CHK(train_side_for(m, s, &fk));
    // the context of the shadow block's weight-gradient products: the side stream and its scratch, or with one stream the main context
    const TrainCtx cxs = r.two_streams ? TrainCtx{fk.side, w + o.scratch2, cx.ops, o.scratch_floats} : cx;
    const std::vector<EncBlockW> W = enc_block_weights(m, o, r.shadows, grads, w);
    m->grad_events_valid = false;
    if (segs) CHK(grad_event_record(m, 0, s));      // the decoder's gradients were written by parseq_train_decoder, earlier on this stream
    const ParamRef norm_w = top("norm.weight");
    CHK(ln_bwd(cx, w + o.x_last, norm_w.p, dmemory, nullptr, g.d_x, norm_w.g, top("norm.bias").g, MS, E, eps, g.d_x16));
    for (int i = depth - 1; i >= 0; --i) {
        // block i + 1 (and, behind the last block, encoder.norm) is final: segment depth - 1 - i
        if (segs && i < depth - 1) CHK(grad_event_record(m, depth - 1 - i, s));
        const EncBlockRec rec = enc_block_rec(o, w, i, depth, r);
        if (!r.shadows) { CHK(enc_block_bwd_f32(cx, m, batch, rec, W[i], g)); continue; }
        if (const int rc = enc_block_bwd_shadow(cx, cxs, fk, m, batch, rec, W[i], g)) {
            if (fk.on) (void)hipStreamSynchronize(fk.side);      // whatever was enqueued there has finished with `grads` and the workspace before the caller hears of the failure
            return rc;
        }
    }
    CHK(colsum(cx, g.d_x, (long)S * E, batch, S * E, top("pos_embed").g, true));
    const ParamRef pe_w = top("patch_embed.proj.weight");
    float* pe_db = top("patch_embed.proj.bias").g;
    if (m->vitstr) {
        // d cls_token = sum over the images of row 0; the patch embedding sees rows 1 .. S - 1 only (gathered into `tmp`)
        const int MP = batch * (S - 1);
        CHK(colsum(cx, g.d_x, (long)S * E, batch, E, top("cls_token").g, true));
        CHK(launch(gather_image_rows_kernel, dim3(MP), dim3(256), 0, s, g.d_x, S, 1, w + o.tmp, S - 1, E));
        CHK(lin_bwd(cx, w + o.patches, pe_w.p, w + o.tmp, pe_w.g, pe_db, nullptr, MP, E, PK));
    } else {
        CHK(lin_bwd(cx, w + o.patches, pe_w.p, g.d_x, pe_w.g, pe_db, nullptr, MS, E, PK));
    }
    if (segs) CHK(grad_event_record(m, depth, s));      // block 0, patch_embed, pos_embed (and pos_queries): everything is final
    m->grad_events_valid = segs;
    return 0;
}

// ---- training step, ViTSTR head and loss (strhub/models/base.py:194-204 forward_logits_loss, vitstr/system.py:75-82) ------------------
// logits of tokens 1 .. T of every image (the class token's row is computed by the reference and dropped), cross-entropy over
// C = num_classes with ignore_index = <pad>, mean over the kept targets; backward into head.* and d memory (zero on row 0 and past T).
struct VitstrHeadLayout { size_t hin, logits, dh, row_loss, counts, scratch, scratch_floats, total; };
static VitstrHeadLayout vitstr_head_layout(const parseq_model* m, int B, int T) {
    const size_t E = m->cfg.embed_dim, C = m->classes, R = (size_t)B * T;
    VitstrHeadLayout o;
    Take take;
    o.hin = take(R * E); o.logits = take(R * C); o.dh = take(R * E); o.row_loss = take(R); o.counts = take(1);
    o.scratch_floats = train_scratch_floats(R, E); o.scratch = take(o.scratch_floats);
    o.total = take.off;
    return o;
}
extern "C" size_t parseq_train_vitstr_head_workspace_bytes(const parseq_model* m, int batch, int T) {
    if (!m || batch <= 0 || T <= 0) return 0;
    return vitstr_head_layout(m, batch, T).total * sizeof(float);
}
extern "C" int parseq_train_vitstr_head(parseq_model* m, const float* memory, const int32_t* targets, int batch, int T, int total_targets,
                                        float* loss_out, float* grads, float* dmemory, void* workspace, size_t workspace_bytes, void* stream) {
    if (!m || !memory || !targets || !loss_out || !grads || !dmemory || !workspace) return fail(PARSEQ_E_INVALID, "null argument");
    if (!m->vitstr) return fail(PARSEQ_E_INVALID, "parseq_train_vitstr_head on a PARSeq model (arch 0): use parseq_train_decoder");
    const int S = m->tokens;
    if (batch <= 0 || T < 1 || T > m->cfg.max_label_length + 1 || T + 1 > S || total_targets <= 0)
        return fail(PARSEQ_E_INVALID, "bad shape: batch %d, %d target positions (1..%d), %d targets", batch, T, m->cfg.max_label_length + 1, total_targets);
    CHK(require_params_set(m));
    const VitstrHeadLayout o = vitstr_head_layout(m, batch, T);
    if (workspace_bytes < o.total * sizeof(float)) return fail(PARSEQ_E_INVALID, "workspace: %zu bytes given, %zu needed", workspace_bytes, o.total * sizeof(float));
    DevGuard dg(m->device);
    hipStream_t s = (hipStream_t)stream;
    const int E = m->cfg.embed_dim, C = m->classes, R = batch * T;
    float* w = reinterpret_cast<float*>(workspace);
    const ParamRef head_w = param_ref(m, "head.weight", grads), head_b = param_ref(m, "head.bias", grads);
    const TrainCtx cx{s, w + o.scratch, m->train_precision, o.scratch_floats};
    CHK(launch(gather_image_rows_kernel, dim3(R), dim3(256), 0, s, memory, S, 1, w + o.hin, T, E));
    CHK(lin_fwd(cx, w + o.hin, head_w.p, head_b.p, nullptr, 0, w + o.logits, R, C, E));
    CHK(ce_loss_and_grad(s, w + o.logits, targets, 1, R, C, m->cfg.pad_id, w + o.row_loss, loss_out, reinterpret_cast<int*>(w + o.counts), total_targets));
    CHK(lin_bwd(cx, w + o.hin, head_w.p, w + o.logits, head_w.g, head_b.g, w + o.dh, R, C, E));
    return launch(scatter_image_rows_kernel, dim3(batch * S), dim3(256), 0, s, w + o.dh, T, 1, dmemory, S, E);
}

// ---- training step, optimiser ---------------------------------------------------------------------------------------------
extern "C" int parseq_grad_norm(const float* grads, int64_t n, float* norm_out, float* workspace, void* stream) {
    if (!grads || !norm_out || !workspace || n <= 0) return fail(PARSEQ_E_INVALID, "null / empty argument");
    hipStream_t s = (hipStream_t)stream;
    CHK(launch(sumsq_partial_kernel, dim3(SUMSQ_BLOCKS), dim3(256), 0, s, grads, (size_t)n, workspace));
    return launch(sumsq_final_kernel, dim3(1), dim3(256), 0, s, workspace, norm_out);
}

extern "C" int parseq_adamw_step(parseq_model* m, const float* grads, float* exp_avg, float* exp_avg_sq, const int32_t* decay_flags, float lr,
                                 float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_norm, float max_norm,
                                 void* stream) {
    if (!m || !grads || !exp_avg || !exp_avg_sq) return fail(PARSEQ_E_INVALID, "null argument");
    if (step < 1) return fail(PARSEQ_E_INVALID, "step %d: steps count from 1", step);
    DevGuard dg(m->device);
    CHK(require_params_set(m));
    hipStream_t s = (hipStream_t)stream;
    const float bc1 = 1.0f - powf(beta1, (float)step), bc2_sqrt = sqrtf(1.0f - powf(beta2, (float)step));
    // runs of consecutive tensors with the same weight-decay flag are one launch (with weight_decay == 0, the reference's
    // configuration, the whole buffer is)
    const int np = (int)m->params.size();
    int i = 0;
    while (i < np) {
        const bool decay = decay_flags && weight_decay != 0.f && decay_flags[i];
        int j = i + 1;
        while (j < np && (decay_flags && weight_decay != 0.f && decay_flags[j]) == decay) ++j;
        const size_t lo = m->params[i].offset, hi = j < np ? m->params[j].offset : m->master_elems;
        CHK(launch(adamw_kernel, dim3((unsigned)((hi - lo + 255) / 256)), dim3(256), 0, s, m->master + lo, grads + lo, exp_avg + lo, exp_avg_sq + lo, hi - lo, lr,
                   beta1, beta2, eps, decay ? weight_decay : 0.f, bc1, bc2_sqrt, grad_norm, max_norm));
        i = j;
    }
    m->version++;
    return 0;
}

// Stochastic weight averaging: one grid-stride launch over the flat buffer (train_rows.h weights_average_kernel)
extern "C" int parseq_op_weights_average(const float* weights, float* avg, int64_t n, int64_t n_averaged, void* stream) {
    if (!weights || !avg || n <= 0 || n_averaged < 0) return fail(PARSEQ_E_INVALID, "null / empty argument or a negative count");
    const int vec = (reinterpret_cast<uintptr_t>(weights) | reinterpret_cast<uintptr_t>(avg)) % 16 == 0;
    const unsigned blocks = (unsigned)std::min<int64_t>(AVERAGE_BLOCKS, (n + 1023) / 1024);
    return launch(weights_average_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)stream, weights, avg, (size_t)n, n_averaged == 0 ? 1 : 0,
                  (float)(n_averaged + 1), vec);
}
extern "C" int parseq_weights_average(parseq_model* m, float* avg, int64_t n_averaged, void* stream) {
    if (!m || !avg) return fail(PARSEQ_E_INVALID, "null argument");
    CHK(require_params_set(m));
    DevGuard dg(m->device);
    return parseq_op_weights_average(m->master, avg, (int64_t)m->master_elems, n_averaged, stream);
}
// The whole flat buffer back into the master weights (the averaged weights at the end of training): the mirror of parseq_model_get_params
extern "C" int parseq_model_set_params(parseq_model* m, const float* flat, void* stream) {
    if (!m || !flat) return fail(PARSEQ_E_INVALID, "null argument");
    DevGuard dg(m->device);
    HIPCHK(hipMemcpyAsync(m->master, flat, m->master_elems * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    for (ParamSpec& ps : m->params) ps.set = true;
    m->version++;
    return 0;
}

extern "C" int parseq_model_get_param(const parseq_model* m, const char* key, float* device_ptr, int64_t numel, void* stream) {
    if (!m || !key || !device_ptr) return fail(PARSEQ_E_INVALID, "null argument");
    auto it = m->index.find(key);
    if (it == m->index.end()) return fail(PARSEQ_E_INVALID, "unknown parameter key '%s'", key);
    const ParamSpec& ps = m->params[it->second];
    if (ps.numel != numel) return fail(PARSEQ_E_INVALID, "parameter %s: numel %lld, expected %lld", key, (long long)numel, (long long)ps.numel);
    DevGuard dg(m->device);
    HIPCHK(hipMemcpyAsync(device_ptr, m->master + ps.offset, (size_t)numel * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return 0;
}

// Every parameter out in ONE launch (the per-tensor form above is ~170 small device copies per optimiser step: 0.6 ms of a 34 ms step).
// The table of copy pieces is rebuilt only when the destination pointers change (never, in a training loop).
extern "C" int parseq_model_get_params(parseq_model* m, float* const* device_ptrs, int count, void* stream) {
    if (!m || !device_ptrs) return fail(PARSEQ_E_INVALID, "null argument");
    if (count != (int)m->params.size()) return fail(PARSEQ_E_INVALID, "%d destination pointers for %d parameters", count, (int)m->params.size());
    for (int i = 0; i < count; ++i) if (!device_ptrs[i]) return fail(PARSEQ_E_INVALID, "parameter %s: null destination", m->params[i].key.c_str());
    DevGuard dg(m->device);
    hipStream_t s = (hipStream_t)stream;
    if (!m->out_chunks || m->out_ptrs.size() != (size_t)count || !std::equal(m->out_ptrs.begin(), m->out_ptrs.end(), device_ptrs)) {
        std::vector<CopyPiece> pieces;
        for (int i = 0; i < count; ++i) {
            const ParamSpec& ps = m->params[i];
            for (int64_t at = 0; at < ps.numel; at += COPY_PIECE_ELEMS)
                pieces.push_back(CopyPiece{m->master + ps.offset + at, device_ptrs[i] + at, (int)std::min<int64_t>(COPY_PIECE_ELEMS, ps.numel - at)});
        }
        HIPCHK(hipStreamSynchronize(s));      // a launch that still reads the old table
        if (m->out_chunks) { (void)hipFree(m->out_chunks); m->out_chunks = nullptr; }
        HIPCHK(hipMalloc(&m->out_chunks, pieces.size() * sizeof(CopyPiece)));
        HIPCHK(hipMemcpy(m->out_chunks, pieces.data(), pieces.size() * sizeof(CopyPiece), hipMemcpyHostToDevice));
        m->out_chunk_count = (int)pieces.size();
        m->out_ptrs.assign(device_ptrs, device_ptrs + count);
    }
    return launch(copy_pieces_kernel, dim3((unsigned)m->out_chunk_count), dim3(256), 0, s, reinterpret_cast<const CopyPiece*>(m->out_chunks));
}

// -------------------------------------------------------------------------------------------------------------------
// input resize
