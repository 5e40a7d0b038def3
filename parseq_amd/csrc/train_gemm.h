// The matrix products of the training step: every kernel takes one SgemmArgs and computes
//   C (+)= alpha * A B + bias + R[m % rper]   with strided operands, so one description covers X W^T (forward, dX) and dY^T X (dW).
//   sgemm_kernel          fp32 on the VALU, any shape and stride: the route of last resort
//   mfma_sgemm_kernel     fp32 on the matrix cores (exact 16x16x4 products), whole 128 x 128 tiles
//   mfma_bgemm_kernel     the bf16-operand mode: fp32 (or one bf16 shadow) operand in memory, rounded to bf16 on the way into LDS, with
//                         bg_epilogue's folded row sums, GELU, GELU backward and bf16 second outputs
//   mfma_x3gemm_kernel    the bf16x3 mode: each fp32 operand split into a bf16 (hi, lo) pair, three products per term
//   mfma_bgemm16_kernel / mfma_bgemm16t_kernel    both operands bf16 shadows, 64-deep stages (k-contiguous / outer-contiguous)
//   splitk_reduce_kernel  folds the split-K partials of all of the above, in a fixed order
// and beside them what the products' callers need: weight_shadows_kernel (the bf16 copies of the weights, one launch), pad_copy_kernel
// and add_into_kernel (the zero-padded operands of a product whose width is no multiple of 4).
// Matrices are row-major; accumulation is fp32 everywhere; kernels that accumulate into their output say so; nothing uses atomics, so
// every result is bit-identical from run to run.  Which kernel a product takes is lib_train.hip's sgemm().
#pragma once
#include "common.h"
#include <type_traits>

namespace pq {


// -------------------------------------------------------------------------------------------------------------------
// C[m][n] (+)= alpha * sum_k A(m, k) * B(k, n) + bias[n] + R[m % rper][n]
// A(m, k) = A[m * sam + k * sak], B(k, n) = B[k * sbk + n * sbn]: one kernel covers X W^T (forward, dX) and dY^T X (dW).
// -------------------------------------------------------------------------------------------------------------------
struct SgemmArgs {
    const float* A; long sam, sak;
    const float* B; long sbk, sbn;
    const float* bias;                   // [N] or nullptr
    const float* R; long ldr; int rper;  // residual rows (row m reads R[(m % rper) * ldr + n]) or nullptr
    float* C; long ldc;
    int M, N, K;
    float alpha;
    int accumulate;                      // C += ... instead of C = ...
    float* asum;                         // [M] += sum_k A(m, k) (fp32, before any rounding) or nullptr: the bias gradient riding on the dW
                                         // product dY^T X (A = dY^T), which streams dY anyway — mfma_bgemm_kernel only
    const float* gelu_pre;               // [M][ldc] or nullptr: the stored value is multiplied by gelu'(gelu_pre[m][n]) — the GELU backward
                                         // riding on the dX product through fc2 (d hpre = (dY W2) * gelu'(hpre)) — mfma_bgemm_kernel only
    float* gelu_out;                     // [M][ldc] or nullptr: gelu(stored value) is written here as well (fc1: pre-activation AND activation from one
                                         // epilogue) — mfma_bgemm_kernel only
    // bf16 SHADOW operands (round 3; the matrix-core kernels of the bf16-operand mode only): the producer of an activation writes it as
    // bfloat16 — the same round-to-nearest-even the operand loaders applied on the way into LDS, so the products are bit-identical — and
    // the GEMM reads half the bytes with nothing to convert.  a16 / b16: A / B point at bf16_t data (strides in elements).
    int a16, b16;
    bf16_t* c16;                         // [M][ldc] or nullptr: the stored value again, rounded to bf16 (the next product's operand)
    bf16_t* gelu_out16;                  // [M][ldc] or nullptr: gelu(stored value) as bf16 (instead of gelu_out)
    // bf16-ONLY storage (the step's default in the bf16-operand mode, what bf16-mixed autocast keeps of a Linear output): C may be nullptr
    // when c16 is given — the fp32 copy of the result is not written at all — and the GELU backward can read its pre-activation as bf16
    const bf16_t* gelu_pre16;            // [M][ldc] or nullptr: as gelu_pre, from the bf16 copy of the pre-activation
};
__device__ __forceinline__ float bf16_lo(unsigned w) { return __uint_as_float(w << 16); }
__device__ __forceinline__ float bf16_hi(unsigned w) { return __uint_as_float(w & 0xffff0000u); }

constexpr int SG_BM = 64, SG_BN = 64, SG_BK = 16;

static __global__ __launch_bounds__(256)
void sgemm_kernel(const SgemmArgs a) {
    __shared__ float As[SG_BK][SG_BM + 4];
    __shared__ float Bs[SG_BK][SG_BN + 4];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.y * SG_BM, n0 = blockIdx.x * SG_BN;
    const int tm = (tid >> 4) * 4, tn = (tid & 15) * 4;
    const bool a_kfast = a.sak == 1, b_nfast = a.sbn == 1;      // walk the contiguous axis with consecutive threads
    float acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;
    for (int k0 = 0; k0 < a.K; k0 += SG_BK) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int idx = tid + 256 * i;
            const int am = a_kfast ? idx / SG_BK : idx % SG_BM, ak = a_kfast ? idx % SG_BK : idx / SG_BM;
            const int gm = m0 + am, gk = k0 + ak;
            As[ak][am] = (gm < a.M && gk < a.K) ? a.A[(size_t)gm * a.sam + (size_t)gk * a.sak] : 0.f;
            const int bn = b_nfast ? idx % SG_BN : idx / SG_BK, bk = b_nfast ? idx / SG_BN : idx % SG_BK;
            const int gn = n0 + bn, gk2 = k0 + bk;
            Bs[bk][bn] = (gn < a.N && gk2 < a.K) ? a.B[(size_t)gk2 * a.sbk + (size_t)gn * a.sbn] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int kk = 0; kk < SG_BK; ++kk) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { av[i] = As[kk][tm + i]; bv[i] = Bs[kk][tn + i]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
        }
        __syncthreads();
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int gm = m0 + tm + i;
        if (gm >= a.M) continue;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int gn = n0 + tn + j;
            if (gn >= a.N) continue;
            float v = a.alpha * acc[i][j];
            if (a.bias) v += a.bias[gn];
            if (a.R) v += a.R[(size_t)(gm % a.rper) * a.ldr + gn];
            float* c = a.C + (size_t)gm * a.ldc + gn;
            *c = a.accumulate ? *c + v : v;
        }
    }
}

// The same contraction on the matrix cores (v_mfma_f32_16x16x4_f32: exact fp32 products, fp32 accumulate) for the shapes that
// carry the step's FLOPs: M % 128 == 0, N % 128 == 0, K % 16 == 0, 16-byte aligned rows.  128 x 128 block tile, four waves of
// 64 x 64, 16 of K per LDS stage, operands parked k-major in LDS (As[k][m], Bs[k][n]) so that a lane's MFMA operand is one
// ds_read_b32 and either memory orientation of A / B (k- or m/n-contiguous) is loaded with 16-byte accesses.
// blockIdx.z splits K (the dW contractions run over batch * tokens rows but have few output tiles): split z handles
// [z * k_chunk, +k_chunk) and, when gridDim.z > 1, writes its tile to partial[z][M][N]; splitk_reduce_kernel folds them in a
// fixed order (deterministic).  bias / residual / accumulate are applied by whichever kernel writes C.
constexpr int MG_BM = 128, MG_BN = 128, MG_BK = 16, MG_LD = 128 + 16;

__device__ __forceinline__ void mg_load_tile(const float* __restrict__ base, long s_outer, long s_k, int outer0, int k0, bool k_fast,
                                            float (*tile)[MG_LD], int tid) {
    // tile[k][o] = base[(outer0 + o) * s_outer + (k0 + k) * s_k]   for o < 128, k < 16; one of s_outer / s_k is 1
#pragma unroll
    for (int it = 0; it < 2; ++it) {
        if (k_fast) {
            const int o = tid & 127, k4 = (tid >> 7) + 2 * it;             // 4 consecutive k of one row
            const float4 v = *reinterpret_cast<const float4*>(base + (size_t)(outer0 + o) * s_outer + k0 + 4 * k4);
            tile[4 * k4 + 0][o] = v.x; tile[4 * k4 + 1][o] = v.y; tile[4 * k4 + 2][o] = v.z; tile[4 * k4 + 3][o] = v.w;
        } else {
            const int o4 = tid & 31, k = (tid >> 5) + 8 * it;              // 4 consecutive rows of one k
            const float4 v = *reinterpret_cast<const float4*>(base + (size_t)(k0 + k) * s_k + outer0 + 4 * o4);
            *reinterpret_cast<float4*>(&tile[k][4 * o4]) = v;
        }
    }
}

static __global__ __launch_bounds__(256)
void mfma_sgemm_kernel(const SgemmArgs a, int k_chunk, float* __restrict__ partial) {
    __shared__ __attribute__((aligned(16))) float As[MG_BK][MG_LD];
    __shared__ __attribute__((aligned(16))) float Bs[MG_BK][MG_LD];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int m0 = blockIdx.y * MG_BM, n0 = blockIdx.x * MG_BN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r16 = lane & 15, g = lane >> 4;
    const bool a_kfast = a.sak == 1, b_kfast = a.sbk == 1;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kbeg = blockIdx.z * k_chunk, kend = min(a.K, kbeg + k_chunk);
    for (int k0 = kbeg; k0 < kend; k0 += MG_BK) {
        mg_load_tile(a.A, a.sam, a.sak, m0, k0, a_kfast, As, tid);
        mg_load_tile(a.B, a.sbn, a.sbk, n0, k0, b_kfast, Bs, tid);
        __syncthreads();
#pragma unroll
        for (int ks = 0; ks < MG_BK / 4; ++ks) {
            float av[4], bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) { av[i] = As[4 * ks + g][wm + 16 * i + r16]; bv[i] = Bs[4 * ks + g][wn + 16 * i + r16]; }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[i], bv[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }
    // lane holds D[row = 16 i + 4 g + r][col = 16 j + r16]
    const bool direct = gridDim.z == 1;
    float* out = direct ? a.C : partial + (size_t)blockIdx.z * a.M * a.N;
    const long ldo = direct ? a.ldc : a.N;
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gm = m0 + wm + 16 * i + 4 * g + r;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int gn = n0 + wn + 16 * j + r16;
                float v = acc[i][j][r];
                float* c = out + (size_t)gm * ldo + gn;
                if (direct) {
                    v *= a.alpha;
                    if (a.bias) v += a.bias[gn];
                    if (a.R) v += a.R[(size_t)(gm % a.rper) * a.ldr + gn];
                    if (a.accumulate) v += *c;
                }
                *c = v;
            }
        }
}

// The same contraction with bf16 OPERANDS (every element of A and B rounded to bfloat16, round-to-nearest-even, on its way into LDS),
// fp32 products and accumulation on v_mfma_f32_16x16x32_bf16, fp32 master data in memory: the training step's "bf16" mode
// (BASELINE configs[4] trains bf16-mixed; the gate is oracle.decoder_backward.rounding('bf16'): cosine >= 0.9996 per gradient tensor).
// K % 32 == 0; M and N arbitrary (edge tiles: see bg_fetch).  128 x 128 block tile, four waves of 64 x 64, 32 of K per stage; operands sit in LDS as
// [outer][k] bf16 rows of 80 bytes (64 + 16 pad: the 16 lanes of a ds_read_b128 group fall on distinct banks), so a lane's MFMA operand
// is one ds_read_b128 whichever way the matrix lies in memory; two LDS stages, the next stage's global loads are issued before the
// current stage's MFMAs and converted / stored after them (one barrier per stage).  Split-K and epilogue exactly as mfma_sgemm_kernel.
constexpr int BG_BK = 32, BG_LD = 40;       // elements

// Tiles may hang over the edge of the matrix: over-the-edge lanes re-read the last valid row (k-contiguous operand) or the last valid
// group of four (outer-contiguous operand; the outer extent is a multiple of 4 there) and their products land in accumulator rows /
// columns the epilogue does not store.
// Round 3 (profiles/r03_train_gemm_counters_v0.md: 60 % of the wave cycles parked at s_waitcnt, 10 VALU instructions per MFMA, L2 hit
// rate 42 % with 1.4-3x the algorithmic bytes fetched from HBM):
//   * the kernel is a template on the two operand orientations and every thread's four source pointers per operand are computed ONCE
//     — the loop body used to redo 64-bit index arithmetic with clamps per load behind a run-time orientation branch, and the
//     register shuffling that came with it made the compiler wait for five of the eight loads of stage k + 1 BEFORE the MFMAs of stage
//     k (the disassembly showed `s_waitcnt vmcnt(7)`, `vmcnt(3)` ahead of the first MFMA): the prefetch hid nothing;
//   * XCD-aware tile order: the hardware deals consecutive workgroup ids to the eight XCDs (private L2s) round-robin, so the N-tiles
//     that share an A row panel all landed on different XCDs and each fetched the panel from HBM for itself.  Workgroup id L now maps to
//     logical id (L % 8) * (total / 8) + L / 8 and logical ids walk the N-tiles of one row panel first: a panel's consumers share an L2.
template <bool KFAST, typename T = float>
struct BgOperand {
    static constexpr bool HALF = sizeof(T) == 2;                 // bf16 shadow operand: loaded and parked as it is
    static constexpr int NL = (KFAST && HALF) ? 2 : 4;           // loads per thread and stage
    using V = std::conditional_t<!HALF, float4, std::conditional_t<KFAST, u32x4, u32x2>>;      // native vectors: HIP's uint4 / uint2 structs in an array end up in scratch
    const T* p[NL];               // this thread's loads of the current stage
    long step;                    // pointer increment per 32-deep stage
    __device__ __forceinline__ void init(const T* __restrict__ base, long s_outer, long s_k, int outer0, int limit, int k0, int tid) {
#pragma unroll
        for (int it = 0; it < NL; ++it) {
            if constexpr (KFAST && !HALF) {         // rows of 32 consecutive k: thread = (row idx >> 3, 4 consecutive k at 4 (idx & 7))
                const int idx = tid + 256 * it, o = min(outer0 + (idx >> 3), limit - 1);
                p[it] = base + (size_t)o * s_outer + k0 + 4 * (idx & 7);
            } else if constexpr (KFAST) {           // bf16 rows of 32 k = 64 bytes: thread = (row idx >> 2, 8 consecutive k at 8 (idx & 3))
                const int idx = tid + 256 * it, o = min(outer0 + (idx >> 2), limit - 1);
                p[it] = base + (size_t)o * s_outer + k0 + 8 * (idx & 3);
            } else {                                 // four CONSECUTIVE k of the same four outer indices per thread
                const int k = 4 * (tid >> 5) + it, o = min(outer0 + 4 * (tid & 31), limit - 4);
                p[it] = base + (size_t)(k0 + k) * s_k + o;
            }
        }
        step = KFAST ? (long)BG_BK : (long)BG_BK * s_k;
    }
    __device__ __forceinline__ void fetch(V (&r)[NL]) {
#pragma unroll
        for (int it = 0; it < NL; ++it) { r[it] = *reinterpret_cast<const V*>(p[it]); p[it] += step; }
    }
    static __device__ __forceinline__ void park(bf16_t (*tile)[BG_LD], const V (&r)[NL], int tid) {
        if constexpr (KFAST && !HALF) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                const int idx = tid + 256 * it, o = idx >> 3, k4 = idx & 7;
                union { uint2 u; bf16_t e[4]; } h;
                h.e[0] = static_cast<bf16_t>(r[it].x); h.e[1] = static_cast<bf16_t>(r[it].y); h.e[2] = static_cast<bf16_t>(r[it].z); h.e[3] = static_cast<bf16_t>(r[it].w);
                *reinterpret_cast<uint2*>(&tile[o][4 * k4]) = h.u;
            }
        } else if constexpr (KFAST) {
#pragma unroll
            for (int it = 0; it < 2; ++it) {
                const int idx = tid + 256 * it;
                *reinterpret_cast<u32x4*>(&tile[idx >> 2][8 * (idx & 3)]) = r[it];
            }
        } else if constexpr (!HALF) {
            // r[it] = four outer indices (4 o4 .. 4 o4 + 3) at k = 4 kq + it: transposed in registers, one 8-byte store per outer index
            // (these stores conflict 8-way in LDS — rows four apart are 16 banks apart; rotating each lane's row order made them 2-way and
            // changed nothing measurable: the dW products are not bound by it)
            const int kq = tid >> 5, o4 = tid & 31;
            const float v[4][4] = {{r[0].x, r[0].y, r[0].z, r[0].w}, {r[1].x, r[1].y, r[1].z, r[1].w}, {r[2].x, r[2].y, r[2].z, r[2].w}, {r[3].x, r[3].y, r[3].z, r[3].w}};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                union { uint2 u; bf16_t e[4]; } h;
#pragma unroll
                for (int it = 0; it < 4; ++it) h.e[it] = static_cast<bf16_t>(v[it][i]);
                *reinterpret_cast<uint2*>(&tile[4 * o4 + i][4 * kq]) = h.u;
            }
        } else {
            // the same 4 x 4 transposition on 16-bit values: r[it] = {lo 16 bits of .x: outer 0, hi: outer 1, .y: outer 2, 3} at k = 4 kq + it
            const int kq = tid >> 5, o4 = tid & 31;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                unsigned e[4];
#pragma unroll
                for (int it = 0; it < 4; ++it) { const unsigned w = (i & 2) ? r[it].y : r[it].x; e[it] = (i & 1) ? (w >> 16) : (w & 0xffffu); }
                *reinterpret_cast<u32x2*>(&tile[4 * o4 + i][4 * kq]) = u32x2{e[0] | (e[1] << 16), e[2] | (e[3] << 16)};
            }
        }
    }
};

// Epilogue of the bf16-operand kernels.  Lane holds D[row = 16 i + 4 g + r][col = 16 j + r16] of its wave's 64 x 64 quarter.
//
// Staged form (round 3, the usual case): the accumulators go through LDS — the operand tiles are dead — 64 rows at a time, and come back
// as 16-byte row pieces: 32 lanes write 512 contiguous bytes of a row of C (and read the residual / old-C / GELU rows the same way),
// the bf16 shadows leave as 8-byte pieces.  The direct form below it (one 4-byte access per lane and element, 16 lanes = 64 bytes per row
// and instruction, 64 store instructions per lane and output) ran the products whose output is large at 1-2 TB/s of C — the stores, not
// the operand traffic, were what bounded them (49 152 x 1536: 302 MB of C in 169 us; with a second, 2-byte shadow store per element
// 229 us).  Same arithmetic in the same order: (alpha acc + ((bias + residual) + old C)) * gelu'(pre).
// The direct form remains for outputs that are not 16-byte addressable (the 95-class head) and for edge tiles in N.
constexpr int EP_LD = 132;       // floats per staged row: 128 + 4 (the four row groups of a store land on distinct banks)
constexpr int EP_STAGE_BYTES = 64 * EP_LD * 4;
__device__ __forceinline__ bool ep_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
// XCD-aware order of the workgroups of a launch.  The hardware deals consecutive workgroup ids (x fastest, then z) to the eight XCDs
// round-robin; id L is mapped to the logical id (L % 8) * (T / 8) + L / 8 so that ONE XCD walks a contiguous range of logical ids, and logical
// ids walk the N-tiles of a row panel first, then the row panels (a panel's consumers share an L2).  The tail that does not fill a group of
// eight keeps its id.
// SPLIT_AWARE (round 3, second half; the fp32-operand kernel): the split index is part of the walk — logical ids walk the tiles of split 0, then
// of split 1, ... — because the tiles of one split all read the same k range of both operands and, spread over eight XCDs, every private L2
// fetched that range for itself.  Counters per dW launch, before -> after: fp32 operands (the decoder's) 673 -> 290 MB from HBM (184 MB of
// operands) and 124 -> 106 us; all-bf16 (the encoder's, mfma_bgemm16t_kernel) 472 -> 222 MB (190 MB of operands) but 102 -> 109 us — that kernel
// was not waiting on HBM, and eight XCDs each serving an eighth of every split's tiles spread its L2 reads better — so the all-bf16 kernels
// keep the split in blockIdx.z (profiles/r03_train_pmc_hbm_traffic.md, r03_train_pmc_fetch_after.md).
struct BgTile { int tm, tn, z; };
template <bool SPLIT_AWARE>
__device__ __forceinline__ BgTile bg_tile(int gn, int gm) {
    const int total = gn * gm;
    const int T = SPLIT_AWARE ? total * (int)gridDim.z : total, L = (int)blockIdx.x + (SPLIT_AWARE ? total * (int)blockIdx.z : 0), whole = T & ~7;
    const int logical = L < whole ? (L & 7) * (whole >> 3) + (L >> 3) : L;
    BgTile t;
    t.z = SPLIT_AWARE ? logical / total : (int)blockIdx.z;
    const int in_split = SPLIT_AWARE ? logical - t.z * total : logical;
    t.tn = in_split % gn; t.tm = in_split / gn;
    return t;
}

__device__ __forceinline__ void bg_epilogue(const SgemmArgs& a, const f32x4 (&acc)[4][4], float* __restrict__ partial, float* __restrict__ stage,
                                            int m0, int n0, int tid, int zsplit) {
    const int lane = tid & 63, wave = tid >> 6, r16 = lane & 15, g = lane >> 4;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const bool direct = gridDim.z == 1;
    float* __restrict__ out = direct ? a.C : partial + (size_t)zsplit * a.M * a.N;
    const long ldo = direct ? a.ldc : a.N;
    const float* __restrict__ Rb = direct ? a.R : nullptr;
    const bool acc_c = direct && a.accumulate;
    const float alpha = direct ? a.alpha : 1.f;
    bool vec = n0 + MG_BN <= a.N && ldo % 4 == 0 && ep_al16(out);
    if (direct)
        vec = vec && ep_al16(a.gelu_pre16) && ep_al16(a.bias) && ep_al16(a.R) && a.ldr % 4 == 0 && ep_al16(a.gelu_pre) && ep_al16(a.gelu_out) && ep_al16(a.c16) && ep_al16(a.gelu_out16);
    if (vec) {
        const int c4 = tid & 31, gn = n0 + 4 * c4;
        f32x4 b4 = f32x4{0.f, 0.f, 0.f, 0.f};
        if (direct && a.bias) b4 = *reinterpret_cast<const f32x4*>(a.bias + gn);
        const float* __restrict__ pre = direct ? a.gelu_pre : nullptr;
        const bf16_t* __restrict__ pre16 = direct ? a.gelu_pre16 : nullptr;
        const bool store32 = out != nullptr;
        float* __restrict__ gout = direct ? a.gelu_out : nullptr;
        bf16_t* __restrict__ c16 = direct ? a.c16 : nullptr;
        bf16_t* __restrict__ g16 = direct ? a.gelu_out16 : nullptr;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if ((wave >> 1) == h) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
#pragma unroll
                        for (int j = 0; j < 4; ++j) stage[(16 * i + 4 * g + r) * EP_LD + wn + 16 * j + r16] = acc[i][j][r];
            }
            __syncthreads();
#pragma unroll
            for (int qq = 0; qq < 4; ++qq) {
                // two row pieces per thread and round (four would spill at three waves per SIMD): everything they read is requested
                // before the first of them is stored
                constexpr int NQ = 2;
                f32x4 v[NQ], rv[NQ], cv[NQ], pv[NQ];
                bool ok[NQ];
                size_t at[NQ];
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    const int row = (tid >> 5) + 8 * (NQ * qq + q), gm_ = m0 + 64 * h + row;
                    ok[q] = gm_ < a.M;
                    at[q] = (size_t)gm_ * ldo + gn;
                    v[q] = *reinterpret_cast<const f32x4*>(stage + row * EP_LD + 4 * c4);
                    rv[q] = cv[q] = pv[q] = f32x4{0.f, 0.f, 0.f, 0.f};
                    if (Rb && ok[q]) rv[q] = *reinterpret_cast<const f32x4*>(Rb + (size_t)(gm_ < a.rper ? gm_ : gm_ % a.rper) * a.ldr + gn);
                    if (acc_c && ok[q]) cv[q] = *reinterpret_cast<const f32x4*>(out + at[q]);
                    if (pre && ok[q]) pv[q] = *reinterpret_cast<const f32x4*>(pre + at[q]);
                    if (pre16 && ok[q]) {
                        const u32x2 w = *reinterpret_cast<const u32x2*>(pre16 + at[q]);
                        pv[q] = f32x4{bf16_lo(w.x), bf16_hi(w.x), bf16_lo(w.y), bf16_hi(w.y)};
                    }
                }
#pragma unroll
                for (int q = 0; q < NQ; ++q) {
                    if (!ok[q]) continue;
                    f32x4 add = b4;
                    if (Rb) add += rv[q];
                    if (acc_c) add += cv[q];
                    f32x4 o;
#pragma unroll
                    for (int e = 0; e < 4; ++e) o[e] = fmaf(alpha, v[q][e], add[e]);      // spelled out: both forms and every instantiation round alike
                    if (pre || pre16) {
#pragma unroll
                        for (int e = 0; e < 4; ++e) o[e] *= gelu_grad(pv[q][e]);
                    }
                    if (store32) *reinterpret_cast<f32x4*>(out + at[q]) = o;
                    if (c16) {
                        union { u32x2 u; bf16_t e[4]; } hh;
#pragma unroll
                        for (int e = 0; e < 4; ++e) hh.e[e] = static_cast<bf16_t>(o[e]);
                        *reinterpret_cast<u32x2*>(c16 + at[q]) = hh.u;
                    }
                    if (gout || g16) {
                        f32x4 ge;
#pragma unroll
                        for (int e = 0; e < 4; ++e) ge[e] = gelu_erf(o[e]);
                        if (gout) *reinterpret_cast<f32x4*>(gout + at[q]) = ge;
                        if (g16) {
                            union { u32x2 u; bf16_t e[4]; } hh;
#pragma unroll
                            for (int e = 0; e < 4; ++e) hh.e[e] = static_cast<bf16_t>(ge[e]);
                            *reinterpret_cast<u32x2*>(g16 + at[q]) = hh.u;
                        }
                    }
                }
            }
            __syncthreads();
        }
        return;
    }
    const int gn0 = n0 + wn + r16;
    bool cok[4];
    float bj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        cok[j] = gn0 + 16 * j < a.N;
        bj[j] = (direct && a.bias && cok[j]) ? a.bias[gn0 + 16 * j] : 0.f;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int gm_ = m0 + wm + 16 * i + 4 * g + r;
            if (gm_ >= a.M) continue;
            float* __restrict__ crow = out + (size_t)gm_ * ldo + gn0;
            float add[4] = {bj[0], bj[1], bj[2], bj[3]};
            if (Rb) {
                const float* __restrict__ rrow = Rb + (size_t)(gm_ < a.rper ? gm_ : gm_ % a.rper) * a.ldr + gn0;
                float rv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) rv[j] = cok[j] ? rrow[16 * j] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) add[j] += rv[j];
            }
            if (acc_c) {
                float cv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) cv[j] = cok[j] ? crow[16 * j] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) add[j] += cv[j];
            }
            float mul[4] = {1.f, 1.f, 1.f, 1.f};
            if (direct && a.gelu_pre16) {
                const bf16_t* __restrict__ prow = a.gelu_pre16 + (size_t)gm_ * a.ldc + gn0;
#pragma unroll
                for (int j = 0; j < 4; ++j) mul[j] = gelu_grad(cok[j] ? static_cast<float>(prow[16 * j]) : 0.f);
            }
            if (direct && a.gelu_pre) {
                const float* __restrict__ prow = a.gelu_pre + (size_t)gm_ * a.ldc + gn0;
                float pv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) pv[j] = cok[j] ? prow[16 * j] : 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) mul[j] = gelu_grad(pv[j]);
            }
            float* __restrict__ grow = (direct && a.gelu_out) ? a.gelu_out + (size_t)gm_ * a.ldc + gn0 : nullptr;
            bf16_t* __restrict__ c16row = (direct && a.c16) ? a.c16 + (size_t)gm_ * a.ldc + gn0 : nullptr;
            bf16_t* __restrict__ g16row = (direct && a.gelu_out16) ? a.gelu_out16 + (size_t)gm_ * a.ldc + gn0 : nullptr;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (cok[j]) {
                    const float v = fmaf(alpha, acc[i][j][r], add[j]) * mul[j];
                    if (out) crow[16 * j] = v;
                    if (c16row) c16row[16 * j] = static_cast<bf16_t>(v);
                    if (grow) grow[16 * j] = gelu_erf(v);
                    if (g16row) g16row[16 * j] = static_cast<bf16_t>(gelu_erf(v));
                }
        }
}

// grid: (tiles_n * tiles_m, 1, splits) workgroups; gn, gm = the tile counts.  B16: the B operand is a bf16 shadow (a.b16).
// A16: so is the A operand (a.a16; outer-contiguous only: the dW products' dY^T, whose row sums — the bias gradient — are then the sums
// of the bf16 values)
template <bool AKF, bool BKF, bool B16 = false, bool A16 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(3, 3)))
void mfma_bgemm_kernel(const SgemmArgs a, int k_chunk, float* __restrict__ partial, int gn, int gm) {
    static_assert(!(A16 && AKF), "a k-contiguous bf16 A goes to mfma_bgemm16_kernel");
    using TB = std::conditional_t<B16, bf16_t, float>;
    using OpB = BgOperand<BKF, TB>;
    using TA = std::conditional_t<A16, bf16_t, float>;
    using OpA = BgOperand<AKF, TA>;
    // one LDS block: the two operands' two stages, then (all of it) the epilogue's staging tile
    constexpr int TILE_BYTES = 2 * MG_BM * BG_LD * 2;
    static_assert(2 * TILE_BYTES >= EP_STAGE_BYTES && 2 * TILE_BYTES >= 8 * 128 * 4, "LDS block too small for the epilogue");
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TILE_BYTES];
    bf16_t (*As)[MG_BM][BG_LD] = reinterpret_cast<bf16_t (*)[MG_BM][BG_LD]>(smem);
    bf16_t (*Bs)[MG_BN][BG_LD] = reinterpret_cast<bf16_t (*)[MG_BN][BG_LD]>(smem + TILE_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    // XCD-aware tile order (see above); the tail that does not fill a whole group of eight keeps its id
    const BgTile bt = bg_tile<true>(gn, gm);
    const int tn_ = bt.tn, tm_ = bt.tm, zsplit = bt.z;
    const int m0 = tm_ * MG_BM, n0 = tn_ * MG_BN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kbeg = zsplit * k_chunk, kend = min(a.K, kbeg + k_chunk);
    OpA oa; OpB ob;
    oa.init(reinterpret_cast<const TA*>(a.A), a.sam, a.sak, m0, a.M, kbeg, tid);
    ob.init(reinterpret_cast<const TB*>(a.B), a.sbn, a.sbk, n0, a.N, kbeg, tid);
    typename OpA::V ra[OpA::NL];
    typename OpB::V rb[OpB::NL];
    // row sums of A over this workgroup's k range (a.asum; only the first N-tile of a row panel adds them up): rs[i] belongs to outer
    // index 4 (tid & 31) + i (outer-contiguous A) or to row (tid >> 3) + 32 i (k-contiguous A: eight lanes per row)
    const bool do_sum = a.asum != nullptr && tn_ == 0;
    float rs[4] = {0.f, 0.f, 0.f, 0.f};
    auto add_rows = [&]() {
        if constexpr (A16) {
#pragma unroll
            for (int it = 0; it < 4; ++it) { rs[0] += bf16_lo(ra[it].x); rs[1] += bf16_hi(ra[it].x); rs[2] += bf16_lo(ra[it].y); rs[3] += bf16_hi(ra[it].y); }
        } else if constexpr (AKF) {
#pragma unroll
            for (int it = 0; it < 4; ++it) rs[it] += (ra[it].x + ra[it].y) + (ra[it].z + ra[it].w);
        } else {
#pragma unroll
            for (int it = 0; it < 4; ++it) { rs[0] += ra[it].x; rs[1] += ra[it].y; rs[2] += ra[it].z; rs[3] += ra[it].w; }
        }
    };
    if (kbeg < kend) {
        oa.fetch(ra); ob.fetch(rb);
        if (do_sum) add_rows();
        OpA::park(As[0], ra, tid);
        OpB::park(Bs[0], rb, tid);
    }
    __syncthreads();
    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += BG_BK) {
        const bool more = k0 + BG_BK < kend;
        if (more) { oa.fetch(ra); ob.fetch(rb); }       // in flight under this stage's MFMAs; first touched by park() below
        bf16x8 av[4], bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            av[i] = *reinterpret_cast<const bf16x8*>(&As[cur][wm + 16 * i + r16][8 * g]);
            bv[i] = *reinterpret_cast<const bf16x8*>(&Bs[cur][wn + 16 * i + r16][8 * g]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);              // nothing of park() (its waits for the loads) moves above the MFMAs
        if (more) {
            if (do_sum) add_rows();
            OpA::park(As[cur ^ 1], ra, tid);
            OpB::park(Bs[cur ^ 1], rb, tid);
        }
        __syncthreads();
        cur ^= 1;
    }
    if (do_sum) {
        // fold the threads' partial row sums in a fixed order through LDS (the operand tiles are dead) and add them to a.asum
        // (split-K: to this split's slot behind the product's partials; splitk_reduce_kernel adds the slots up)
        float* red = reinterpret_cast<float*>(smem);                   // [8][128]
        if constexpr (AKF) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                float v = rs[it];
                v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
                if ((tid & 7) == 0) red[(tid >> 3) + 32 * it] = v;
            }
        } else {
#pragma unroll
            for (int i = 0; i < 4; ++i) red[(tid >> 5) * 128 + 4 * (tid & 31) + i] = rs[i];
        }
        __syncthreads();
        if (tid < 128 && m0 + tid < a.M) {
            float v;
            if constexpr (AKF) v = red[tid];
            else v = ((red[tid] + red[128 + tid]) + (red[256 + tid] + red[384 + tid])) + ((red[512 + tid] + red[640 + tid]) + (red[768 + tid] + red[896 + tid]));
            if (gridDim.z == 1) a.asum[m0 + tid] += v;
            else partial[(size_t)gridDim.z * a.M * a.N + (size_t)zsplit * a.M + m0 + tid] = v;
        }
        __syncthreads();
    }
    bg_epilogue(a, acc, partial, reinterpret_cast<float*>(smem), m0, n0, tid, zsplit);
}

// The same contraction with SPLIT-bf16 operands (the training step's "bf16x3" mode; gemm.h SPLIT is the inference form): every fp32
// element v of A and B goes into LDS as a PAIR of bf16, hi = bf16(v) and lo = bf16(v - hi) (the subtraction is exact in fp32), and every
// product is evaluated as lo*hi + hi*lo + hi*hi on v_mfma_f32_16x16x32_bf16 — three MFMAs per fragment pair into the same accumulator,
// small terms first.  The three bf16 products are exact in fp32; what is dropped is lo*lo and the second rounding of lo, under
// 3 * 2^-16 relative to sum |a||b|.  Geometry, tile order, split-K, row sums (of the unsplit fp32 values) and epilogue are
// mfma_bgemm_kernel's; each operand parks two planes per stage, so the LDS block is 80 KiB and two workgroups share a CU.
//
// x3_split keeps the residual a scalar-f32 subtraction pinned to its own register (the empty asm): see the note above ln_apply4 in
// gemm.h — packed-f32 arithmetic next to this convert / subtract / convert sequence once produced wrong values in lanes 48-63.
__device__ __forceinline__ void x3_split(float v, bf16_t& hi, bf16_t& lo) {
    hi = static_cast<bf16_t>(v);                     // round to nearest even
    float d = v - static_cast<float>(hi);            // exact
    asm volatile("" : "+v"(d));
    lo = static_cast<bf16_t>(d);
}
// BgOperand<KFAST, float>::park with the split: the same threads, rows and 8-byte stores, once into each plane
template <bool KFAST>
__device__ __forceinline__ void x3_park(bf16_t (*hi)[BG_LD], bf16_t (*lo)[BG_LD], const float4 (&r)[4], int tid) {
    if constexpr (KFAST) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it, o = idx >> 3, k4 = idx & 7;
            union { uint2 u; bf16_t e[4]; } h, l;
            x3_split(r[it].x, h.e[0], l.e[0]); x3_split(r[it].y, h.e[1], l.e[1]); x3_split(r[it].z, h.e[2], l.e[2]); x3_split(r[it].w, h.e[3], l.e[3]);
            *reinterpret_cast<uint2*>(&hi[o][4 * k4]) = h.u;
            *reinterpret_cast<uint2*>(&lo[o][4 * k4]) = l.u;
        }
    } else {
        const int kq = tid >> 5, o4 = tid & 31;
        const float v[4][4] = {{r[0].x, r[0].y, r[0].z, r[0].w}, {r[1].x, r[1].y, r[1].z, r[1].w}, {r[2].x, r[2].y, r[2].z, r[2].w}, {r[3].x, r[3].y, r[3].z, r[3].w}};
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            union { uint2 u; bf16_t e[4]; } h, l;
#pragma unroll
            for (int it = 0; it < 4; ++it) x3_split(v[it][i], h.e[it], l.e[it]);
            *reinterpret_cast<uint2*>(&hi[4 * o4 + i][4 * kq]) = h.u;
            *reinterpret_cast<uint2*>(&lo[4 * o4 + i][4 * kq]) = l.u;
        }
    }
}

// The row-sum rider's tail as in mfma_bgemm_kernel (which keeps its own inline copy: calling this helper there changes the register
// allocation of those tuned kernels, 150 -> 166 VGPRs in the k-contiguous forms): the threads' partial row sums of A over
// this workgroup's k range — rs[i] belongs to outer index 4 (tid & 31) + i (outer-contiguous A) or to row (tid >> 3) + 32 i (k-contiguous A:
// eight lanes per row) — folded in a fixed order through LDS (`red`, [8][128] floats: the operand tiles are dead) and added to a.asum
// (split-K: to this split's slot behind the product's partials; splitk_reduce_kernel adds the slots up)
template <bool AKF>
__device__ __forceinline__ void bg_fold_row_sums(const SgemmArgs& a, const float (&rs)[4], float* red, float* partial,
                                                 int m0, int zsplit, int tid) {
    if constexpr (AKF) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            float v = rs[it];
            v += __shfl_xor(v, 1, 64); v += __shfl_xor(v, 2, 64); v += __shfl_xor(v, 4, 64);
            if ((tid & 7) == 0) red[(tid >> 3) + 32 * it] = v;
        }
    } else {
#pragma unroll
        for (int i = 0; i < 4; ++i) red[(tid >> 5) * 128 + 4 * (tid & 31) + i] = rs[i];
    }
    __syncthreads();
    if (tid < 128 && m0 + tid < a.M) {
        float v;
        if constexpr (AKF) v = red[tid];
        else v = ((red[tid] + red[128 + tid]) + (red[256 + tid] + red[384 + tid])) + ((red[512 + tid] + red[640 + tid]) + (red[768 + tid] + red[896 + tid]));
        if (gridDim.z == 1) a.asum[m0 + tid] += v;
        else partial[(size_t)gridDim.z * a.M * a.N + (size_t)zsplit * a.M + m0 + tid] = v;
    }
    __syncthreads();
}

template <bool AKF, bool BKF>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(2, 2)))
void mfma_x3gemm_kernel(const SgemmArgs a, int k_chunk, float* __restrict__ partial, int gn, int gm) {
    using OpA = BgOperand<AKF, float>;
    using OpB = BgOperand<BKF, float>;
    // one LDS block: per stage the hi and lo planes of A, then of B; two stages; then (all of it) the epilogue's staging tile
    constexpr int PLANE_BYTES = MG_BM * BG_LD * 2, STAGE_BYTES = 4 * PLANE_BYTES;
    static_assert(MG_BM == MG_BN, "one plane size for both operands");
    static_assert(2 * STAGE_BYTES >= EP_STAGE_BYTES && 2 * STAGE_BYTES >= 8 * 128 * 4, "LDS block too small for the epilogue");
    static_assert(2 * (2 * STAGE_BYTES) <= 160 * 1024, "two workgroups per CU");
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * STAGE_BYTES];
    using Plane = bf16_t (*)[BG_LD];
    auto plane = [&](int stage, int which) { return reinterpret_cast<Plane>(smem + stage * STAGE_BYTES + which * PLANE_BYTES); };      // which: A hi, A lo, B hi, B lo
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BgTile bt = bg_tile<true>(gn, gm);
    const int tn_ = bt.tn, tm_ = bt.tm, zsplit = bt.z;
    const int m0 = tm_ * MG_BM, n0 = tn_ * MG_BN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kbeg = zsplit * k_chunk, kend = min(a.K, kbeg + k_chunk);
    OpA oa; OpB ob;
    oa.init(a.A, a.sam, a.sak, m0, a.M, kbeg, tid);
    ob.init(a.B, a.sbn, a.sbk, n0, a.N, kbeg, tid);
    float4 ra[4], rb[4];
    // row sums of A over this workgroup's k range, of the fp32 values before the split, in mfma_bgemm_kernel's order.  They read the
    // registers x3_park splits next, so every addition is a scalar-f32 one pinned to its register like x3_split's residual (unpinned,
    // the compiler packs them into v_pk_add_f32 right in front of the convert / subtract / convert sequence)
    const bool do_sum = a.asum != nullptr && tn_ == 0;
    float rs[4] = {0.f, 0.f, 0.f, 0.f};
    auto add_rows = [&]() {
        if constexpr (AKF) {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                float s0 = ra[it].x + ra[it].y, s1 = ra[it].z + ra[it].w;
                asm volatile("" : "+v"(s0)); asm volatile("" : "+v"(s1));
                s0 += s1; asm volatile("" : "+v"(s0));
                rs[it] += s0; asm volatile("" : "+v"(rs[it]));
            }
        } else {
#pragma unroll
            for (int it = 0; it < 4; ++it) {
                // (a pin behind each sum alone left the first two additions of a call packed: the addends are pinned as well)
                float x = ra[it].x, y = ra[it].y, z = ra[it].z, w = ra[it].w;
                asm volatile("" : "+v"(x)); rs[0] += x; asm volatile("" : "+v"(rs[0]));
                asm volatile("" : "+v"(y)); rs[1] += y; asm volatile("" : "+v"(rs[1]));
                asm volatile("" : "+v"(z)); rs[2] += z; asm volatile("" : "+v"(rs[2]));
                asm volatile("" : "+v"(w)); rs[3] += w; asm volatile("" : "+v"(rs[3]));
            }
        }
    };
    if (kbeg < kend) {
        oa.fetch(ra); ob.fetch(rb);
        if (do_sum) add_rows();
        x3_park<AKF>(plane(0, 0), plane(0, 1), ra, tid);
        x3_park<BKF>(plane(0, 2), plane(0, 3), rb, tid);
    }
    __syncthreads();
    int cur = 0;
    for (int k0 = kbeg; k0 < kend; k0 += BG_BK) {
        const bool more = k0 + BG_BK < kend;
        if (more) { oa.fetch(ra); ob.fetch(rb); }       // in flight under this stage's MFMAs; first touched by x3_park() below
        const Plane Ah = plane(cur, 0), Al = plane(cur, 1), Bh = plane(cur, 2), Bl = plane(cur, 3);
        bf16x8 ah[4], al[4], bh[4], bl[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            ah[i] = *reinterpret_cast<const bf16x8*>(&Ah[wm + 16 * i + r16][8 * g]);
            al[i] = *reinterpret_cast<const bf16x8*>(&Al[wm + 16 * i + r16][8 * g]);
            bh[i] = *reinterpret_cast<const bf16x8*>(&Bh[wn + 16 * i + r16][8 * g]);
            bl[i] = *reinterpret_cast<const bf16x8*>(&Bl[wn + 16 * i + r16][8 * g]);
        }
        // per accumulator lo*hi, then hi*lo, then hi*hi; the sixteen accumulators of one term are independent
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(al[i], bh[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bl[j], acc[i][j], 0, 0, 0);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(ah[i], bh[j], acc[i][j], 0, 0, 0);
        __builtin_amdgcn_sched_barrier(0);              // nothing of x3_park() (its waits for the loads) moves above the MFMAs
        if (more) {
            if (do_sum) add_rows();
            x3_park<AKF>(plane(cur ^ 1, 0), plane(cur ^ 1, 1), ra, tid);
            x3_park<BKF>(plane(cur ^ 1, 2), plane(cur ^ 1, 3), rb, tid);
        }
        __syncthreads();
        cur ^= 1;
    }
    if (do_sum) bg_fold_row_sums<AKF>(a, rs, reinterpret_cast<float*>(smem), partial, m0, zsplit, tid);
    bg_epilogue(a, acc, partial, reinterpret_cast<float*>(smem), m0, n0, tid, zsplit);
}

// Both operands bf16 shadows with k contiguous (the forward products x W^T of the encoder, and dX = dY W through the transposed
// weight shadow): 64 of K per stage — a row of a stage is 128 bytes, one whole cache line per row and request, where a 32-deep stage of
// bf16 would use half of every line it pulls into the CU's L1 — loaded as 16-byte pieces and parked in LDS as they are (no conversion,
// no VALU work between the load and the ds_write_b128).  One LDS buffer of 128 x (64 + 8) per operand (36 KiB: three workgroups per CU
// as before), the next stage waits in registers under the current stage's 32 MFMAs per wave.  Same tile order, accumulation order
// (ascending k in steps of 32), split-K and epilogue as mfma_bgemm_kernel: bit-identical results.  K % 64 == 0.
constexpr int BH_BK = 64, BH_LD = 72;
// one 32-deep half of a 64-deep stage: 16 MFMAs of a wave's 64 x 64 tile.  ONE_B: the B fragments one at a time (the four-workgroup forms)
template <bool ONE_B>
__device__ __forceinline__ void bg16_stage_mfma(const bf16_t (*As)[72], const bf16_t (*Bs)[72], f32x4 (&acc)[4][4], int wm, int wn, int r16, int g, int kk) {
    bf16x8 av[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) av[i] = *reinterpret_cast<const bf16x8*>(&As[wm + 16 * i + r16][32 * kk + 8 * g]);
    if constexpr (ONE_B) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const bf16x8 bj = *reinterpret_cast<const bf16x8*>(&Bs[wn + 16 * j + r16][32 * kk + 8 * g]);
#pragma unroll
            for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bj, acc[i][j], 0, 0, 0);
        }
    } else {
        bf16x8 bv[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) bv[i] = *reinterpret_cast<const bf16x8*>(&Bs[wn + 16 * i + r16][32 * kk + 8 * g]);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(av[i], bv[j], acc[i][j], 0, 0, 0);
    }
}
// WHOLE (M and N multiples of 128 — every product of the PARSeq-S / ViTSTR encoders): FOUR workgroups per CU.  The kernel waits on memory, not on
// the matrix pipe (six 64-deep stages per tile at K = 384, one stage of register prefetch), so what it needs is more waves to switch to; at 140
// registers it sat at three.  The loads become buffer loads — one resource per operand in SGPRs, ONE constant byte offset per thread and
// operand in a VGPR, the piece's 32-row distance and the k position in the scalar offset: no 64-bit pointers, no per-piece offsets — and the
// B fragments are read one at a time (16 instead of 32 fragment registers): 126 VGPRs, no scratch.
template <bool WHOLE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WHOLE ? 4 : 3, WHOLE ? 4 : 3)))
void mfma_bgemm16_kernel(const SgemmArgs a, int k_chunk, float* __restrict__ partial, int gn, int gm) {
    constexpr int TILE_BYTES = MG_BM * BH_LD * 2;
    static_assert(2 * TILE_BYTES >= EP_STAGE_BYTES, "LDS block too small for the epilogue");
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TILE_BYTES];
    bf16_t (*As)[BH_LD] = reinterpret_cast<bf16_t (*)[BH_LD]>(smem);
    bf16_t (*Bs)[BH_LD] = reinterpret_cast<bf16_t (*)[BH_LD]>(smem + TILE_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BgTile bt = bg_tile<false>(gn, gm);
    const int tn_ = bt.tn, tm_ = bt.tm, zsplit = bt.z;
    const int m0 = tm_ * MG_BM, n0 = tn_ * MG_BN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kbeg = zsplit * k_chunk, kend = min(a.K, kbeg + k_chunk);
    // thread = (row idx >> 3, 8 consecutive k at 8 (idx & 7)), idx = tid + 256 it; rows past the edge re-read the last valid row
    const bf16_t* pa[WHOLE ? 1 : 4];
    const bf16_t* pb[WHOLE ? 1 : 4];
    __amdgpu_buffer_rsrc_t ares, bres;
    unsigned oa = 0, ob = 0, pa_step = 0, pb_step = 0, kbyte = 0;
    if constexpr (WHOLE) {
        ares = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.A), 0, 0x7FFFF000, 0x00020000);
        bres = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.B), 0, 0x7FFFF000, 0x00020000);
        oa = 2u * ((unsigned)(m0 + (tid >> 3)) * (unsigned)a.sam + 8u * (tid & 7));
        ob = 2u * ((unsigned)(n0 + (tid >> 3)) * (unsigned)a.sbn + 8u * (tid & 7));
        pa_step = 64u * (unsigned)a.sam; pb_step = 64u * (unsigned)a.sbn;      // 32 rows, in bytes
        kbyte = 2u * (unsigned)kbeg;
    } else {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it;
            pa[it] = reinterpret_cast<const bf16_t*>(a.A) + (size_t)min(m0 + (idx >> 3), a.M - 1) * a.sam + kbeg + 8 * (idx & 7);
            pb[it] = reinterpret_cast<const bf16_t*>(a.B) + (size_t)min(n0 + (idx >> 3), a.N - 1) * a.sbn + kbeg + 8 * (idx & 7);
        }
    }
    u32x4 ra[4], rb[4];
    auto fetch = [&]() {
        if constexpr (WHOLE) {
#pragma unroll
            for (int it = 0; it < 4; ++it) ra[it] = __builtin_amdgcn_raw_buffer_load_b128(ares, oa, kbyte + it * pa_step, 0);
#pragma unroll
            for (int it = 0; it < 4; ++it) rb[it] = __builtin_amdgcn_raw_buffer_load_b128(bres, ob, kbyte + it * pb_step, 0);
            kbyte += 2u * BH_BK;
        } else {
#pragma unroll
            for (int it = 0; it < 4; ++it) { ra[it] = *reinterpret_cast<const u32x4*>(pa[it]); pa[it] += BH_BK; }
#pragma unroll
            for (int it = 0; it < 4; ++it) { rb[it] = *reinterpret_cast<const u32x4*>(pb[it]); pb[it] += BH_BK; }
        }
    };
    if (kbeg < kend) fetch();
    for (int k0 = kbeg; k0 < kend; k0 += BH_BK) {
#pragma unroll
        for (int it = 0; it < 4; ++it) {
            const int idx = tid + 256 * it;
            *reinterpret_cast<u32x4*>(&As[idx >> 3][8 * (idx & 7)]) = ra[it];
            *reinterpret_cast<u32x4*>(&Bs[idx >> 3][8 * (idx & 7)]) = rb[it];
        }
        __syncthreads();
        if (k0 + BH_BK < kend) fetch();                 // in flight under this stage's MFMAs; first touched by the stores above, next round
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bg16_stage_mfma<WHOLE>(As, Bs, acc, wm, wn, r16, g, kk);
        }
        __builtin_amdgcn_sched_barrier(0);              // the waits for the loads stay below the MFMAs
        __syncthreads();
    }
    bg_epilogue(a, acc, partial, reinterpret_cast<float*>(smem), m0, n0, tid, zsplit);
}

// The dW products dY^T X with BOTH operands bf16 in memory and outer-contiguous (the contraction index m is the row index of dY [m, n]
// and of X [m, k']): 64 rows of m per stage.  A thread loads 8-byte pieces (four outer indices at one m), eight of them per operand
// and stage, and parks them transposed: for each of its four outer indices the eight m values as ONE 16-byte LDS store.  One LDS buffer
// + the next stage in registers, as mfma_bgemm16_kernel; with 32-deep stages the kernel paid one exposed memory round trip per 16
// MFMAs per wave (49 152-deep contractions in 15 splits: 102 stages of 1.9 us) — at 64 deep it pays one per 32.  Row sums of A (the bias
// gradient, a.asum) are sums of the bf16 values.  K % 64 == 0, M % 4 == 0, N % 4 == 0.
// WHOLE: as mfma_bgemm16_kernel<true> — four workgroups per CU, buffer loads with the k position of a piece in the scalar offset (128 VGPRs, no scratch)
template <bool WHOLE>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(WHOLE ? 4 : 3, WHOLE ? 4 : 3)))
void mfma_bgemm16t_kernel(const SgemmArgs a, int k_chunk, float* __restrict__ partial, int gn, int gm) {
    constexpr int TILE_BYTES = MG_BM * BH_LD * 2;
    static_assert(2 * TILE_BYTES >= EP_STAGE_BYTES && 2 * TILE_BYTES >= 8 * 128 * 4, "LDS block too small for the epilogue");
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * TILE_BYTES];
    bf16_t (*As)[BH_LD] = reinterpret_cast<bf16_t (*)[BH_LD]>(smem);
    bf16_t (*Bs)[BH_LD] = reinterpret_cast<bf16_t (*)[BH_LD]>(smem + TILE_BYTES);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const BgTile bt = bg_tile<false>(gn, gm);
    const int tn_ = bt.tn, tm_ = bt.tm, zsplit = bt.z;
    const int m0 = tm_ * MG_BM, n0 = tn_ * MG_BN;
    const int wm = (wave >> 1) * 64, wn = (wave & 1) * 64;
    const int r16 = lane & 15, g = lane >> 4;
    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    const int kbeg = zsplit * k_chunk, kend = min(a.K, kbeg + k_chunk);
    // thread = (outer group o4 = tid & 31: outer indices 4 o4 .. 4 o4 + 3, k octet kq = tid >> 5: k = 8 kq + it); groups past the edge
    // re-read the last valid group of four
    const int o4 = tid & 31, kq = tid >> 5;
    const bf16_t* pa = nullptr; const bf16_t* pb = nullptr;
    const long sa = a.sak, sb = a.sbk;
    __amdgpu_buffer_rsrc_t ares, bres;
    unsigned sa2 = 0, sb2 = 0, oa = 0, ob = 0, ka = 0, kb = 0;
    if constexpr (WHOLE) {
        ares = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.A), 0, 0x7FFFF000, 0x00020000);
        bres = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.B), 0, 0x7FFFF000, 0x00020000);
        sa2 = 2u * (unsigned)a.sak; sb2 = 2u * (unsigned)a.sbk;      // bytes per k
        oa = 8u * (unsigned)kq * sa2 + 2u * (unsigned)(m0 + 4 * o4);
        ob = 8u * (unsigned)kq * sb2 + 2u * (unsigned)(n0 + 4 * o4);
        ka = (unsigned)kbeg * sa2; kb = (unsigned)kbeg * sb2;
    } else {
        pa = reinterpret_cast<const bf16_t*>(a.A) + (size_t)(kbeg + 8 * kq) * a.sak + min(m0 + 4 * o4, a.M - 4);
        pb = reinterpret_cast<const bf16_t*>(a.B) + (size_t)(kbeg + 8 * kq) * a.sbk + min(n0 + 4 * o4, a.N - 4);
    }
    u32x2 ra[8], rb[8];
    auto fetch = [&]() {
        if constexpr (WHOLE) {
#pragma unroll
            for (int it = 0; it < 8; ++it) ra[it] = __builtin_amdgcn_raw_buffer_load_b64(ares, oa, ka + it * sa2, 0);
#pragma unroll
            for (int it = 0; it < 8; ++it) rb[it] = __builtin_amdgcn_raw_buffer_load_b64(bres, ob, kb + it * sb2, 0);
            ka += BH_BK * sa2; kb += BH_BK * sb2;
        } else {
#pragma unroll
            for (int it = 0; it < 8; ++it) ra[it] = *reinterpret_cast<const u32x2*>(pa + it * sa);
#pragma unroll
            for (int it = 0; it < 8; ++it) rb[it] = *reinterpret_cast<const u32x2*>(pb + it * sb);
            pa += BH_BK * sa; pb += BH_BK * sb;
        }
    };
    // r[it] = {outer 0 | outer 1 << 16, outer 2 | outer 3 << 16} at k = 8 kq + it  ->  row (4 o4 + i): k = 8 kq .. 8 kq + 7 as four dwords
    auto park = [&](bf16_t (*tile)[BH_LD], const u32x2 (&r)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            u32x4 o;
#pragma unroll
            for (int d = 0; d < 4; ++d) {
                const unsigned w0 = (i & 2) ? r[2 * d].y : r[2 * d].x, w1 = (i & 2) ? r[2 * d + 1].y : r[2 * d + 1].x;
                o[d] = (i & 1) ? ((w0 >> 16) | (w1 & 0xffff0000u)) : ((w0 & 0xffffu) | (w1 << 16));
            }
            *reinterpret_cast<u32x4*>(&tile[4 * o4 + i][8 * kq]) = o;
        }
    };
    const bool do_sum = a.asum != nullptr && tn_ == 0;
    float rs[4] = {0.f, 0.f, 0.f, 0.f};
    if (kbeg < kend) fetch();
    for (int k0 = kbeg; k0 < kend; k0 += BH_BK) {
        if (do_sum) {
#pragma unroll
            for (int it = 0; it < 8; ++it) { rs[0] += bf16_lo(ra[it].x); rs[1] += bf16_hi(ra[it].x); rs[2] += bf16_lo(ra[it].y); rs[3] += bf16_hi(ra[it].y); }
        }
        park(As, ra);
        park(Bs, rb);
        __syncthreads();
        if (k0 + BH_BK < kend) fetch();                 // in flight under this stage's MFMAs
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            bg16_stage_mfma<WHOLE>(As, Bs, acc, wm, wn, r16, g, kk);
        }
        __builtin_amdgcn_sched_barrier(0);
        __syncthreads();
    }
    if (do_sum) {
        // as mfma_bgemm_kernel: the eight k octets' partial sums of every row through LDS in a fixed order
        float* red = reinterpret_cast<float*>(smem);                   // [8][128]
#pragma unroll
        for (int i = 0; i < 4; ++i) red[kq * 128 + 4 * o4 + i] = rs[i];
        __syncthreads();
        if (tid < 128 && m0 + tid < a.M) {
            const float v = ((red[tid] + red[128 + tid]) + (red[256 + tid] + red[384 + tid])) + ((red[512 + tid] + red[640 + tid]) + (red[768 + tid] + red[896 + tid]));
            if (gridDim.z == 1) a.asum[m0 + tid] += v;
            else partial[(size_t)gridDim.z * a.M * a.N + (size_t)zsplit * a.M + m0 + tid] = v;
        }
        __syncthreads();
    }
    bg_epilogue(a, acc, partial, reinterpret_cast<float*>(smem), m0, n0, tid, zsplit);
}

// bf16 shadows of a Linear weight W [N, K] (fp32 master): W16 [N, K] and its transpose Wt16 [K, N], once per step.  N, K multiples of 32.
// All of a step's weight shadows in ONE launch: the table lists the matrices (master offset, shape, first tile, destination relative to the
// shadows' base: W16 there, Wt16 right behind it); workgroup t converts tile t - tile0 of the matrix whose range holds t.
struct ShadowEntry { unsigned src, N, K, tile0; unsigned long long dst; };
static __global__ __launch_bounds__(256)
void weight_shadows_kernel(const float* __restrict__ master, const ShadowEntry* __restrict__ tab, int entries, bf16_t* __restrict__ base) {
    __shared__ float t[32][33];
    int e = 0;
    while (e + 1 < entries && tab[e + 1].tile0 <= blockIdx.x) ++e;
    const ShadowEntry se = tab[e];
    const int N = (int)se.N, K = (int)se.K, tile = (int)(blockIdx.x - se.tile0), kt = K / 32;
    const float* W = master + se.src;
    bf16_t* W16 = base + se.dst; bf16_t* Wt16 = W16 + (size_t)N * K;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const int n0 = (tile / kt) * 32, k0 = (tile % kt) * 32;
#pragma unroll
    for (int r = ty; r < 32; r += 8) {
        const float v = W[(size_t)(n0 + r) * K + k0 + tx];
        t[r][tx] = v;
        W16[(size_t)(n0 + r) * K + k0 + tx] = static_cast<bf16_t>(v);
    }
    __syncthreads();
#pragma unroll
    for (int r = ty; r < 32; r += 8) Wt16[(size_t)(k0 + r) * N + n0 + tx] = static_cast<bf16_t>(t[tx][r]);
}

// dst[Rd, Cd] = src[Rs, Cs] in its top-left corner, zeros elsewhere (Rd >= Rs, Cd >= Cs)
static __global__ __launch_bounds__(256)
void pad_copy_kernel(const float* __restrict__ src, int Rs, int Cs, float* __restrict__ dst, int Rd, int Cd) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)Rd * Cd) return;
    const int r = (int)(i / Cd), c = (int)(i % Cd);
    dst[i] = (r < Rs && c < Cs) ? src[(size_t)r * Cs + c] : 0.f;
}
static __global__ __launch_bounds__(256)
void add_into_kernel(const float* __restrict__ src, float* __restrict__ dst, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

static __global__ __launch_bounds__(256)
void splitk_reduce_kernel(const SgemmArgs a, const float* __restrict__ partial, int splits) {
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x, total = (size_t)a.M * a.N;
    if (idx >= total) {                       // the threads past the product fold the row sums of A (partials behind the product's, [splits][M])
        const size_t m = idx - total;
        if (a.asum && m < (size_t)a.M) {
            float t = 0.f;
            for (int z = 0; z < splits; ++z) t += partial[(size_t)splits * total + (size_t)z * a.M + m];
            a.asum[m] += t;
        }
        return;
    }
    const int gm = (int)(idx / a.N), gn = (int)(idx % a.N);
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += partial[(size_t)z * total + idx];
    v *= a.alpha;
    if (a.bias) v += a.bias[gn];
    if (a.R) v += a.R[(size_t)(gm % a.rper) * a.ldr + gn];
    float* c = a.C + (size_t)gm * a.ldc + gn;
    if (a.accumulate) v += *c;
    if (a.gelu_pre) v *= gelu_grad(a.gelu_pre[(size_t)gm * a.ldc + gn]);
    if (a.gelu_pre16) v *= gelu_grad(static_cast<float>(a.gelu_pre16[(size_t)gm * a.ldc + gn]));
    if (a.C) *c = v;
    if (a.c16) a.c16[(size_t)gm * a.ldc + gn] = static_cast<bf16_t>(v);
    if (a.gelu_out) a.gelu_out[(size_t)gm * a.ldc + gn] = gelu_erf(v);
    if (a.gelu_out16) a.gelu_out16[(size_t)gm * a.ldc + gn] = static_cast<bf16_t>(gelu_erf(v));
}

}  // namespace pq
