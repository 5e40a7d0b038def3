// The attention of the training step with a head's whole K / V resident in LDS: TrainAttnArgs, which
// every attention kernel of the step takes (those of train_attn_wide.h too), and four kernel families, forward and backward each:
//   train_attn_kernel<BACKWARD, HD>          fp32 on the VALU, head width 32 or 64, masks, dropout, several passes per launch
//   train_attn_mfma_kernel<BACKWARD>         fp32 on the matrix cores (exact 16x16x4 products): head width 64, <= 128 keys, no masks
//   train_attn_bf16_kernel<BACKWARD>         the bf16-operand mode's encoder shape: 128 tokens, head width 64, no masks, no dropout
//   train_attn_dec_bf16_kernel<BACKWARD, KT> the bf16-operand mode's decoder shapes: head width 32, <= 32 queries, <= 128 keys, masks,
//                                            dropout, the passes of a batch in one launch or in one workgroup (pass_loop)
// Beside each kernel stands the function that gives its dynamic LDS bytes (train_attn_lds_floats, train_attn_mfma_lds,
// train_attn_bf16_lds, train_attn_dec_lds); the two bf16 kernels build their pointers and those sizes from one map (AttnBf16Map).
// Which kernel a call takes, and what each accepts, is lib_train.hip's train_attn_plan().  One workgroup per (image, head); everything
// is deterministic (no atomics); dK / dV accumulate into their output only if kv_accumulate.
#pragma once
#include "common.h"
#include "train_rows.h"      // DropSpec / drop_factor: the dropout on the probabilities

namespace pq {

// -------------------------------------------------------------------------------------------------------------------
// Soft-max attention (decoder: head width 32, encoder: 64), one workgroup per (image b, head h), operands in LDS, the
// queries walked in blocks of 32 rows (the key / value gradients of a head stay in registers across the blocks).
//   q row (b, l): q + b * q_bstride + l * ldq + HD h        (q_bstride = 0: the queries are shared by the batch)
//   k / v row (b, j): k|v + (b * Lk + j) * ldkv + HD h
//   key j of query l is masked when qmask[l * Lk + j] or kmask[b * ldkm + j] (either pointer may be null)
// Every query must keep at least one key (true on this path: <bos> is never masked).  Lk * HD <= 8192.
// -------------------------------------------------------------------------------------------------------------------
struct TrainAttnArgs {
    const float* q; long q_bstride; int ldq;
    const float* k; const float* v; int ldkv;
    const unsigned char* qmask; const unsigned char* kmask; int ldkm;
    float* o; int ldo;                                           // forward output, row (b, l): o + (b * Lq + l) * ldo + HD h
    bf16_t* o16 = nullptr;                                       // train_attn_bf16_kernel forward: write o here as bf16 INSTEAD (same layout)
    bf16_t* dq16 = nullptr; bf16_t* dk16 = nullptr; bf16_t* dv16 = nullptr;      // train_attn_bf16_kernel backward: write dq / dk / dv here as bf16
                                                                 // INSTEAD (layouts of dq / dk / dv; no kv_accumulate)
    const float* d_o;                                            // backward: gradient of o (same layout as o)
    float* dq; int lddq;                                         // backward: stored, row (b, l) even when q is shared
    float* dk; float* dv; int lddkv;                             // backward: layout of k / v; accumulated into if kv_accumulate
    int kv_accumulate;
    int Lq, Lk, H;
    float scale;
    DropSpec drop; unsigned drop_site;                           // dropout on the probabilities, element ((b H + h) Lq + l) Lk + j
    // Several permutation passes in one launch (train_attn_kernel and train_attn_dec_bf16_kernel; 0 = off): the batch is [passes][pass_B]
    // images, image index b = p * pass_B + bl.  q / o / d_o / dq / dk / dv rows are indexed by b; the key-padding mask and the dropout
    // element index by bl (what pass p's own launch would use), the query mask is qmask + p * qmask_pstride, the dropout site
    // drop_site + p * site_pstride; kv_shared: k / v rows are image bl's for every pass (cross-attention over the encoder memory).
    int pass_B = 0; long qmask_pstride = 0; unsigned site_pstride = 0; int kv_shared = 0;
    // train_attn_dec_bf16_kernel only, with pass_B and kv_shared: the launch has pass_B * H workgroups and each walks pass_loop passes of its
    // image (K / V staged once, dK / dV summed over the passes in the accumulators and stored once, rows of image bl)
    int pass_loop = 0;
    // train_attn_wide.h only (encoder self-attention past 128 tokens): each query row's log-sum-exp of the scaled scores, written by the
    // forward and read by the backward, and the backward's D = rowsum(dO o O); both [B, H, Lq]
    float* lse = nullptr; float* dsum = nullptr;
};
// (image over all passes, head) of a workgroup -> what the pass-batched launch indexes with; pass_B == 0 reduces to the plain launch
struct TrainAttnIdx { int bf, bl, bkv, h; const unsigned char* qmask; unsigned site; unsigned long long dblock; };
__device__ __forceinline__ TrainAttnIdx train_attn_idx(const TrainAttnArgs& a) {
    TrainAttnIdx x;
    x.bf = blockIdx.x / a.H; x.h = blockIdx.x % a.H;
    const int p = a.pass_B ? x.bf / a.pass_B : 0;
    x.bl = a.pass_B ? x.bf - p * a.pass_B : x.bf;
    x.bkv = a.kv_shared ? x.bl : x.bf;
    x.qmask = a.qmask ? a.qmask + (size_t)p * a.qmask_pstride : nullptr;
    x.site = a.drop_site + (unsigned)p * a.site_pstride;
    x.dblock = (unsigned long long)x.bl * a.H + x.h;
    return x;
}

constexpr int TA_QB = 32, TA_NACC = 32;

__host__ __device__ inline size_t train_attn_lds_floats(int Lq, int Lk, int hd, bool backward) {
    const int nq = Lq < TA_QB ? Lq : TA_QB;
    return (size_t)2 * Lk * (hd + 1) + (size_t)(backward ? 2 : 1) * nq * (hd + 1) + (size_t)(backward ? 3 : 1) * nq * (Lk + 1);
}

template <bool BACKWARD, int HD>
__global__ __launch_bounds__(256)
void train_attn_kernel(const TrainAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ta_smem[];
    constexpr int PAD = HD + 1;
    const int Lq = a.Lq, Lk = a.Lk, ldp = Lk + 1;
    const int nqmax = Lq < TA_QB ? Lq : TA_QB;
    float* Ks = ta_smem;                          // [Lk][PAD]
    float* Vs = Ks + (size_t)Lk * PAD;            // [Lk][PAD]
    float* Qs = Vs + (size_t)Lk * PAD;            // [nq][PAD]
    float* P = Qs + (size_t)nqmax * PAD;          // [nq][Lk + 1]
    float* dOs = P + (size_t)nqmax * ldp;         // [nq][PAD]      (backward only)
    float* dS = dOs + (size_t)nqmax * PAD;        // [nq][Lk + 1]   (backward only)
    float* PD = dS + (size_t)nqmax * ldp;         // [nq][Lk + 1]   (backward only) probabilities after dropout
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const TrainAttnIdx ix = train_attn_idx(a);
    const int b = ix.bf, h = ix.h;      // b: the image over all passes (rows of q / o / d_o / dq / dk / dv)

    for (int idx = tid; idx < Lk * HD; idx += 256) {
        const int j = idx / HD, d = idx % HD;
        const size_t g = ((size_t)ix.bkv * Lk + j) * a.ldkv + h * HD + d;
        Ks[j * PAD + d] = a.k[g];
        Vs[j * PAD + d] = a.v[g];
    }
    float gk[TA_NACC], gv[TA_NACC];
#pragma unroll
    for (int i = 0; i < TA_NACC; ++i) { gk[i] = 0.f; gv[i] = 0.f; }

    for (int q0 = 0; q0 < Lq; q0 += TA_QB) {
        const int nq = (Lq - q0) < TA_QB ? (Lq - q0) : TA_QB;
        __syncthreads();                          // the previous block's readers are done with Qs / P / dOs / dS
        for (int idx = tid; idx < nq * HD; idx += 256) {
            const int l = idx / HD, d = idx % HD;
            Qs[l * PAD + d] = a.q[(size_t)b * a.q_bstride + (size_t)(q0 + l) * a.ldq + h * HD + d];
            if (BACKWARD) dOs[l * PAD + d] = a.d_o[((size_t)b * Lq + q0 + l) * a.ldo + h * HD + d];
        }
        __syncthreads();
        // scores (and, backward, dP = dO V^T)
        for (int idx = tid; idx < nq * Lk; idx += 256) {
            const int l = idx / Lk, j = idx % Lk;
            float s = 0.f, dp = 0.f;
#pragma unroll
            for (int d = 0; d < HD; ++d) {
                s = fmaf(Qs[l * PAD + d], Ks[j * PAD + d], s);
                if (BACKWARD) dp = fmaf(dOs[l * PAD + d], Vs[j * PAD + d], dp);
            }
            const bool masked = (ix.qmask && ix.qmask[(size_t)(q0 + l) * Lk + j]) || (a.kmask && a.kmask[(size_t)ix.bl * a.ldkm + j]);
            P[l * ldp + j] = masked ? -INFINITY : s * a.scale;
            if (BACKWARD) dS[l * ldp + j] = dp;
        }
        __syncthreads();
        // soft-max over the keys, one wave per query row (and, backward, dS = P * (dP - sum_j dP P) * scale)
        for (int l = wave; l < nq; l += 4) {
            float mx = -INFINITY;
            for (int j = lane; j < Lk; j += 64) mx = fmaxf(mx, P[l * ldp + j]);
            mx = wave_max(mx);
            float sum = 0.f;
            for (int j = lane; j < Lk; j += 64) { const float e = expf(P[l * ldp + j] - mx); P[l * ldp + j] = e; sum += e; }
            const float inv = 1.0f / wave_sum(sum);
            const unsigned long long row = (ix.dblock * Lq + q0 + l) * Lk;
            float dot = 0.f;
            for (int j = lane; j < Lk; j += 64) {
                const float p = P[l * ldp + j] * inv;
                const float f = drop_factor(a.drop, ix.site, row + j);
                if (BACKWARD) {
                    P[l * ldp + j] = p;                       // soft-max output
                    PD[l * ldp + j] = p * f;                  // what multiplied V
                    const float dp = dS[l * ldp + j] * f;     // gradient w.r.t. the soft-max output
                    dS[l * ldp + j] = dp;
                    dot += dp * p;
                } else {
                    P[l * ldp + j] = p * f;
                }
            }
            if (BACKWARD) {
                dot = wave_sum(dot);
                for (int j = lane; j < Lk; j += 64) dS[l * ldp + j] = P[l * ldp + j] * (dS[l * ldp + j] - dot) * a.scale;
            }
        }
        __syncthreads();
        if (!BACKWARD) {
            for (int idx = tid; idx < nq * HD; idx += 256) {
                const int l = idx / HD, d = idx % HD;
                float o = 0.f;
                for (int j = 0; j < Lk; ++j) o = fmaf(P[l * ldp + j], Vs[j * PAD + d], o);
                a.o[((size_t)b * Lq + q0 + l) * a.ldo + h * HD + d] = o;
            }
        } else {
            for (int idx = tid; idx < nq * HD; idx += 256) {
                const int l = idx / HD, d = idx % HD;
                float g = 0.f;
                for (int j = 0; j < Lk; ++j) g = fmaf(dS[l * ldp + j], Ks[j * PAD + d], g);
                a.dq[((size_t)b * Lq + q0 + l) * a.lddq + h * HD + d] = g;
            }
#pragma unroll
            for (int i = 0; i < TA_NACC; ++i) {
                const int idx = tid + 256 * i;
                if (idx < Lk * HD) {
                    const int j = idx / HD, d = idx % HD;
                    for (int l = 0; l < nq; ++l) {
                        gk[i] = fmaf(dS[l * ldp + j], Qs[l * PAD + d], gk[i]);
                        gv[i] = fmaf(PD[l * ldp + j], dOs[l * PAD + d], gv[i]);
                    }
                }
            }
        }
    }
    if (BACKWARD) {
#pragma unroll
        for (int i = 0; i < TA_NACC; ++i) {
            const int idx = tid + 256 * i;
            if (idx < Lk * HD) {
                const int j = idx / HD, d = idx % HD;
                const size_t g = ((size_t)b * Lk + j) * a.lddkv + h * HD + d;
                a.dk[g] = a.kv_accumulate ? a.dk[g] + gk[i] : gk[i];
                a.dv[g] = a.kv_accumulate ? a.dv[g] + gv[i] : gv[i];
            }
        }
    }
}

// The encoder's attention (head width 64, no masks, no dropout, Lq % 32 == 0, Lk % 16 == 0, Lk <= 128) with its five products on
// the matrix cores (v_mfma_f32_16x16x4_f32, exact fp32): same LDS residency, query blocks and register-held dK / dV as above.
// MFMA conventions as in mfma_sgemm_kernel: lane (r16 = lane & 15, g = lane >> 4) feeds A[row r16][k g] and B[k g][col r16] and
// receives D[row 4 g + r][col r16], r = 0..3.
constexpr int TM_HD = 64, TM_QB = 32, TM_K = 128;      // head width, query rows per block, keys held (TM_K / 16 accumulator tiles per wave)
// bytes of dynamic LDS: K and V [Lk][65], Q (and dO) [32][65], P (and dS) [32][Lk + 1]
__host__ __device__ inline size_t train_attn_mfma_lds(int Lk, bool backward) {
    return sizeof(float) * ((size_t)2 * Lk * (TM_HD + 1) + (size_t)(backward ? 2 : 1) * TM_QB * ((TM_HD + 1) + (Lk + 1)));
}

template <bool BACKWARD>
__global__ __launch_bounds__(256)
void train_attn_mfma_kernel(const TrainAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) float ta_smem[];
    constexpr int HD = TM_HD, PAD = HD + 1, QB = TM_QB, MAXJT = TM_K / 16;
    const int Lq = a.Lq, Lk = a.Lk, ldp = Lk + 1, njt = Lk / 16;
    float* Ks = ta_smem;                          // [Lk][PAD]
    float* Vs = Ks + (size_t)Lk * PAD;            // [Lk][PAD]
    float* Qs = Vs + (size_t)Lk * PAD;            // [QB][PAD]
    float* P = Qs + (size_t)QB * PAD;             // [QB][Lk + 1]
    float* dOs = P + (size_t)QB * ldp;            // [QB][PAD]      (backward only)
    float* dS = dOs + (size_t)QB * PAD;           // [QB][Lk + 1]   (backward only)
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;

    for (int idx = tid; idx < Lk * HD; idx += 256) {
        const int j = idx / HD, d = idx % HD;
        const size_t gi = ((size_t)b * Lk + j) * a.ldkv + h * HD + d;
        Ks[j * PAD + d] = a.k[gi];
        Vs[j * PAD + d] = a.v[gi];
    }
    f32x4 gk[MAXJT], gv[MAXJT];                   // dK / dV tiles (key tile jt, head columns [16 wave, +16)) of this wave
#pragma unroll
    for (int i = 0; i < MAXJT; ++i) { gk[i] = f32x4{0.f, 0.f, 0.f, 0.f}; gv[i] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    for (int q0 = 0; q0 < Lq; q0 += QB) {
        __syncthreads();
        for (int idx = tid; idx < QB * HD; idx += 256) {
            const int l = idx / HD, d = idx % HD;
            Qs[l * PAD + d] = a.q[(size_t)b * a.q_bstride + (size_t)(q0 + l) * a.ldq + h * HD + d];
            if (BACKWARD) dOs[l * PAD + d] = a.d_o[((size_t)b * Lq + q0 + l) * a.ldo + h * HD + d];
        }
        __syncthreads();
        // S = Q K^T (and dP = dO V^T): key tiles wave, wave + 4 for both 16-row halves of the query block
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            const int jt = wave + 4 * jj;
            if (jt < njt) {
                f32x4 sacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
                f32x4 pacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 4
                for (int ks = 0; ks < HD / 4; ++ks) {
                    const float kb = Ks[(16 * jt + r16) * PAD + 4 * ks + g];
                    const float q0v = Qs[r16 * PAD + 4 * ks + g], q1v = Qs[(16 + r16) * PAD + 4 * ks + g];
                    sacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(q0v, kb, sacc[0], 0, 0, 0);
                    sacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(q1v, kb, sacc[1], 0, 0, 0);
                    if (BACKWARD) {
                        const float vb = Vs[(16 * jt + r16) * PAD + 4 * ks + g];
                        const float o0 = dOs[r16 * PAD + 4 * ks + g], o1 = dOs[(16 + r16) * PAD + 4 * ks + g];
                        pacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(o0, vb, pacc[0], 0, 0, 0);
                        pacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(o1, vb, pacc[1], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int lt = 0; lt < 2; ++lt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int at = (16 * lt + 4 * g + r) * ldp + 16 * jt + r16;
                        P[at] = sacc[lt][r] * a.scale;
                        if (BACKWARD) dS[at] = pacc[lt][r];
                    }
            }
        }
        __syncthreads();
        // soft-max over the keys, one wave per query row (and, backward, dS = P * (dP - sum_j dP P) * scale)
        for (int l = wave; l < QB; l += 4) {
            float mx = -INFINITY;
            for (int j = lane; j < Lk; j += 64) mx = fmaxf(mx, P[l * ldp + j]);
            mx = wave_max(mx);
            float sum = 0.f;
            for (int j = lane; j < Lk; j += 64) { const float e = expf(P[l * ldp + j] - mx); P[l * ldp + j] = e; sum += e; }
            const float inv = 1.0f / wave_sum(sum);
            float dot = 0.f;
            for (int j = lane; j < Lk; j += 64) {
                const float p = P[l * ldp + j] * inv;
                P[l * ldp + j] = p;
                if (BACKWARD) dot += dS[l * ldp + j] * p;
            }
            if (BACKWARD) {
                dot = wave_sum(dot);
                for (int j = lane; j < Lk; j += 64) dS[l * ldp + j] = P[l * ldp + j] * (dS[l * ldp + j] - dot) * a.scale;
            }
        }
        __syncthreads();
        // O = P V (forward) / dQ = dS K (backward): head columns [16 wave, +16) for both halves of the query block
        {
            const float* L_ = BACKWARD ? dS : P;
            const float* R_ = BACKWARD ? Ks : Vs;
            f32x4 oacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
#pragma unroll 4
            for (int ks = 0; ks < Lk / 4; ++ks) {
                const float rb = R_[(4 * ks + g) * PAD + 16 * wave + r16];
                const float l0 = L_[r16 * ldp + 4 * ks + g], l1 = L_[(16 + r16) * ldp + 4 * ks + g];
                oacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(l0, rb, oacc[0], 0, 0, 0);
                oacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(l1, rb, oacc[1], 0, 0, 0);
            }
            float* dst = BACKWARD ? a.dq : a.o;
            const int ldd = BACKWARD ? a.lddq : a.ldo;
#pragma unroll
            for (int lt = 0; lt < 2; ++lt)
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    dst[((size_t)b * Lq + q0 + 16 * lt + 4 * g + r) * ldd + h * HD + 16 * wave + r16] = oacc[lt][r];
        }
        if (BACKWARD) {
            // dK += dS^T Q, dV += P^T dO over the 32 query rows of the block: every key tile, head columns [16 wave, +16)
            // (ks is NOT unrolled: with all 64 (ks, jt) bodies in flight the scheduler hoists 128 LDS loads and spills 2000 VGPRs)
#pragma unroll 1
            for (int ks = 0; ks < QB / 4; ++ks) {
                const float qb = Qs[(4 * ks + g) * PAD + 16 * wave + r16];
                const float ob = dOs[(4 * ks + g) * PAD + 16 * wave + r16];
#pragma unroll
                for (int jt = 0; jt < MAXJT; ++jt) {
                    if (jt < njt) {
                        const float sa = dS[(4 * ks + g) * ldp + 16 * jt + r16];
                        const float pa = P[(4 * ks + g) * ldp + 16 * jt + r16];
                        gk[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(sa, qb, gk[jt], 0, 0, 0);
                        gv[jt] = __builtin_amdgcn_mfma_f32_16x16x4f32(pa, ob, gv[jt], 0, 0, 0);
                    }
                }
            }
        }
    }
    if (BACKWARD) {
#pragma unroll
        for (int jt = 0; jt < MAXJT; ++jt) {
            if (jt < njt) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const size_t gi = ((size_t)b * Lk + 16 * jt + 4 * g + r) * a.lddkv + h * HD + 16 * wave + r16;
                    a.dk[gi] = a.kv_accumulate ? a.dk[gi] + gk[jt][r] : gk[jt][r];
                    a.dv[gi] = a.kv_accumulate ? a.dv[gi] + gv[jt][r] : gv[jt][r];
                }
            }
        }
    }
}

// -------------------------------------------------------------------------------------------------------------------
// Encoder attention of the training step in the bf16-operand mode (train_precision = bf16): 128 tokens, head width 64, no masks, no
// dropout — the five products S = Q K^T, O = P V, dP = dO V^T, dQ = dS K, dK = dS^T Q, dV = P^T dO on v_mfma_f32_16x16x32_bf16 with
// fp32 accumulation, soft-max and its backward in fp32 registers (the fp32 mode keeps train_attn_mfma_kernel: exact 16x16x4 products).
// One workgroup of four waves per (image, head); the queries are walked in two blocks of 64, wave w owns the block's query tile w.
//   S^T = K Q^T is computed (A = K rows, B = Q rows): lane (r16, g) then holds, for ITS query l = r16, the scores of keys
//   16 jt + 4 g + r — the soft-max over the keys is a reduction over the lane's registers and the four lane groups (rows4_max / sum),
//   and the probabilities are already the B operand (k-slots = keys) of O^T = V^T P^T and, backward, dS^T of dQ^T = K^T dS^T: no LDS
//   round trip between the score product and the products that contract over the keys (the inference kernel's trick,
//   encoder_attn.h).  The products that contract over the QUERIES (dK, dV) need P^T / dS^T with lanes indexed by key: those go
//   through LDS as bf16 [key][query] images, written two bytes at a time; the operands indexed by head column with a token k-axis
//   (V^T, K^T, Q^T, dO^T) are staged transposed once.
// Rounding points of the mode: q, k, v, dO (operands), p and dS (operands of the second-level products) are rounded to bf16;
// everything else is fp32.  MFMA conventions as everywhere (common.h mma16): result lane (r16, g) holds D[row 4 g + r][col r16].
// -------------------------------------------------------------------------------------------------------------------
constexpr int TB_N = 128, TB_HD = 64, TB_QB = 64;
constexpr int attn_bf16_pitch(int n) { return n + 8; }      // elements per row of an LDS image of n bf16: 16 bytes past the row, conflict-free ds_read_b128
constexpr int TB_RP = attn_bf16_pitch(TB_HD);          // pitch of [token][d] images (144 B rows)
constexpr int TB_TP = attn_bf16_pitch(TB_N);           // pitch of [d][key] images (V^T, K^T)
constexpr int TB_PP = attn_bf16_pitch(TB_QB);          // pitch of [key][query in block] / [d][query in block] images

// The LDS map of the two bf16 kernels, in elements from the start of the dynamic LDS, for `keys` keys held, head width hd and query
// blocks of qb rows: K [keys][hd + 8]; backward: V likewise; X^T [hd][keys + 8] (forward: V^T, backward: K^T); Q [qb][hd + 8]; and,
// backward only, dO [qb][hd + 8], Q^T and dO^T [hd][qb + 8], P^T and dS^T [keys][qb + 8].  The kernels take their pointers from it
// and the launch its byte count (`end`), so a size and its layout cannot drift apart.
struct AttnBf16Map { int k, v, xt, q, d_o, qt, d_ot, pt, dst, end; };
constexpr AttnBf16Map attn_bf16_map(int keys, int hd, int qb, bool backward) {
    // image sizes, [rows][columns + 8]: keys x head, queries x head, head x keys, head x queries, keys x queries
    const int kxd = keys * attn_bf16_pitch(hd), qxd = qb * attn_bf16_pitch(hd), dxk = hd * attn_bf16_pitch(keys), dxq = hd * attn_bf16_pitch(qb),
              kxq = keys * attn_bf16_pitch(qb);
    AttnBf16Map m{};
    m.k = 0; m.v = m.k + kxd; m.xt = backward ? m.v + kxd : m.v; m.q = m.xt + dxk; m.d_o = m.q + qxd;
    m.qt = backward ? m.d_o + qxd : m.d_o; m.d_ot = m.qt + dxq; m.pt = m.d_ot + dxq; m.dst = m.pt + kxq;
    m.end = backward ? m.dst + kxq : m.d_o;
    return m;
}
constexpr size_t train_attn_bf16_lds(bool backward) { return sizeof(bf16_t) * (size_t)attn_bf16_map(TB_N, TB_HD, TB_QB, backward).end; }

// Staging of both bf16 kernels: rows [0, MAXR) of a [*, HD] fp32 matrix (src: row 0, row stride ld) -> bf16 row-major image (pitch RP)
// and / or transposed image (dst_t[d][row], pitch tp); NT threads, 16-byte global loads.  nr: the rows the source has, rows_out (<= MAXR):
// the rows of the images to write — BOUNDED: rows >= nr are staged as zeros and rows >= rows_out are not written; otherwise both are
// MAXR and neither is looked at.
// All of a call's loads are issued before the first conversion (MAXR is a compile-time row count: the loop form was compiled to one load,
// `s_waitcnt vmcnt(0)`, its LDS stores, next load ... — a full memory round trip per 16 bytes and thread, most of the first version's time).
template <bool ROWS, bool TRANS, int HD, int NT, int RP, int MAXR, bool BOUNDED>
__device__ __forceinline__ void attn_bf16_stage(const float* __restrict__ src, long ld, bf16_t* dst_r, bf16_t* dst_t, int tp, int tid, int nr, int rows_out) {
    static_assert(HD == 32 || HD == 64, "head width");
    constexpr int IT = MAXR * (HD / 4) / NT, SH = HD == 64 ? 4 : 3, CM = HD / 4 - 1;      // 16-byte pieces per thread; piece -> (row, column) by shift and mask
    float4 ld4[IT];
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + NT * it, row = idx >> SH;
        if constexpr (BOUNDED) {
            ld4[it] = make_float4(0.f, 0.f, 0.f, 0.f);
            if (row < nr) ld4[it] = *reinterpret_cast<const float4*>(src + (size_t)row * ld + (idx & CM) * 4);
        } else {
            ld4[it] = *reinterpret_cast<const float4*>(src + (size_t)row * ld + (idx & CM) * 4);
        }
    }
#pragma unroll
    for (int it = 0; it < IT; ++it) {
        const int idx = tid + NT * it, row = idx >> SH, c4 = (idx & CM) * 4;
        if constexpr (BOUNDED) { if (row >= rows_out) continue; }
        const float4 v = ld4[it];
        const bf16_t e0 = static_cast<bf16_t>(v.x), e1 = static_cast<bf16_t>(v.y), e2 = static_cast<bf16_t>(v.z), e3 = static_cast<bf16_t>(v.w);
        if constexpr (ROWS) {
            bf16x4 o; o[0] = e0; o[1] = e1; o[2] = e2; o[3] = e3;
            *reinterpret_cast<bf16x4*>(dst_r + row * RP + c4) = o;
        }
        if constexpr (TRANS) {
            dst_t[(c4 + 0) * tp + row] = e0; dst_t[(c4 + 1) * tp + row] = e1;
            dst_t[(c4 + 2) * tp + row] = e2; dst_t[(c4 + 3) * tp + row] = e3;
        }
    }
}

// A fragment of a [d][key] image (pitch TP) for the key k-slot order of the S^T accumulators: lane (d = row0 + r16, g), k-step kk (32 keys):
// slots 0-3 = keys 32 kk + 4 g + [0, 4), slots 4-7 = keys 32 kk + 16 + 4 g + [0, 4)
template <int TP>
__device__ __forceinline__ Frag<bf16_t> keyslot_frag(const bf16_t* img, int row, int kk, int g) {
    const bf16x4 lo = *reinterpret_cast<const bf16x4*>(img + row * TP + 32 * kk + 4 * g);
    const bf16x4 hi = *reinterpret_cast<const bf16x4*>(img + row * TP + 32 * kk + 16 + 4 * g);
    Frag<bf16_t> f;
    f.v[0] = lo[0]; f.v[1] = lo[1]; f.v[2] = lo[2]; f.v[3] = lo[3]; f.v[4] = hi[0]; f.v[5] = hi[1]; f.v[6] = hi[2]; f.v[7] = hi[3];
    return f;
}

template <bool BACKWARD>
__global__ __launch_bounds__(256)
void train_attn_bf16_kernel(const TrainAttnArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char tb_smem[];
    constexpr AttnBf16Map M = attn_bf16_map(TB_N, TB_HD, TB_QB, BACKWARD);
    bf16_t* smem = reinterpret_cast<bf16_t*>(tb_smem);
    bf16_t* Ks = smem + M.k;                                        // [128][TB_RP]  K
    bf16_t* Vs = smem + M.v;                                        // backward: [128][TB_RP] V
    bf16_t* XT = smem + M.xt;                                       // [64][TB_TP]  forward: V^T; backward: K^T
    bf16_t* Qs = smem + M.q;                                        // [64][TB_RP]  Q block
    bf16_t* dOs = smem + M.d_o;                                     // backward: [64][TB_RP] dO block
    bf16_t* Qt = smem + M.qt;                                       // backward: [64 d][TB_PP] Q^T block
    bf16_t* dOt = smem + M.d_ot;                                    // backward: [64 d][TB_PP] dO^T block
    bf16_t* Pt = smem + M.pt;                                       // backward: [128 key][TB_PP] P^T
    bf16_t* dSt = smem + M.dst;                                     // backward: [128 key][TB_PP] dS^T
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.x / a.H, h = blockIdx.x % a.H;
    const float sl2 = a.scale * 1.44269504088896340736f;           // scale * log2(e): p = exp2((s - max) * sl2)

    const float* kg = a.k + (size_t)b * TB_N * a.ldkv + h * TB_HD;
    const float* vg = a.v + (size_t)b * TB_N * a.ldkv + h * TB_HD;
    if constexpr (BACKWARD) {
        attn_bf16_stage<true, true, TB_HD, 256, TB_RP, TB_N, false>(kg, a.ldkv, Ks, XT, TB_TP, tid, TB_N, TB_N);
        attn_bf16_stage<true, false, TB_HD, 256, TB_RP, TB_N, false>(vg, a.ldkv, Vs, nullptr, 0, tid, TB_N, TB_N);
    } else {
        attn_bf16_stage<true, false, TB_HD, 256, TB_RP, TB_N, false>(kg, a.ldkv, Ks, nullptr, 0, tid, TB_N, TB_N);
        attn_bf16_stage<false, true, TB_HD, 256, TB_RP, TB_N, false>(vg, a.ldkv, nullptr, XT, TB_TP, tid, TB_N, TB_N);
    }
    f32x4 gk[2][4], gv[2][4];                    // backward: dK / dV of key tiles 2 wave + {0, 1}, head-column tiles 0..3
    if constexpr (BACKWARD) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) { gk[jj][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; gv[jj][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }
    }

    for (int q0 = 0; q0 < TB_N; q0 += TB_QB) {
        __syncthreads();                         // the previous block's readers of Qs / dOs / Qt / dOt / Pt / dSt are done
        const float* qg = a.q + (size_t)b * a.q_bstride + (size_t)q0 * a.ldq + h * TB_HD;
        if constexpr (BACKWARD) {
            attn_bf16_stage<true, true, TB_HD, 256, TB_RP, TB_QB, false>(qg, a.ldq, Qs, Qt, TB_PP, tid, TB_QB, TB_QB);
            attn_bf16_stage<true, true, TB_HD, 256, TB_RP, TB_QB, false>(a.d_o + ((size_t)b * TB_N + q0) * a.ldo + h * TB_HD, a.ldo, dOs, dOt, TB_PP, tid, TB_QB, TB_QB);
        } else {
            attn_bf16_stage<true, false, TB_HD, 256, TB_RP, TB_QB, false>(qg, a.ldq, Qs, nullptr, 0, tid, TB_QB, TB_QB);
        }
        __syncthreads();
        // ---- S^T (and dP^T) of this wave's 16 queries against all 128 keys
        Frag<bf16_t> qf[2], of[2];
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            qf[ks].v = *reinterpret_cast<const bf16x8*>(Qs + (16 * wave + r16) * TB_RP + 32 * ks + 8 * g);
            if constexpr (BACKWARD) of[ks].v = *reinterpret_cast<const bf16x8*>(dOs + (16 * wave + r16) * TB_RP + 32 * ks + 8 * g);
        }
        f32x4 sacc[8], pacc[8];
#pragma unroll
        for (int jt = 0; jt < 8; ++jt) {
            sacc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
            if constexpr (BACKWARD) pacc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                Frag<bf16_t> kf;
                kf.v = *reinterpret_cast<const bf16x8*>(Ks + (16 * jt + r16) * TB_RP + 32 * ks + 8 * g);
                mma16(sacc[jt], kf, qf[ks]);
                if constexpr (BACKWARD) {
                    Frag<bf16_t> vf;
                    vf.v = *reinterpret_cast<const bf16x8*>(Vs + (16 * jt + r16) * TB_RP + 32 * ks + 8 * g);
                    mma16(pacc[jt], vf, of[ks]);
                }
            }
        }
        // ---- soft-max over the keys of query l = r16: registers, then the four lane groups
        float mx = -INFINITY;
#pragma unroll
        for (int jt = 0; jt < 8; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) mx = fmaxf(mx, sacc[jt][r]);
        mx = rows4_max(mx);
        float sum = 0.f;
#pragma unroll
        for (int jt = 0; jt < 8; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f((sacc[jt][r] - mx) * sl2); sacc[jt][r] = e; sum += e; }
        sum = rows4_sum(sum);
        const float inv = 1.0f / sum;
        if constexpr (!BACKWARD) {
            // ---- O^T = V^T P^T with the un-normalised probabilities as the B operand; 1 / sum applied to the result
            Frag<bf16_t> pf[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int s8 = 0; s8 < 8; ++s8) pf[kk].v[s8] = static_cast<bf16_t>(sacc[2 * kk + (s8 >> 2)][s8 & 3]);
            float* og = a.o + ((size_t)b * TB_N + q0 + 16 * wave + r16) * a.ldo + h * TB_HD;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                f32x4 oacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) mma16(oacc, keyslot_frag<TB_TP>(XT, 16 * dt + r16, kk, g), pf[kk]);
                // oacc[r] = O[query r16][d = 16 dt + 4 g + r]
                if (a.o16) {
                    union { uint2 u; bf16_t e[4]; } h;
#pragma unroll
                    for (int r = 0; r < 4; ++r) h.e[r] = static_cast<bf16_t>(oacc[r] * inv);
                    *reinterpret_cast<uint2*>(a.o16 + (og - a.o) + 16 * dt + 4 * g) = h.u;
                } else
                *reinterpret_cast<f32x4*>(og + 16 * dt + 4 * g) = oacc * inv;
            }
        } else {
            // ---- dS^T = P^T * (dP^T - sum_j P dP) * scale; P^T and dS^T to LDS ([key][query]) for the products over the queries
            float dot = 0.f;
#pragma unroll
            for (int jt = 0; jt < 8; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) { sacc[jt][r] *= inv; dot += sacc[jt][r] * pacc[jt][r]; }
            dot = rows4_sum(dot);
#pragma unroll
            for (int jt = 0; jt < 8; ++jt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float p = sacc[jt][r];
                    const float ds = p * (pacc[jt][r] - dot) * a.scale;
                    pacc[jt][r] = ds;
                    Pt[(16 * jt + 4 * g + r) * TB_PP + 16 * wave + r16] = static_cast<bf16_t>(p);
                    dSt[(16 * jt + 4 * g + r) * TB_PP + 16 * wave + r16] = static_cast<bf16_t>(ds);
                }
            // ---- dQ^T = K^T dS^T with dS^T straight from the registers (k-slots = keys)
            Frag<bf16_t> df[4];
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int s8 = 0; s8 < 8; ++s8) df[kk].v[s8] = static_cast<bf16_t>(pacc[2 * kk + (s8 >> 2)][s8 & 3]);
            float* dqg = a.dq + ((size_t)b * TB_N + q0 + 16 * wave + r16) * a.lddq + h * TB_HD;
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                f32x4 qacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int kk = 0; kk < 4; ++kk) mma16(qacc, keyslot_frag<TB_TP>(XT, 16 * dt + r16, kk, g), df[kk]);
                if (a.dq16) {
                    union { u32x2 u; bf16_t e[4]; } hq;
#pragma unroll
                    for (int r = 0; r < 4; ++r) hq.e[r] = static_cast<bf16_t>(qacc[r]);
                    *reinterpret_cast<u32x2*>(a.dq16 + (dqg - a.dq) + 16 * dt + 4 * g) = hq.u;
                } else
                *reinterpret_cast<f32x4*>(dqg + 16 * dt + 4 * g) = qacc;
            }
            __syncthreads();                     // P^T / dS^T of all 64 queries of the block are in LDS
            // ---- dV += P^T dO, dK += dS^T Q over the block's 64 queries: key tiles 2 wave + jj, every head-column tile
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                Frag<bf16_t> pa[2], sa[2];
#pragma unroll
                for (int jj = 0; jj < 2; ++jj) {
                    pa[jj].v = *reinterpret_cast<const bf16x8*>(Pt + (16 * (2 * wave + jj) + r16) * TB_PP + 32 * ks + 8 * g);
                    sa[jj].v = *reinterpret_cast<const bf16x8*>(dSt + (16 * (2 * wave + jj) + r16) * TB_PP + 32 * ks + 8 * g);
                }
#pragma unroll
                for (int dt = 0; dt < 4; ++dt) {
                    Frag<bf16_t> ob, qb;
                    ob.v = *reinterpret_cast<const bf16x8*>(dOt + (16 * dt + r16) * TB_PP + 32 * ks + 8 * g);
                    qb.v = *reinterpret_cast<const bf16x8*>(Qt + (16 * dt + r16) * TB_PP + 32 * ks + 8 * g);
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        mma16(gv[jj][dt], ob, pa[jj]);       // transposed tiles: gv[r] = dV[key 16 jt + r16][d = 16 dt + 4 g + r] (16-byte stores below)
                        mma16(gk[jj][dt], qb, sa[jj]);
                    }
                }
            }
        }
    }
    if constexpr (BACKWARD) {
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int dt = 0; dt < 4; ++dt) {
                const size_t gi = ((size_t)b * TB_N + 16 * (2 * wave + jj) + r16) * a.lddkv + h * TB_HD + 16 * dt + 4 * g;
                if (a.dk16) {
                    union { u32x2 u; bf16_t e[4]; } hk, hv;
#pragma unroll
                    for (int r = 0; r < 4; ++r) { hk.e[r] = static_cast<bf16_t>(gk[jj][dt][r]); hv.e[r] = static_cast<bf16_t>(gv[jj][dt][r]); }
                    *reinterpret_cast<u32x2*>(a.dk16 + gi) = hk.u;
                    *reinterpret_cast<u32x2*>(a.dv16 + gi) = hv.u;
                    continue;
                }
                f32x4 ok_ = f32x4{0.f, 0.f, 0.f, 0.f}, ov_ = f32x4{0.f, 0.f, 0.f, 0.f};
                if (a.kv_accumulate) { ok_ = *reinterpret_cast<const f32x4*>(a.dk + gi); ov_ = *reinterpret_cast<const f32x4*>(a.dv + gi); }
                *reinterpret_cast<f32x4*>(a.dk + gi) = ok_ + gk[jj][dt];
                *reinterpret_cast<f32x4*>(a.dv + gi) = ov_ + gv[jj][dt];
            }
    }
}

// -------------------------------------------------------------------------------------------------------------------
// Decoder attention of the training step in the bf16-operand mode: head width 32, <= 32 queries (one block), <= 128 keys, torch-style
// boolean masks (query x key and per-image key padding) and dropout on the probabilities — the same arrangement as
// train_attn_bf16_kernel (S^T = K Q^T, lane = query; probabilities as the B operand of the key-contracting products; P^T / dS^T
// through LDS for dK / dV) at the decoder's shapes: one workgroup of TWO waves per (image, head), wave w owns query tile w and the
// key tiles jt = w (mod 2) of dK / dV.  Queries past Lq and keys past Lk are zero rows (keys additionally masked), so they
// contribute nothing and are never stored.  Dropout: the counter-based generator of train_attn_kernel, same element index
// ((b H + h) Lq + l) Lk + j, so the two kernels drop the same probabilities.
// -------------------------------------------------------------------------------------------------------------------
constexpr int TD_HD = 32, TD_Q = 32, TD_K = 128;
constexpr int TD_RP = attn_bf16_pitch(TD_HD);          // pitch of [token][d] images (80-byte rows)
constexpr int TD_PP = attn_bf16_pitch(TD_Q);           // pitch of [key][query] and [d][query] images
// KT: the 16-key tiles the instantiation holds — 8 (128 keys: the cross-attention over the encoder memory) or 2 (32 keys: the self-attention
// over <= 26 context positions, whose workgroups then take a quarter of the LDS and a third of the registers: 27 648 of them per step
// batch, each a chain of dependent memory round trips, so what the launch needs is more of them resident)
constexpr size_t train_attn_dec_lds(bool backward, int KT = 8) { return sizeof(bf16_t) * (size_t)attn_bf16_map(16 * KT, TD_HD, TD_Q, backward).end; }

template <bool BACKWARD, int KT = 8>
__global__ __launch_bounds__(128)
void train_attn_dec_bf16_kernel(const TrainAttnArgs a) {
    static_assert(KT == 2 || KT == 8, "key tiles per instantiation");
    constexpr int KMAX = 16 * KT, TP = attn_bf16_pitch(KMAX), KK = KT / 2, JJ = KT / 2;      // keys held, pitch of the [d][key] image, 32-key k-steps, key tiles per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char td_smem[];
    constexpr AttnBf16Map M = attn_bf16_map(KMAX, TD_HD, TD_Q, BACKWARD);
    bf16_t* smem = reinterpret_cast<bf16_t*>(td_smem);
    bf16_t* Ks = smem + M.k;                                        // [KMAX][TD_RP]  K
    bf16_t* Vs = smem + M.v;                                        // backward: [KMAX][TD_RP] V
    bf16_t* XT = smem + M.xt;                                       // [32][TP]  forward: V^T; backward: K^T
    bf16_t* Qs = smem + M.q;                                        // [32][TD_RP]  Q
    bf16_t* dOs = smem + M.d_o;                                     // backward: [32][TD_RP] dO
    bf16_t* Qt = smem + M.qt;                                       // backward: [32 d][TD_PP] Q^T
    bf16_t* dOt = smem + M.d_ot;                                    // backward: [32 d][TD_PP] dO^T
    bf16_t* Pt = smem + M.pt;                                       // backward: [KMAX key][TD_PP] (P * dropout factor)^T
    bf16_t* dSt = smem + M.dst;                                     // backward: [KMAX key][TD_PP] dS^T
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const TrainAttnIdx ix = train_attn_idx(a);
    const int h = ix.h;
    const int Lq = a.Lq, Lk = a.Lk;
    const int njt = (Lk + 15) >> 4, nkk = (njt + 1) >> 1, NKP = 32 * nkk;      // key tiles, 32-key k-steps, padded key count
    const float sl2 = a.scale * 1.44269504088896340736f;
    // pass_loop (> 1, with pass_B and kv_shared): ONE workgroup per (image bl, head) walks that image's pass_loop permutation passes — K / V
    // are staged once for all of them and dK / dV accumulate in the matrix-core accumulators across the passes, one store at the end
    // (the cross-attention over the encoder memory: its K | V and their gradients are 300 MB per pass otherwise).  Else one pass: p0.
    const int npass = a.pass_loop > 1 ? a.pass_loop : 1;

    const float* kg = a.k + (size_t)ix.bkv * Lk * a.ldkv + h * TD_HD;
    const float* vg = a.v + (size_t)ix.bkv * Lk * a.ldkv + h * TD_HD;
    if constexpr (BACKWARD) {
        attn_bf16_stage<true, true, TD_HD, 128, TD_RP, KMAX, true>(kg, a.ldkv, Ks, XT, TP, tid, Lk, NKP);
        attn_bf16_stage<true, false, TD_HD, 128, TD_RP, KMAX, true>(vg, a.ldkv, Vs, nullptr, 0, tid, Lk, NKP);
    } else {
        attn_bf16_stage<true, false, TD_HD, 128, TD_RP, KMAX, true>(kg, a.ldkv, Ks, nullptr, 0, tid, Lk, NKP);
        attn_bf16_stage<false, true, TD_HD, 128, TD_RP, KMAX, true>(vg, a.ldkv, nullptr, XT, TP, tid, Lk, NKP);
    }
    f32x4 gkacc[JJ][2], gvacc[JJ][2];                                // backward: dK / dV tiles (jj, dt) of this wave, over the passes
#pragma unroll
    for (int jj = 0; jj < JJ; ++jj)
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) { gkacc[jj][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; gvacc[jj][dt] = f32x4{0.f, 0.f, 0.f, 0.f}; }

    for (int pp = 0; pp < npass; ++pp) {
    // b: the image over all passes (rows of q / o / d_o / dq); with pass_loop the launch's images are bl and the passes come from the loop
    const int b = a.pass_loop > 1 ? pp * a.pass_B + ix.bl : ix.bf;
    const unsigned char* qmask = a.pass_loop > 1 ? (a.qmask ? a.qmask + (size_t)pp * a.qmask_pstride : nullptr) : ix.qmask;
    const unsigned site = a.pass_loop > 1 ? a.drop_site + (unsigned)pp * a.site_pstride : ix.site;
    const float* qg = a.q + (size_t)b * a.q_bstride + h * TD_HD;
    if (pp) __syncthreads();                     // the previous pass's readers are done with Q / dO / P^T / dS^T
    if constexpr (BACKWARD) {
        attn_bf16_stage<true, true, TD_HD, 128, TD_RP, TD_Q, true>(qg, a.ldq, Qs, Qt, TD_PP, tid, Lq, TD_Q);
        attn_bf16_stage<true, true, TD_HD, 128, TD_RP, TD_Q, true>(a.d_o + (size_t)b * Lq * a.ldo + h * TD_HD, a.ldo, dOs, dOt, TD_PP, tid, Lq, TD_Q);
    } else {
        attn_bf16_stage<true, false, TD_HD, 128, TD_RP, TD_Q, true>(qg, a.ldq, Qs, nullptr, 0, tid, Lq, TD_Q);
    }
    __syncthreads();

    // ---- S^T (and dP^T) of this wave's 16 queries; one 32-wide k-step over the head width
    const int l = 16 * wave + r16;                                  // this lane's query
    Frag<bf16_t> qf, of;
    qf.v = *reinterpret_cast<const bf16x8*>(Qs + l * TD_RP + 8 * g);
    if constexpr (BACKWARD) of.v = *reinterpret_cast<const bf16x8*>(dOs + l * TD_RP + 8 * g);
    f32x4 sacc[KT], pacc[KT];
    float fdrop[KT][4];                                             // backward: dropout factor of (query l, key)
    const unsigned long long drow = (ix.dblock * Lq + l) * Lk;
    float mx = -INFINITY;
#pragma unroll
    for (int jt = 0; jt < KT; ++jt) {
        sacc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if constexpr (BACKWARD) pacc[jt] = f32x4{0.f, 0.f, 0.f, 0.f};
        if (jt < 2 * nkk) {
            Frag<bf16_t> kf;
            kf.v = *reinterpret_cast<const bf16x8*>(Ks + (16 * jt + r16) * TD_RP + 8 * g);
            mma16(sacc[jt], kf, qf);
            if constexpr (BACKWARD) {
                Frag<bf16_t> vf;
                vf.v = *reinterpret_cast<const bf16x8*>(Vs + (16 * jt + r16) * TD_RP + 8 * g);
                mma16(pacc[jt], vf, of);
            }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 16 * jt + 4 * g + r;
            bool masked = j >= Lk;
            if (!masked && l < Lq) masked = (qmask && qmask[(size_t)l * Lk + j]) || (a.kmask && a.kmask[(size_t)ix.bl * a.ldkm + j]);
            if (masked) sacc[jt][r] = -INFINITY;
            mx = fmaxf(mx, sacc[jt][r]);
        }
    }
    mx = rows4_max(mx);
    float sum = 0.f;
#pragma unroll
    for (int jt = 0; jt < KT; ++jt)
#pragma unroll
        for (int r = 0; r < 4; ++r) { const float e = __builtin_amdgcn_exp2f((sacc[jt][r] - mx) * sl2); sacc[jt][r] = e; sum += e; }
    sum = rows4_sum(sum);
    const float inv = 1.0f / sum;
    if constexpr (!BACKWARD) {
        // ---- O^T = V^T (P f)^T: un-normalised probabilities times the dropout factor as the B operand, 1 / sum on the result
        Frag<bf16_t> pf[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
#pragma unroll
            for (int s8 = 0; s8 < 8; ++s8) {
                const int jt = 2 * kk + (s8 >> 2), r = s8 & 3, j = 16 * jt + 4 * g + r;
                float e = sacc[jt][r];
                if (a.drop.thresh && j < Lk && l < Lq) e *= drop_factor(a.drop, site, drow + j);
                pf[kk].v[s8] = static_cast<bf16_t>(e);
            }
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            f32x4 oacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                if (kk < nkk) mma16(oacc, keyslot_frag<TP>(XT, 16 * dt + r16, kk, g), pf[kk]);
            if (l < Lq) *reinterpret_cast<f32x4*>(a.o + ((size_t)b * Lq + l) * a.ldo + h * TD_HD + 16 * dt + 4 * g) = oacc * inv;
        }
    } else {
        // ---- P = e / sum;  PD = P f (what multiplied V);  dp = dP f;  dS = P (dp - sum_j dp P) scale
        float dot = 0.f;
#pragma unroll
        for (int jt = 0; jt < KT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = 16 * jt + 4 * g + r;
                const float f = (a.drop.thresh && j < Lk && l < Lq) ? drop_factor(a.drop, site, drow + j) : 1.0f;
                fdrop[jt][r] = f;
                sacc[jt][r] *= inv;
                pacc[jt][r] *= f;
                dot += sacc[jt][r] * pacc[jt][r];
            }
        dot = rows4_sum(dot);
#pragma unroll
        for (int jt = 0; jt < KT; ++jt)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float p = sacc[jt][r];
                const float ds = p * (pacc[jt][r] - dot) * a.scale;
                pacc[jt][r] = ds;
                if (jt < 2 * nkk) {
                    Pt[(16 * jt + 4 * g + r) * TD_PP + l] = static_cast<bf16_t>(p * fdrop[jt][r]);
                    dSt[(16 * jt + 4 * g + r) * TD_PP + l] = static_cast<bf16_t>(ds);
                }
            }
        // ---- dQ^T = K^T dS^T, dS^T from the registers
        Frag<bf16_t> df[KK];
#pragma unroll
        for (int kk = 0; kk < KK; ++kk)
#pragma unroll
            for (int s8 = 0; s8 < 8; ++s8) df[kk].v[s8] = static_cast<bf16_t>(pacc[2 * kk + (s8 >> 2)][s8 & 3]);
#pragma unroll
        for (int dt = 0; dt < 2; ++dt) {
            f32x4 qacc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kk = 0; kk < KK; ++kk)
                if (kk < nkk) mma16(qacc, keyslot_frag<TP>(XT, 16 * dt + r16, kk, g), df[kk]);
            if (l < Lq) *reinterpret_cast<f32x4*>(a.dq + ((size_t)b * Lq + l) * a.lddq + h * TD_HD + 16 * dt + 4 * g) = qacc;
        }
        __syncthreads();                         // (P f)^T and dS^T of all 32 queries are in LDS
        // ---- dV += (P f)^T dO, dK += dS^T Q over the 32 queries (one k-step): key tiles jt = wave, wave + 2, ...
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
            const int jt = wave + 2 * jj;
            if (jt < njt) {
                Frag<bf16_t> pa, sa;
                pa.v = *reinterpret_cast<const bf16x8*>(Pt + (16 * jt + r16) * TD_PP + 8 * g);
                sa.v = *reinterpret_cast<const bf16x8*>(dSt + (16 * jt + r16) * TD_PP + 8 * g);
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    Frag<bf16_t> ob, qb;
                    ob.v = *reinterpret_cast<const bf16x8*>(dOt + (16 * dt + r16) * TD_PP + 8 * g);
                    qb.v = *reinterpret_cast<const bf16x8*>(Qt + (16 * dt + r16) * TD_PP + 8 * g);
                    // the TRANSPOSED tiles (operands swapped: the same products in the same order): a lane holds four consecutive head
                    // columns of ONE key — gv[r] = dV[key 16 jt + r16][d = 16 dt + 4 g + r] — so the read-modify-write of dK / dV is one
                    // 16-byte access per lane and tile instead of four 4-byte ones
                    mma16(gvacc[jj][dt], ob, pa);
                    mma16(gkacc[jj][dt], qb, sa);
                }
            }
        }
    }
    }      // passes
    if constexpr (BACKWARD) {
        // dK / dV leave once: rows of image ix.bf (pass_loop: ix.bl — one copy for all the passes), added to the old values if kv_accumulate
        const int bo = a.pass_loop > 1 ? ix.bl : ix.bf;
#pragma unroll
        for (int jj = 0; jj < JJ; ++jj) {
            const int jt = wave + 2 * jj, j = 16 * jt + r16;
            if (jt < njt && j < Lk) {
#pragma unroll
                for (int dt = 0; dt < 2; ++dt) {
                    const size_t gi = ((size_t)bo * Lk + j) * a.lddkv + h * TD_HD + 16 * dt + 4 * g;
                    f32x4 ok_ = f32x4{0.f, 0.f, 0.f, 0.f}, ov_ = f32x4{0.f, 0.f, 0.f, 0.f};      // old values (accumulate): both requested before the first store
                    if (a.kv_accumulate) { ok_ = *reinterpret_cast<const f32x4*>(a.dk + gi); ov_ = *reinterpret_cast<const f32x4*>(a.dv + gi); }
                    *reinterpret_cast<f32x4*>(a.dk + gi) = ok_ + gkacc[jj][dt];
                    *reinterpret_cast<f32x4*>(a.dv + gi) = ov_ + gvacc[jj][dt];
                }
            }
        }
    }
}

}  // namespace pq
