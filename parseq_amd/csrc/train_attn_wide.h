// Encoder attention of the training step past 128 tokens (ViTSTR: 129, PARSeq-patch16-224: 196; any N in (128, 256]), head width 64,
// non-causal, no masks, no dropout, fp32 operands in both training precisions.
//
// The kernels of train_attn.h keep a head's whole K / V (and, backward, its dK / dV) resident: in LDS that stops fitting at ~200 keys and
// in registers at 128.  Here the keys stream through LDS in 32-key tiles:
//   forward   one workgroup per (32-query block, image, head): S = Q K^T tile by tile, online soft-max, O = P V accumulated in
//             registers; writes O and each query row's log-sum-exp lse = max + log(sum) of the scaled scores ([B, H, N], `a.lse`).
//   dQ        one workgroup per (32-query block, image, head): D = rowsum(dO o O) of its rows (written to `a.dsum`, [B, H, N]), then
//             P = exp(S - lse), dS = P (dO V^T - D) scale and dQ = dS K over the key tiles.
//   dK / dV   one workgroup per (32-key block, image, head), launched after dQ (it reads D): dV = P^T dO, dK = dS^T Q over the query
//             blocks, P and dS recomputed from Q, K, lse and D.
// Every sum runs in a fixed order and every output element has one writer: no atomics, results bit-identical from run to run.
// Rows past N (the tail of the last block) are staged as zeros, their probabilities forced to 0, and nothing is stored for them.
// MFMA conventions as in train_attn_mfma_kernel: v_mfma_f32_16x16x4_f32 (exact fp32 products), lane (r16 = lane & 15, g = lane >> 4)
// feeds A[row r16][k g] and B[k g][col r16] and receives D[row 4 g + r][col r16], r = 0..3.
#pragma once

#include "train_attn.h"

constexpr int TW_HD = 64, TW_BLK = 32, TW_MAXN = 256;
constexpr int TW_PAD = TW_HD + 1;        // [row][d] images
constexpr int TW_PP = TW_BLK + 1;        // [query][key] tiles

// rows [r0, r0 + 32) of a [N, ld] fp32 matrix (src: row 0, head column 0) -> [32][TW_PAD] in LDS, zeros past row N; 16-byte loads
__device__ __forceinline__ void tw_stage(const float* __restrict__ src, long ld, int r0, int N, float* dst, int tid) {
#pragma unroll
    for (int it = 0; it < TW_BLK * TW_HD / 4 / 256; ++it) {
        const int idx = tid + 256 * it, l = idx >> 4, c4 = (idx & 15) * 4;
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (r0 + l < N) v = *reinterpret_cast<const float4*>(src + (size_t)(r0 + l) * ld + c4);
        float* d = dst + l * TW_PAD + c4;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

// 16 x 16 tile of X Y^T over the 64 head columns: rows [16 xt, +16) of X, rows [16 yt, +16) of Y (both [32][TW_PAD] images)
__device__ __forceinline__ f32x4 tw_dot_tile(const float* X, int xt, const float* Y, int yt, int r16, int g) {
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int ks = 0; ks < TW_HD / 4; ++ks)
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(X[(16 * xt + r16) * TW_PAD + 4 * ks + g], Y[(16 * yt + r16) * TW_PAD + 4 * ks + g], acc, 0, 0, 0);
    return acc;
}

// forward: grid (ceil(N / 32), B * H)
__global__ __launch_bounds__(256)
void train_attn_wide_fwd_kernel(const TrainAttnArgs a) {
    __shared__ float Qs[TW_BLK * TW_PAD], Ks[TW_BLK * TW_PAD], Vs[TW_BLK * TW_PAD], Ss[TW_BLK * TW_PP];
    __shared__ float alpha_s[TW_BLK], l_s[TW_BLK];
    const int N = a.Lk, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H, q0 = blockIdx.x * TW_BLK;
    const int lt = wave & 1, jt = wave >> 1;          // the score tile of this wave: queries [16 lt, +16), keys [16 jt, +16)
    const int srow = tid >> 3, spart = tid & 7;       // soft-max statistics: row srow, keys [4 spart, +4) of a tile
    tw_stage(a.q + (size_t)b * a.q_bstride + h * TW_HD, a.ldq, q0, N, Qs, tid);
    const float* kg = a.k + (size_t)b * N * a.ldkv + h * TW_HD;
    const float* vg = a.v + (size_t)b * N * a.ldkv + h * TW_HD;
    float m_run = -INFINITY, l_run = 0.f;
    f32x4 oacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};      // O rows [16 lt', +16), head columns [16 wave, +16)
    for (int k0 = 0; k0 < N; k0 += TW_BLK) {
        __syncthreads();                              // the previous tile's readers of Ks / Vs / Ss are done
        tw_stage(kg, a.ldkv, k0, N, Ks, tid);
        tw_stage(vg, a.ldkv, k0, N, Vs, tid);
        __syncthreads();
        {
            const f32x4 s = tw_dot_tile(Qs, lt, Ks, jt, r16, g);
#pragma unroll
            for (int r = 0; r < 4; ++r)
                Ss[(16 * lt + 4 * g + r) * TW_PP + 16 * jt + r16] = (k0 + 16 * jt + r16 < N) ? s[r] * a.scale : -INFINITY;
        }
        __syncthreads();
        {   // online soft-max: eight lanes per row (an aligned group of one wave), every lane of the group ends with the same statistics
            float* sr = Ss + srow * TW_PP + 4 * spart;
            float mx = fmaxf(fmaxf(sr[0], sr[1]), fmaxf(sr[2], sr[3]));
            mx = fmaxf(mx, __shfl_xor(mx, 1, 8)); mx = fmaxf(mx, __shfl_xor(mx, 2, 8)); mx = fmaxf(mx, __shfl_xor(mx, 4, 8));
            const float m_new = fmaxf(m_run, mx);     // finite: key 0 of every tile is a real key
            const float al = expf(m_run - m_new);
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < 4; ++c) { const float p = expf(sr[c] - m_new); sr[c] = p; sum += p; }
            sum += __shfl_xor(sum, 1, 8); sum += __shfl_xor(sum, 2, 8); sum += __shfl_xor(sum, 4, 8);
            l_run = l_run * al + sum;
            m_run = m_new;
            if (spart == 0) alpha_s[srow] = al;
        }
        __syncthreads();
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
            for (int r = 0; r < 4; ++r) oacc[t][r] *= alpha_s[16 * t + 4 * g + r];
#pragma unroll 4
        for (int ks = 0; ks < TW_BLK / 4; ++ks) {
            const float vb = Vs[(4 * ks + g) * TW_PAD + 16 * wave + r16];
            oacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ss[r16 * TW_PP + 4 * ks + g], vb, oacc[0], 0, 0, 0);
            oacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ss[(16 + r16) * TW_PP + 4 * ks + g], vb, oacc[1], 0, 0, 0);
        }
    }
    if (spart == 0) {
        l_s[srow] = l_run;
        if (q0 + srow < N) a.lse[((size_t)b * a.H + h) * N + q0 + srow] = m_run + logf(l_run);
    }
    __syncthreads();
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = 16 * t + 4 * g + r;
            if (q0 + l < N) a.o[((size_t)b * N + q0 + l) * a.ldo + h * TW_HD + 16 * wave + r16] = oacc[t][r] / l_s[l];
        }
}

// P and dS of one 16 x 16 (query, key) tile from the score and dO V^T accumulators: P = exp(S scale - lse), dS = P (dP - D) scale;
// zero where the query or the key is past N
__device__ __forceinline__ void tw_p_ds(const f32x4& s, const f32x4& dp, const float* lse_s, const float* D_s, int q_lo, int q_base, int k_col,
                                        int N, float scale, float* P, float* dS, int g) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int l = q_lo + 4 * g + r;
        const bool live = q_base + l < N && k_col < N;
        const float p = live ? expf(s[r] * scale - lse_s[l]) : 0.f;
        if (P) P[l * TW_PP] = p;
        dS[l * TW_PP] = p * (dp[r] - D_s[l]) * scale;
    }
}

// backward, dQ and D: grid (ceil(N / 32), B * H)
__global__ __launch_bounds__(256)
void train_attn_wide_dq_kernel(const TrainAttnArgs a) {
    __shared__ float Qs[TW_BLK * TW_PAD], dOs[TW_BLK * TW_PAD], Ks[TW_BLK * TW_PAD], Vs[TW_BLK * TW_PAD], dSs[TW_BLK * TW_PP];
    __shared__ float lse_s[TW_BLK], D_s[TW_BLK];
    const int N = a.Lk, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H, q0 = blockIdx.x * TW_BLK;
    const int lt = wave & 1, jt = wave >> 1;
    const size_t stat0 = ((size_t)b * a.H + h) * N;
    tw_stage(a.q + (size_t)b * a.q_bstride + h * TW_HD, a.ldq, q0, N, Qs, tid);
    tw_stage(a.d_o + (size_t)b * N * a.ldo + h * TW_HD, a.ldo, q0, N, dOs, tid);
    {   // D = rowsum(dO o O): eight lanes per row, eight head columns each
        const int row = tid >> 3, part = tid & 7;
        float d = 0.f;
        if (q0 + row < N) {
            const float* op = a.o + ((size_t)b * N + q0 + row) * a.ldo + h * TW_HD + 8 * part;
            const float* gp = a.d_o + ((size_t)b * N + q0 + row) * a.ldo + h * TW_HD + 8 * part;
            const float4 o0 = *reinterpret_cast<const float4*>(op), o1 = *reinterpret_cast<const float4*>(op + 4);
            const float4 g0 = *reinterpret_cast<const float4*>(gp), g1 = *reinterpret_cast<const float4*>(gp + 4);
            d = o0.x * g0.x + o0.y * g0.y + o0.z * g0.z + o0.w * g0.w + o1.x * g1.x + o1.y * g1.y + o1.z * g1.z + o1.w * g1.w;
        }
        d += __shfl_xor(d, 1, 8); d += __shfl_xor(d, 2, 8); d += __shfl_xor(d, 4, 8);
        if (part == 0) {
            D_s[row] = d;
            lse_s[row] = q0 + row < N ? a.lse[stat0 + q0 + row] : 0.f;
            if (q0 + row < N) a.dsum[stat0 + q0 + row] = d;
        }
    }
    const float* kg = a.k + (size_t)b * N * a.ldkv + h * TW_HD;
    const float* vg = a.v + (size_t)b * N * a.ldkv + h * TW_HD;
    f32x4 gacc[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};      // dQ rows [16 t, +16), head columns [16 wave, +16)
    for (int k0 = 0; k0 < N; k0 += TW_BLK) {
        __syncthreads();
        tw_stage(kg, a.ldkv, k0, N, Ks, tid);
        tw_stage(vg, a.ldkv, k0, N, Vs, tid);
        __syncthreads();
        {
            const f32x4 s = tw_dot_tile(Qs, lt, Ks, jt, r16, g);
            const f32x4 dp = tw_dot_tile(dOs, lt, Vs, jt, r16, g);
            tw_p_ds(s, dp, lse_s, D_s, 16 * lt, q0, k0 + 16 * jt + r16, N, a.scale, nullptr, dSs + 16 * jt + r16, g);
        }
        __syncthreads();
#pragma unroll 4
        for (int ks = 0; ks < TW_BLK / 4; ++ks) {
            const float kb = Ks[(4 * ks + g) * TW_PAD + 16 * wave + r16];
            gacc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(dSs[r16 * TW_PP + 4 * ks + g], kb, gacc[0], 0, 0, 0);
            gacc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(dSs[(16 + r16) * TW_PP + 4 * ks + g], kb, gacc[1], 0, 0, 0);
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int l = 16 * t + 4 * g + r;
            if (q0 + l < N) a.dq[((size_t)b * N + q0 + l) * a.lddq + h * TW_HD + 16 * wave + r16] = gacc[t][r];
        }
}

// backward, dK / dV: grid (ceil(N / 32), B * H), after train_attn_wide_dq_kernel (reads its D)
__global__ __launch_bounds__(256)
void train_attn_wide_dkv_kernel(const TrainAttnArgs a) {
    __shared__ float Ks[TW_BLK * TW_PAD], Vs[TW_BLK * TW_PAD], Qs[TW_BLK * TW_PAD], dOs[TW_BLK * TW_PAD], Ps[TW_BLK * TW_PP], dSs[TW_BLK * TW_PP];
    __shared__ float lse_s[TW_BLK], D_s[TW_BLK];
    const int N = a.Lk, tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int r16 = lane & 15, g = lane >> 4;
    const int b = blockIdx.y / a.H, h = blockIdx.y % a.H, k0 = blockIdx.x * TW_BLK;
    const int lt = wave & 1, jt = wave >> 1;
    const size_t stat0 = ((size_t)b * a.H + h) * N;
    tw_stage(a.k + (size_t)b * N * a.ldkv + h * TW_HD, a.ldkv, k0, N, Ks, tid);
    tw_stage(a.v + (size_t)b * N * a.ldkv + h * TW_HD, a.ldkv, k0, N, Vs, tid);
    const float* qg = a.q + (size_t)b * a.q_bstride + h * TW_HD;
    const float* og = a.d_o + (size_t)b * N * a.ldo + h * TW_HD;
    f32x4 gk[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};       // dK / dV rows (keys) [16 t, +16), head columns [16 wave, +16)
    f32x4 gv[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};
    for (int q0 = 0; q0 < N; q0 += TW_BLK) {
        __syncthreads();
        tw_stage(qg, a.ldq, q0, N, Qs, tid);
        tw_stage(og, a.ldo, q0, N, dOs, tid);
        if (tid < TW_BLK) {
            lse_s[tid] = q0 + tid < N ? a.lse[stat0 + q0 + tid] : 0.f;
            D_s[tid] = q0 + tid < N ? a.dsum[stat0 + q0 + tid] : 0.f;
        }
        __syncthreads();
        {
            const f32x4 s = tw_dot_tile(Qs, lt, Ks, jt, r16, g);
            const f32x4 dp = tw_dot_tile(dOs, lt, Vs, jt, r16, g);
            tw_p_ds(s, dp, lse_s, D_s, 16 * lt, q0, k0 + 16 * jt + r16, N, a.scale, Ps + 16 * jt + r16, dSs + 16 * jt + r16, g);
        }
        __syncthreads();
        // dV += P^T dO, dK += dS^T Q over the block's 32 queries: A[key r16][query k] = P[query][key], B[query k][d] = dO / Q
#pragma unroll 2
        for (int ks = 0; ks < TW_BLK / 4; ++ks) {
            const float ob = dOs[(4 * ks + g) * TW_PAD + 16 * wave + r16];
            const float qb = Qs[(4 * ks + g) * TW_PAD + 16 * wave + r16];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                gv[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(Ps[(4 * ks + g) * TW_PP + 16 * t + r16], ob, gv[t], 0, 0, 0);
                gk[t] = __builtin_amdgcn_mfma_f32_16x16x4f32(dSs[(4 * ks + g) * TW_PP + 16 * t + r16], qb, gk[t], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int j = 16 * t + 4 * g + r;
            if (k0 + j < N) {
                const size_t gi = ((size_t)b * N + k0 + j) * a.lddkv + h * TW_HD + 16 * wave + r16;
                a.dk[gi] = a.kv_accumulate ? a.dk[gi] + gk[t][r] : gk[t][r];
                a.dv[gi] = a.kv_accumulate ? a.dv[gi] + gv[t][r] : gv[t][r];
            }
        }
}
