// The in-flight AR decode as ONE launch (bf16x3 arithmetic, PARSeq-S geometry, 24-bit K / V rows): a workgroup owns 16 images and
// carries them through all the steps of the loop alone.
//
// The mid / cross-attention / mlp arrangement of decoder_step.h was laid out for the latency of a forward that has the device to itself:
// the cross-attention is a whole-chip launch of one workgroup per image, the MLP is split over six workgroups per row tile.  With batches
// in flight on other streams nobody waits for that latency; what counts is the compute-unit time the decoder takes from the encoder
// launches (profiles/r05_timeline_in_flight.md: 10.8 k CU-us per step).  Nothing in a step crosses images once the cross-attention is
// done by the workgroup that owns the rows, so here a tile's workgroup runs, per step and in today's order,
//
//   [finish step i - 1: decoder.norm -> head -> logits -> greedy pick -> EOS bookkeeping]
//   table self-attention -> out_proj + position query -> norm1 -> q-projection (scaled, into LDS)
//   cross-attention of the tile's 16 images (decoder_attn.h ca24_pair: its 8 waves take the 16 x 12 (image, head) pairs round-robin)
//   cross out_proj + residual -> norm2 -> the six 256-unit hidden slices one after another (linear1 + GELU -> linear2)
//
// with the residual tile, the activations and the picked tokens in LDS / registers from the first step to the last: no exchange between
// workgroups, no grid barrier, no wait on another workgroup.  It streams 16 x 295 KB of K / V and 6.7 MB of weights per step through one
// compute unit; the pieces (ds_wave_gemm, ds_prefetch, ds_layernorm_rows, ds_self_attn_rows, the parameter staging, the pick helpers) are
// decoder_step.h's.
//
// Bit-identity with the three-launch form (dec_step_mid_kernel<E, true, 1>, dec_cross_attn_ar24_kernel<E, false>, dec_step_mlp_kernel<E, true>) is the
// contract: every accumulator receives the same products in the same order — each hidden slice has its own linear2 accumulator, and
// the residual is summed ((t' + b2) + p0) + ... + p5 as the mid kernel sums the partials.
#pragma once
#include "decoder_step.h"

namespace pq {

struct ArTileArgs {
    int M, num_steps, C, testing, eos_id, ldt, ntok, npos;
    float eps, scale;
    // finish
    const float *b2, *lnf_w, *lnf_b, *bh; const bf16_t* Wh;
    float* logits; unsigned char* eos_seen; int *eos_rows, *ar_len, *ar_last;
    // start
    const float *stab, *kvtab; int* tok;
    const bf16_t *Wo, *Wq; const float *bo, *pos_queries, *ln1_w, *ln1_b, *bq;
    // cross-attention
    const unsigned char *kmem, *vmem; size_t plane_elems;
    // cross out_proj + MLP
    const bf16_t *Wco, *W1, *W2; const float *bco, *ln2_w, *ln2_b, *b1;
};

// lnf w | lnf b | head bias (128) | bo | pos query of the step | ln1 w | ln1 b | bq | bco | ln2 w | ln2 b | b2   (b1, 4 E, stays in global memory)
template <int E> constexpr int ds_loop_params() { return 11 * E + 128; }
template <int E> constexpr size_t dec_ar_tile_loop_lds() {
    return (size_t)DS_ROWS * ((E + 8) * 2 * 2 + (E + 4) * 4 + (4 * E / ds_split<E>() + 8) * 2 * 2 + 128 * 4) + (size_t)ds_loop_params<E>() * 4 + (size_t)DS_NW * DS_RING * 1024;
}

template <int E, bool X3>
__global__ __launch_bounds__(64 * DS_NW)
void dec_ar_tile_loop_kernel(const ArTileArgs a) {
    static_assert(X3 && E == 384, "built for the bf16x3 arithmetic at embed_dim 384");
    static_assert(DS_ROWS == CA_TILE && DS_NW == CA_TILE_NW, "the cross-attention's tile is the step kernels' row tile");
    constexpr int H = E / DEC_HD, PA = E + 8, PT = E + 4, TILES = E / 16, TN = (TILES + DS_NW - 1) / DS_NW, PL = 128, RPW = DS_ROWS / DS_NW;
    constexpr int DS_SPLIT = ds_split<E>(), F = 4 * E, FS = F / DS_SPLIT, PH = FS + 8, TN1 = FS / 16 / DS_NW;
    static_assert(FS % (16 * DS_NW) == 0 && FS % 64 == 0, "hidden width must split evenly over the slices and waves");
    constexpr int NPL = 2, ALO = DS_ROWS * PA, HLO = DS_ROWS * PH;      // planes per operand; element offsets of the lo planes
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_ds[];
    static_assert((size_t)DS_ROWS * E * 4 <= (size_t)NPL * DS_ROWS * PH * 2 + (size_t)DS_ROWS * PL * 4, "the queries fit where they are parked");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, r16 = lane & 15, g = lane >> 4;
    const int row0 = (int)blockIdx.x * DS_ROWS, M = a.M, C = a.C, num_steps = a.num_steps;
    float* __restrict__ logits = a.logits;

    // the context tokens live in registers from step to step: lane j of tokv[rr] holds token j of row 2 wave + rr
    int picked[RPW], tokv[RPW], seen[RPW];
#pragma unroll
    for (int rr = 0; rr < RPW; ++rr) {
        picked[rr] = -1; seen[rr] = 0;
        tokv[rr] = lane == 0 ? a.tok[(size_t)min(row0 + wave * RPW + rr, M - 1) * a.ldt] : 0;
    }
    static_assert(E <= 64 * DS_NW, "one parameter per thread and segment");

#pragma unroll 1
    for (int pos = 0; pos <= num_steps; ++pos) {
        const bool do_start = pos < num_steps;
        // Every address below is derived anew in each step from values the compiler cannot see through: hoisted out of the loop, the lane
        // addresses of six weight streams and of the LDS tiles stayed live across all phases and spilled into the weight stream.
        int lds0 = 0;
        const bf16_t* Wh = a.Wh; const bf16_t* Wo = a.Wo; const bf16_t* Wq = a.Wq; const bf16_t* Wco = a.Wco; const bf16_t* W1 = a.W1; const bf16_t* W2 = a.W2;
        const float* b1 = a.b1;
        asm volatile("" : "+s"(lds0), "+s"(Wh), "+s"(Wo), "+s"(Wq), "+s"(Wco), "+s"(W1), "+s"(W2), "+s"(b1));
        bf16_t* abuf = reinterpret_cast<bf16_t*>(smem_ds + lds0);          // [NPL][DS_ROWS][PA]
        float* tl = reinterpret_cast<float*>(abuf + NPL * DS_ROWS * PA);    // [DS_ROWS][PT]
        bf16_t* hbuf = reinterpret_cast<bf16_t*>(tl + DS_ROWS * PT);       // [NPL][DS_ROWS][PH]
        float* lg = reinterpret_cast<float*>(hbuf + NPL * DS_ROWS * PH);   // [DS_ROWS][PL]
        float* qs = reinterpret_cast<float*>(hbuf);                        // [DS_ROWS][E] scaled queries: over hbuf | lg, both dead between the pick and the MLP
        float* prm = lg + DS_ROWS * PL;                                    // [ds_loop_params<E>()]
        float* const s_lnf_w = prm, * const s_lnf_b = prm + E, * const s_bh = prm + 2 * E, * const s_bo = prm + 2 * E + 128, * const s_posq = prm + 3 * E + 128,
             * const s_ln1_w = prm + 4 * E + 128, * const s_ln1_b = prm + 5 * E + 128, * const s_bq = prm + 6 * E + 128, * const s_bco = prm + 7 * E + 128,
             * const s_ln2_w = prm + 8 * E + 128, * const s_ln2_b = prm + 9 * E + 128, * const s_b2 = prm + 10 * E + 128;
        unsigned char* wring = reinterpret_cast<unsigned char*>(prm + ds_loop_params<E>()) + wave * DS_RING * 1024;
        if (pos == 0) {
            float* const prm_dst[11] = {s_lnf_w, s_lnf_b, s_bh, s_bo, s_ln1_w, s_ln1_b, s_bq, s_bco, s_ln2_w, s_ln2_b, s_b2};
            const float* const prm_src[11] = {a.lnf_w, a.lnf_b, a.bh, a.bo, a.ln1_w, a.ln1_b, a.bq, a.bco, a.ln2_w, a.ln2_b, a.b2};
            const int prm_n[11] = {E, E, 128, E, E, E, E, E, E, E, E}, prm_valid[11] = {E, E, C, E, E, E, E, E, E, E, E};
            float prm_v[11];
            ds_params_load<11>(prm_v, prm_src, prm_valid);
            ds_params_store<11>(prm_v, prm_dst, prm_n, prm_valid);
            ds_prefetch<E, TN, NPL>(Wo, TILES, wave, wring);
        }
        if (pos > 0) {
            // ---- finish step pos - 1: tl holds t'' = ((t' + b2) + p0) + ... + p5; the ring holds the head's first fragments ----
            ds_layernorm_rows<E, X3>(tl, PT, abuf, PA, s_lnf_w, s_lnf_b, a.eps, wave, ALO);
            __syncthreads();
            {
                f32x4 acc[1] = {};
                ds_wave_gemm<E, 1, true, NPL>(abuf, PA, Wh, (C + 15) / 16, wave, wring, acc, 0, 0, ALO);
                if (do_start) ds_prefetch<E, TN, NPL>(Wo, TILES, wave, wring);
                const int n = wave * 16 + 4 * g;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (n + r < C) {
                        const float v = acc[0][r] + s_bh[n + r];
                        lg[r16 * PL + n + r] = v;
                        if (row0 + r16 < M) logits[((size_t)(row0 + r16) * num_steps + (pos - 1)) * C + n + r] = v;
                    }
                }
            }
            __syncthreads();                                     // lg complete; abuf free for the next step's self-attention
            if (do_start) {                                      // the pick of position pos - 1 feeds step pos
#pragma unroll
                for (int rr = 0; rr < RPW; ++rr) {
                    const int row = wave * RPW + rr, b = row0 + row;
                    float best = -INFINITY; int bi = ARGMAX_NONE;
                    for (int c = lane; c < C; c += 64) {
                        const float v = lg[row * PL + c];
                        if (argmax_take(v, c, best, bi)) { best = v; bi = c; }
                    }
                    wave_argmax(best, bi);
                    bi = argmax_final(bi, C);
                    picked[rr] = bi;
                    if (lane == 0 && b < M) {
                        a.tok[(size_t)b * a.ldt + pos] = bi;
                        if (a.testing && bi == a.eos_id && !seen[rr]) {
                            // Tiles are not in step with each other, so the row that completes the count need not be the one that finished
                            // last: every row leaves its own first-<eos> position in a running maximum BEFORE it is counted, and whoever
                            // completes the count publishes that maximum (= the step at which the three-launch form sees the last row finish).
                            seen[rr] = 1; a.eos_seen[b] = 1;
                            atomicMax(a.ar_last, pos);                // = (finished step) + 1
                            __threadfence();
                            const int done = atomicAdd(a.eos_rows, 1) + 1;
                            if (done == M) { __threadfence(); *a.ar_len = atomicMax(a.ar_last, 0); }
                        }
                    }
                }
            }
        }
        if (!do_start) break;

        // ---- start step pos ----
        const int Lk = pos + 1;
        if (threadIdx.x < E) s_posq[threadIdx.x] = a.pos_queries[(size_t)min(pos, a.npos - 1) * E + threadIdx.x];      // read behind the next barrier
        {
#pragma unroll
            for (int rr = 0; rr < RPW; ++rr)
                if (picked[rr] >= 0 && lane == pos) tokv[rr] = picked[rr];
            ds_self_attn_rows<E, X3, RPW>(a.stab, a.kvtab, tokv, a.ntok, a.npos, Lk, pos, abuf + wave * RPW * PA, PA, ALO);
        }
        __syncthreads();
        {   // t = pos_queries[pos] + sa @ Wo^T + bo
            f32x4 acc[TN] = {};
            ds_wave_gemm<E, TN, true, NPL>(abuf, PA, Wo, TILES, wave, wring, acc, 0, 0, ALO);
            ds_prefetch<E, TN, NPL>(Wq, TILES, wave, wring);
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const int tile = wave + DS_NW * t;
                if (tile < TILES) {
                    const int n = tile * 16 + 4 * g;
                    const float4 bv = *reinterpret_cast<const float4*>(s_bo + n);
                    const float4 pv = *reinterpret_cast<const float4*>(s_posq + n);
                    f32x4 o = {acc[t][0] + bv.x + pv.x, acc[t][1] + bv.y + pv.y, acc[t][2] + bv.z + pv.z, acc[t][3] + bv.w + pv.w};
                    *reinterpret_cast<f32x4*>(tl + r16 * PT + n) = o;
                }
            }
        }
        __syncthreads();
        ds_layernorm_rows<E, X3>(tl, PT, abuf, PA, s_ln1_w, s_ln1_b, a.eps, wave, ALO);
        __syncthreads();
        {   // q = (norm1(t) @ Wq^T + bq) * scale, parked in LDS for the cross-attention
            f32x4 acc[TN] = {};
            ds_wave_gemm<E, TN, true, NPL>(abuf, PA, Wq, TILES, wave, wring, acc, 0, 0, ALO);
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const int tile = wave + DS_NW * t;
                if (tile < TILES) {
                    const int n = tile * 16 + 4 * g;
                    const float4 bv = *reinterpret_cast<const float4*>(s_bq + n);
                    const f32x4 o = {acc[t][0] + bv.x, acc[t][1] + bv.y, acc[t][2] + bv.z, acc[t][3] + bv.w};
                    const f32x4 q = {o[0] * a.scale, o[1] * a.scale, o[2] * a.scale, o[3] * a.scale};
                    *reinterpret_cast<f32x4*>(qs + r16 * E + n) = q;
                }
            }
        }
        __syncthreads();                                         // qs complete; abuf (norm1's rows) free for the attention's output

        // ---- cross-attention of the tile's images; the f32 result is split into the bf16 pair cross out_proj multiplies ----
        {
            const int kl = lane / 4, dl = lane % 4;
#pragma unroll 1
            for (int pr = wave; pr < DS_ROWS * H; pr += DS_NW) {
                const int img = pr / H, h = pr - img * H, b = row0 + img;
                if (b >= M) break;                                 // rows past the batch: nothing of theirs is ever written out
                float acc[8];
                ca24_pair(a.kmem, a.vmem, a.plane_elems, (size_t)b * H + h, qs + img * E + h * DEC_HD, acc, [] {});
                if (kl == 0) {
                    bf16x8 hi, lo;
#pragma unroll
                    for (int j = 0; j < 8; ++j) { hi[j] = from_f32<bf16_t>(acc[j]); lo[j] = from_f32<bf16_t>(acc[j] - to_f32(hi[j])); }
                    *reinterpret_cast<bf16x8*>(abuf + img * PA + h * DEC_HD + dl * 8) = hi;
                    *reinterpret_cast<bf16x8*>(abuf + ALO + img * PA + h * DEC_HD + dl * 8) = lo;
                }
            }
        }
        ds_prefetch<E, TN, NPL>(Wco, TILES, wave, wring);
        __syncthreads();
        {   // t' = t + ca @ Wco^T + bco
            f32x4 acc[TN] = {};
            ds_wave_gemm<E, TN, true, NPL>(abuf, PA, Wco, TILES, wave, wring, acc, 0, 0, ALO);
            ds_prefetch<E, TN1, NPL>(W1, FS / 16, wave, wring);
#pragma unroll
            for (int t = 0; t < TN; ++t) {
                const int tile = wave + DS_NW * t;
                if (tile < TILES) {
                    const int n = tile * 16 + 4 * g;
                    const float4 bv = *reinterpret_cast<const float4*>(s_bco + n);
                    f32x4* p = reinterpret_cast<f32x4*>(tl + r16 * PT + n);
                    f32x4 o = *p;
                    o[0] += acc[t][0] + bv.x; o[1] += acc[t][1] + bv.y; o[2] += acc[t][2] + bv.z; o[3] += acc[t][3] + bv.w;
                    *p = o;
                }
            }
        }
        __syncthreads();
        ds_layernorm_rows<E, X3>(tl, PT, abuf, PA, s_ln2_w, s_ln2_b, a.eps, wave, ALO);
        __syncthreads();                                         // norm2 has read t': from here every lane sums into its own elements of tl
#pragma unroll 1
        for (int sp = 0; sp < DS_SPLIT; ++sp) {
            {   // h[:, slice] = gelu(norm2(t') @ W1[slice]^T + b1[slice])
                f32x4 acc[TN1] = {};
                ds_wave_gemm<E, TN1, true, NPL>(abuf, PA, W1 + (size_t)sp * (FS / 16) * (E / 64) * (1024 * NPL), FS / 16, wave, wring, acc, 0, 0, ALO);
                ds_prefetch<FS, TN, NPL>(W2, TILES, wave, wring, sp * (FS / 64), F / 64);
#pragma unroll
                for (int t = 0; t < TN1; ++t) {
                    const int n = (wave + DS_NW * t) * 16 + 4 * g;
                    const float4 bv = *reinterpret_cast<const float4*>(b1 + sp * FS + n);
                    const float o[4] = {gelu_erf(acc[t][0] + bv.x), gelu_erf(acc[t][1] + bv.y), gelu_erf(acc[t][2] + bv.z), gelu_erf(acc[t][3] + bv.w)};
                    float ol[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) ol[j] = o[j] - to_f32(from_f32<bf16_t>(o[j]));
                    store4<bf16_t>(hbuf + r16 * PH + n, o);
                    store4<bf16_t>(hbuf + HLO + r16 * PH + n, ol);
                }
            }
            __syncthreads();
            {   // p[slice] = h[:, slice] @ W2[:, slice]^T in an accumulator of its own; t'' = ((t' + b2) + p0) + ... in slice order
                f32x4 acc[TN] = {};
                ds_wave_gemm<FS, TN, true, NPL>(hbuf, PH, W2, TILES, wave, wring, acc, sp * (FS / 64), F / 64, HLO);
                if (sp + 1 < DS_SPLIT) ds_prefetch<E, TN1, NPL>(W1 + (size_t)(sp + 1) * (FS / 16) * (E / 64) * (1024 * NPL), FS / 16, wave, wring);
                else ds_prefetch<E, 1, NPL>(Wh, (C + 15) / 16, wave, wring);
#pragma unroll
                for (int t = 0; t < TN; ++t) {
                    const int tile = wave + DS_NW * t;
                    if (tile < TILES) {
                        const int n = tile * 16 + 4 * g;
                        f32x4* p = reinterpret_cast<f32x4*>(tl + r16 * PT + n);
                        f32x4 v = *p;
                        if (sp == 0) {
                            const float4 bv = *reinterpret_cast<const float4*>(s_b2 + n);
                            v[0] += bv.x; v[1] += bv.y; v[2] += bv.z; v[3] += bv.w;
                        }
                        v += acc[t];
                        *p = v;
                    }
                }
            }
            __syncthreads();                                     // hbuf free for the next slice; after the last one tl is complete
        }
    }
}

}  // namespace pq
