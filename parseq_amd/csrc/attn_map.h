// Character localisation: the head-averaged cross-attention map of a decoder pass, and its reduction to geometry.
//
// Every cross-attention kernel of decoder_attn.h keeps its probabilities in registers or LDS and writes the value mix only.  The map
// kernel here recomputes the soft-max of the pass's queries against the memory's K rows — V is never read — and writes
//     A[b][i][t] = mean_h softmax_t(q[b][h][i] . K[b][h][t] / sqrt(32))          fp32 [B][L][S]
// Scores, soft-max and the head mean are fp32 whatever the plan's precision; only the storage of K differs (AM_K_*).
//
// Shape.  One workgroup of four waves per (image, block of AM_QB = 16 queries); a wave owns AM_QW = 4 queries for ALL heads, a lane owns the
// keys lane, lane + 64, ... (AM_KC = 4 chunks: S <= 256).  Per head the workgroup stages K[b][h] ([S][32]) once into LDS as fp32 at a row
// pitch of 33 words (lane t reads row t: conflict-free), each wave takes its four query rows of that head into one register each (lane d holds
// element d; the score loop broadcasts it with v_readlane, so the queries cost no LDS), and the soft-max reduces over the wave in a fixed
// order.  Because a wave keeps its queries through the whole head loop, the head sum is sixteen accumulator registers added in ascending head
// order: deterministic, and no reduction over heads through LDS or atomics.  A workgroup per (image, head, query block) would expose H times
// more parallelism but needs that cross-workgroup reduction; at 33 KiB of LDS four workgroups share a CU, and the batch sizes that matter
// (>= 64 images x 2 query blocks) already fill the 256 CUs.  The arithmetic is 2 H S 32 flops per query (0.65 GFLOP at batch 512) against one
// pass over K per query block: the kernel is bound by staging K, not by the FMAs, hence no matrix cores.
#pragma once
#include "common.h"
#include "decoder_attn.h"

namespace pq {

enum { AM_K_F32 = 0, AM_K_BF16 = 1, AM_K_F24 = 2 };      // storage of the K rows: f32, bf16, or the 24-bit u16 + u8 planes of decoder_attn.h
constexpr int AM_MAX_S = 256;                             // memory tokens at most
constexpr int AM_WAVES = 4, AM_QW = 4, AM_QB = AM_WAVES * AM_QW;
constexpr int AM_KC = AM_MAX_S / 64;
constexpr int AM_LDK = DEC_HD + 1;

// elements e .. e + 3 (e a multiple of 4) of the K array at `kmem`
template <int KM>
__device__ __forceinline__ void am_load4(const void* __restrict__ kmem, size_t plane_elems, size_t e, float (&v)[4]) {
    if constexpr (KM == AM_K_F32) {
        const float4 f = *reinterpret_cast<const float4*>(reinterpret_cast<const float*>(kmem) + e);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else if constexpr (KM == AM_K_BF16) {
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(kmem) + e);
        v[0] = __uint_as_float(u.x << 16); v[1] = __uint_as_float(u.x & 0xffff0000u);
        v[2] = __uint_as_float(u.y << 16); v[3] = __uint_as_float(u.y & 0xffff0000u);
    } else {
        // bits 31..16 in the u16 plane, bits 15..8 in the u8 plane plane_elems 2-byte elements behind it
        const uint2 u = *reinterpret_cast<const uint2*>(reinterpret_cast<const unsigned short*>(kmem) + e);
        const unsigned lo = *reinterpret_cast<const unsigned*>(reinterpret_cast<const unsigned char*>(kmem) + plane_elems * 2 + e);
        v[0] = __uint_as_float((u.x << 16) | ((lo & 0xffu) << 8));
        v[1] = __uint_as_float((u.x & 0xffff0000u) | (lo & 0xff00u));
        v[2] = __uint_as_float((u.y << 16) | ((lo >> 8) & 0xff00u));
        v[3] = __uint_as_float((u.y & 0xffff0000u) | ((lo >> 16) & 0xff00u));
    }
}

// qc [B * L][E]: the pass's cross-attention queries, projected, unscaled (what the per-operation decoder pass leaves in the plan);
// kmem [B][H][S][32]; kpm [B][ldk] or null: query row i of image b is a valid position iff !kpm[b][i] (the key-padding mask of the content
// starts one past the <eos> position); rows that are not are written as zeros.  grid (B, ceil(L / AM_QB)), 256 threads.
template <int KM>
__global__ __launch_bounds__(64 * AM_WAVES)
void dec_cross_attn_map_kernel(const float* __restrict__ qc, const void* __restrict__ kmem, size_t plane_elems,
                               const unsigned char* __restrict__ kpm, int ldk, int H, int L, int S, float scale, float* __restrict__ A) {
    __shared__ float ks[AM_MAX_S * AM_LDK];
    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6, b = blockIdx.x;
    const int E = H * DEC_HD;
    const int q0 = blockIdx.y * AM_QB + wid * AM_QW;
    float acc[AM_QW][AM_KC];
#pragma unroll
    for (int j = 0; j < AM_QW; ++j)
#pragma unroll
        for (int c = 0; c < AM_KC; ++c) acc[j][c] = 0.f;
    for (int h = 0; h < H; ++h) {
        __syncthreads();      // the previous head's rows have been read
        const size_t base = ((size_t)b * H + h) * (size_t)S * DEC_HD;
        for (int e = tid * 4; e < S * DEC_HD; e += 64 * AM_WAVES * 4) {
            float v[4];
            am_load4<KM>(kmem, plane_elems, base + e, v);
            float* dst = ks + (e >> 5) * AM_LDK + (e & 31);
            dst[0] = v[0]; dst[1] = v[1]; dst[2] = v[2]; dst[3] = v[3];
        }
        __syncthreads();
        float qr[AM_QW];
#pragma unroll
        for (int j = 0; j < AM_QW; ++j) {
            const int qi = q0 + j;
            qr[j] = qi < L ? qc[((size_t)b * L + qi) * E + h * DEC_HD + (lane & 31)] * scale : 0.f;
        }
        float s[AM_QW][AM_KC];
#pragma unroll
        for (int j = 0; j < AM_QW; ++j)
#pragma unroll
            for (int c = 0; c < AM_KC; ++c) s[j][c] = 0.f;
#pragma unroll
        for (int d = 0; d < DEC_HD; ++d) {
            float qd[AM_QW];
#pragma unroll
            for (int j = 0; j < AM_QW; ++j) qd[j] = lane_bcast(qr[j], d);
#pragma unroll
            for (int c = 0; c < AM_KC; ++c) {
                if (c * 64 < S) {      // uniform; rows S .. of the last chunk are never staged: read (inside ks) and masked below
                    const float kd = ks[(c * 64 + lane) * AM_LDK + d];
#pragma unroll
                    for (int j = 0; j < AM_QW; ++j) s[j][c] = fmaf(qd[j], kd, s[j][c]);
                }
            }
        }
#pragma unroll
        for (int j = 0; j < AM_QW; ++j) {
            float mx = -INFINITY;
#pragma unroll
            for (int c = 0; c < AM_KC; ++c) {
                const bool in = c * 64 + lane < S;
                s[j][c] = in ? s[j][c] : -INFINITY;
                mx = fmaxf(mx, s[j][c]);
            }
            mx = wave_max(mx);
            float sum = 0.f;
#pragma unroll
            for (int c = 0; c < AM_KC; ++c) {
                const bool in = c * 64 + lane < S;
                s[j][c] = in ? expf(s[j][c] - mx) : 0.f;
                sum += s[j][c];
            }
            sum = wave_sum(sum);
#pragma unroll
            for (int c = 0; c < AM_KC; ++c) acc[j][c] += s[j][c] / sum;      // heads in ascending order
        }
    }
#pragma unroll
    for (int j = 0; j < AM_QW; ++j) {
        const int qi = q0 + j;
        if (qi >= L) continue;
        const bool valid = !(kpm && kpm[(size_t)b * ldk + qi]);
        float* row = A + ((size_t)b * L + qi) * S;
#pragma unroll
        for (int c = 0; c < AM_KC; ++c) {
            const int t = c * 64 + lane;
            if (t < S) row[t] = valid ? acc[j][c] / (float)H : 0.f;
        }
    }
}

// Content rows of a reading: tok[b] = [bos, reading[b][0 .. L-2]] (model.py:161 with the reading in place of the arg-max).
static __global__ void attn_content_kernel(const int* __restrict__ reading, int B, int L, int bos_id, int* __restrict__ tok, int ldt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= B * L) return;
    const int b = i / L, j = i - b * L;
    tok[(size_t)b * ldt + j] = j == 0 ? bos_id : reading[(size_t)b * L + j - 1];
}

// From the content rows tok[b][0 .. L-1]: the key-padding mask kpm[b][j] = (an <eos> at a position <= j) (model.py:163; skipped when null),
// and what was localised: the reading of L positions (its characters, <eos> at position len, pad_id after) and len = the position of the
// first <eos> of the content minus one, or L - 1 without one (both skipped when null).  One thread per image.
static __global__ void attn_prep_kernel(const int* __restrict__ tok, int ldt, int B, int L, int eos_id, int pad_id,
                                        unsigned char* __restrict__ kpm, int ldk, int* __restrict__ reading, int* __restrict__ lengths) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int* row = tok + (size_t)b * ldt;
    int first = L;
    for (int j = L - 1; j >= 0; --j) if (row[j] == eos_id) first = j;
    if (kpm) for (int j = 0; j < L; ++j) kpm[(size_t)b * ldk + j] = j >= first ? 1 : 0;
    const int len = first - 1 < 0 ? 0 : first - 1;      // (an <eos> in the <bos> slot: an empty reading)
    if (lengths) lengths[b] = len;
    if (reading) for (int i = 0; i < L; ++i) reading[(size_t)b * L + i] = i < len ? row[i + 1] : (i == len ? eos_id : pad_id);
}

// The geometry of a map (section 21): one wave per row (b, i) of A [B][L][S]; token t is cell (t / gw, t % gw) of ph x pw pixels.  Valid rows
// (i <= lengths[b]):
//   centre = (sum A x_c, sum A y_r);  var = sum A (x_c - cx)^2 + pw^2 / 12 in a second pass;  box = centre -+ sqrt(3 var), clipped to the image;
//   peak = the arg-max token (lowest index on ties), peak_mass = its probability.
// Every sum is a lane's terms in ascending t, then wave_sum's fixed tree.  Invalid rows: zeros and peak -1.
static __global__ __launch_bounds__(256)
void attn_geometry_kernel(const float* __restrict__ A, const int* __restrict__ lengths, int rows, int L, int S, int gw, float ph, float pw,
                          float img_h, float img_w, float* __restrict__ centres, float* __restrict__ boxes, int* __restrict__ peak,
                          float* __restrict__ peak_mass) {
    const int lane = threadIdx.x & 63;
    const int w = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (w >= rows) return;
    const int b = w / L, i = w - b * L;
    if (i > lengths[b]) {
        if (lane < 2) centres[(size_t)w * 2 + lane] = 0.f;
        if (lane < 4) boxes[(size_t)w * 4 + lane] = 0.f;
        if (lane == 0) { peak[w] = -1; peak_mass[w] = 0.f; }
        return;
    }
    const float* row = A + (size_t)w * S;
    float sx = 0.f, sy = 0.f, best = -INFINITY; int bi = ARGMAX_NONE;
    for (int t = lane; t < S; t += 64) {
        const float a = row[t];
        const int r = t / gw, c = t - r * gw;
        sx = fmaf(a, ((float)c + 0.5f) * pw, sx);
        sy = fmaf(a, ((float)r + 0.5f) * ph, sy);
        if (argmax_take(a, t, best, bi)) { best = a; bi = t; }
    }
    const float cx = wave_sum(sx), cy = wave_sum(sy);
    wave_argmax(best, bi);
    float vx = 0.f, vy = 0.f;
    for (int t = lane; t < S; t += 64) {
        const float a = row[t];
        const int r = t / gw, c = t - r * gw;
        const float dx = ((float)c + 0.5f) * pw - cx, dy = ((float)r + 0.5f) * ph - cy;
        vx = fmaf(a, dx * dx, vx);
        vy = fmaf(a, dy * dy, vy);
    }
    // sqrt(3 (var + p^2 / 12)) = sqrt(3 var + p^2 / 4): a one-hot map gives half a cell exactly
    const float hx = sqrtf(fmaf(3.f, wave_sum(vx), 0.25f * pw * pw)), hy = sqrtf(fmaf(3.f, wave_sum(vy), 0.25f * ph * ph));
    if (lane == 0) {
        centres[(size_t)w * 2] = cx; centres[(size_t)w * 2 + 1] = cy;
        boxes[(size_t)w * 4] = fminf(fmaxf(cx - hx, 0.f), img_w);
        boxes[(size_t)w * 4 + 1] = fminf(fmaxf(cy - hy, 0.f), img_h);
        boxes[(size_t)w * 4 + 2] = fminf(fmaxf(cx + hx, 0.f), img_w);
        boxes[(size_t)w * 4 + 3] = fminf(fmaxf(cy + hy, 0.f), img_h);
        peak[w] = argmax_final(bi, S); peak_mass[w] = best;
    }
}

}  // namespace pq
