// The row, loss, dropout and optimiser kernels of the training step: column sums, LayerNorm forward and
// backward (a wave per row), GELU and its backward, copies and sums, the decoder's content rows and embedding gradient, cross-entropy,
// the counter-based dropout (DropSpec / drop_factor) with its kernels, im2col of the patch embedding, the gradient norm and AdamW.
// All tensors are fp32 and row-major unless a kernel says otherwise (the bf16 shadows some of them write beside their fp32 output).
// These are plain kernels, bound by memory: each has a one-line CPU counterpart in oracle/decoder_backward.py, which is itself checked
// against autograd.  Kernels that accumulate say so; everything is deterministic (no atomics, every sum in a fixed order).
#pragma once
#include "common.h"

namespace pq {

// out[n] (+)= sum_m A[m * lda + n]: bias gradients, LayerNorm affine gradients, sums over the batch ([B, L * E] views).
// Many rows: two deterministic stages (row chunks -> partials, then this kernel again over the partials).
// 16 row groups x 64 columns per workgroup, rows added in a fixed order.  blockIdx.y = row chunk of `rows_per` rows; with more
// than one chunk the kernel writes out[chunk][n] (a partial, never accumulated into).
static __global__ __launch_bounds__(1024)
void colsum_kernel(const float* __restrict__ A, long lda, int M, int N, float* __restrict__ out, int accumulate, int rows_per,
                   float* __restrict__ out2 = nullptr, int split = 0) {      // out2 (single-chunk form only): columns >= split go to out2[n - split]
    __shared__ float part[16][64];
    const int c = threadIdx.x & 63, rg = threadIdx.x >> 6;
    const int n = blockIdx.x * 64 + c;
    const int m_lo = blockIdx.y * rows_per, m_hi = min(M, m_lo + rows_per);
    float s = 0.f;
    if (n < N)
        for (int m = m_lo + rg; m < m_hi; m += 16) s += A[(size_t)m * lda + n];
    part[rg][c] = s;
    __syncthreads();
    if (rg == 0 && n < N) {
        float t = 0.f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[i][c];
        float* o = (out2 && n >= split) ? out2 + (n - split) : out + (size_t)blockIdx.y * N + n;
        *o = (accumulate && gridDim.y == 1) ? *o + t : t;
    }
}

// LayerNorm forward of the training encoder, E <= 768 and even; one row per wave, a lane owns column pairs (2 lane + 128 i).  Two-pass
// statistics like rowops.h layernorm_kernel; the affine step is ONE explicit fma, so that the fp32 output and the bf16 output (the
// operand shadow of the products that follow, two elements per 4-byte store) are roundings of the same value whatever the compiler
// does with each instantiation (layernorm_kernel<float> and <bf16> contract it differently: 5 of 1.5 M elements a bf16 ulp apart).
template <typename TO>
__global__ __launch_bounds__(256)
void ln_fwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ b, TO* __restrict__ out, int rows, int E, float eps) {
    const int lane = threadIdx.x & 63, row = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const float* __restrict__ xr = x + (size_t)row * E;
    f32x2 v[6];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int c = 2 * lane + 128 * i;
        v[i] = c < E ? *reinterpret_cast<const f32x2*>(xr + c) : f32x2{0.f, 0.f};
        s += v[i][0] + v[i][1];
    }
    const float inv = 1.0f / (float)E;
    const float mean = wave_sum(s) * inv;
    float ss = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i)
        if (2 * lane + 128 * i < E) { const float d0 = v[i][0] - mean, d1 = v[i][1] - mean; ss += d0 * d0 + d1 * d1; }
    const float rstd = 1.0f / sqrtf(wave_sum(ss) * inv + eps);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int c = 2 * lane + 128 * i;
        if (c < E) {
            const f32x2 wv = *reinterpret_cast<const f32x2*>(w + c), bv = *reinterpret_cast<const f32x2*>(b + c);
            const float y0 = fmaf((v[i][0] - mean) * rstd, wv[0], bv[0]), y1 = fmaf((v[i][1] - mean) * rstd, wv[1], bv[1]);
            if constexpr (sizeof(TO) == 2) {
                union { unsigned u; bf16_t e[2]; } h;
                h.e[0] = static_cast<bf16_t>(y0); h.e[1] = static_cast<bf16_t>(y1);
                *reinterpret_cast<unsigned*>(out + (size_t)row * E + c) = h.u;
            } else {
                *reinterpret_cast<f32x2*>(out + (size_t)row * E + c) = f32x2{y0, y1};
            }
        }
    }
}

// LayerNorm backward, statistics recomputed from x (E <= 768); a workgroup owns LNB_ROWS consecutive rows, one wave per row at a time:
//   dx_out = (add ? add : 0) + rstd * (g - mean(g) - xhat * mean(g * xhat)),  g = dy * w
//   partial[chunk][0 .. E)   = sum over the chunk's rows of dy * xhat   (weight gradient)
//   partial[chunk][E .. 2E)  = sum over the chunk's rows of dy          (bias gradient)
// summed per lane over the wave's rows in ascending order, then over the four waves in wave order: deterministic.  The host folds the
// chunks with colsum_kernel.  (Round 3: the first form wrote dy * xhat as a [rows, E] matrix and ran two column-sum passes over it and
// over dy — 225 MB of extra traffic and two more launches per LayerNorm at 49 152 rows.)
constexpr int LNB_ROWS = 4;       // one row per wave: 64 and 32 rows per workgroup (a serial row loop per wave, even with the next row prefetched) ran the kernel at 68-75 us where one row per wave runs it at HBM speed
static __global__ __launch_bounds__(256)
void ln_bwd_kernel(const float* __restrict__ x, const float* __restrict__ w, const float* __restrict__ dy, const float* __restrict__ add,
                   float* __restrict__ dx_out, float* __restrict__ partial, int rows, int E, float eps, bf16_t* __restrict__ dx16) {
    __shared__ float red[4][2][768];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float pg[12], pb[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) { pg[i] = 0.f; pb[i] = 0.f; }
    const float inv = 1.0f / (float)E;
    const int r_first = blockIdx.x * LNB_ROWS + wave * (LNB_ROWS / 4);
    // the next row's x and dy are requested before the current row is worked on (the row loop is a chain of wave reductions: without
    // the prefetch every row paid its own memory round trip)
    float nx[12], nd[12];
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const int c = lane + 64 * i;
        const bool ok = c < E && r_first < rows;
        nx[i] = ok ? x[(size_t)r_first * E + c] : 0.f;
        nd[i] = ok ? dy[(size_t)r_first * E + c] : 0.f;
    }
    for (int rr = 0; rr < LNB_ROWS / 4; ++rr) {
        const int r = r_first + rr;
        if (r >= rows) break;
        const size_t base = (size_t)r * E;
        float xv[12], gv[12], dv[12];
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) { xv[i] = nx[i]; dv[i] = nd[i]; s += xv[i]; }
        if (rr + 1 < LNB_ROWS / 4 && r + 1 < rows) {
#pragma unroll
            for (int i = 0; i < 12; ++i) {
                const int c = lane + 64 * i;
                nx[i] = c < E ? x[base + E + c] : 0.f;
                nd[i] = c < E ? dy[base + E + c] : 0.f;
            }
        }
        const float mean = wave_sum(s) * inv;
        float ss = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int c = lane + 64 * i;
            const float d = c < E ? xv[i] - mean : 0.f;
            ss += d * d;
        }
        const float rstd = 1.0f / sqrtf(wave_sum(ss) * inv + eps);
        float s1 = 0.f, s2 = 0.f;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int c = lane + 64 * i;
            xv[i] = c < E ? (xv[i] - mean) * rstd : 0.f;          // xhat
            gv[i] = c < E ? dv[i] * w[c] : 0.f;
            s1 += gv[i];
            s2 += gv[i] * xv[i];
        }
        const float m1 = wave_sum(s1) * inv, m2 = wave_sum(s2) * inv;
#pragma unroll
        for (int i = 0; i < 12; ++i) {
            const int c = lane + 64 * i;
            if (c < E) {
                float d = rstd * (gv[i] - m1 - xv[i] * m2);
                if (add) d += add[base + c];
                dx_out[base + c] = d;
                if (dx16) dx16[base + c] = static_cast<bf16_t>(d);      // the shadow the next dX product reads
                pg[i] += dv[i] * xv[i];
                pb[i] += dv[i];
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 12; ++i) {
        const int c = lane + 64 * i;
        if (c < E) { red[wave][0][c] = pg[i]; red[wave][1][c] = pb[i]; }
    }
    __syncthreads();
    float* out = partial + (size_t)blockIdx.x * 2 * E;
    for (int c = threadIdx.x; c < 2 * E; c += 256) {
        const int which = c >= E, cc = which ? c - E : c;
        out[c] = ((red[0][which][cc] + red[1][which][cc]) + red[2][which][cc]) + red[3][which][cc];
    }
}

// exact-erf GELU and its derivative (F.gelu default; modules.py:43,77)
static __global__ __launch_bounds__(256)
void gelu_fwd_kernel(const float* __restrict__ pre, float* __restrict__ act, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;      // four elements per thread (16-byte accesses); the tail one by one
    if (i + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(pre + i);
        *reinterpret_cast<float4*>(act + i) = make_float4(gelu_erf(v.x), gelu_erf(v.y), gelu_erf(v.z), gelu_erf(v.w));
    } else {
        for (size_t j = i; j < n; ++j) act[j] = gelu_erf(pre[j]);
    }
}
static __global__ __launch_bounds__(256)
void gelu_bwd_kernel(const float* __restrict__ pre, const float* __restrict__ dact, float* __restrict__ dpre, size_t n) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 4 <= n) {
        const float4 v = *reinterpret_cast<const float4*>(pre + i), d = *reinterpret_cast<const float4*>(dact + i);
        *reinterpret_cast<float4*>(dpre + i) = make_float4(d.x * gelu_grad(v.x), d.y * gelu_grad(v.y), d.z * gelu_grad(v.z), d.w * gelu_grad(v.w));
    } else {
        for (size_t j = i; j < n; ++j) dpre[j] = dact[j] * gelu_grad(pre[j]);
    }
}

// dst[i] = src[i] over a table of pieces, one workgroup per piece (parseq_model_get_params: the master weights back into the caller's tensors)
struct CopyPiece { const float* src; float* dst; int n; };
constexpr int COPY_PIECE_ELEMS = 8192;
static __global__ __launch_bounds__(256)
void copy_pieces_kernel(const CopyPiece* __restrict__ pieces) {
    const CopyPiece c = pieces[blockIdx.x];
    for (int i = threadIdx.x; i < c.n; i += 256) c.dst[i] = c.src[i];
}

// y = a + b (elementwise)
static __global__ __launch_bounds__(256)
void add_kernel(const float* __restrict__ a, const float* __restrict__ b, float* __restrict__ y, size_t n) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) y[i] = a[i] + b[i];
}

// Content stream of the teacher-forced decode (model.py:95-98): row (b, j) = sqrt(E) * emb[tok[b][j]] + (j ? pos_queries[j-1] : 0)
static __global__ __launch_bounds__(256)
void train_content_kernel(const float* __restrict__ emb, const float* __restrict__ posq, const int* __restrict__ tok, int ldt, int L, int E,
                          float scale, float* __restrict__ out) {
    const int row = blockIdx.x, b = row / L, j = row % L;
    const float* e = emb + (size_t)tok[b * ldt + j] * E;
    for (int c = threadIdx.x; c < E; c += 256)
        out[(size_t)row * E + c] = scale * e[c] + (j ? posq[(size_t)(j - 1) * E + c] : 0.f);
}

// d emb[v] += scale * sum over the rows whose token is v, rows visited in ascending order (deterministic; one workgroup per token id).
// The B * L token ids are scanned 256 at a time (one compare per thread, the four waves' ballots through LDS) instead of one after the
// other by the whole workgroup — the first form spent 2.4 ms per step on 9 984 dependent loads; the summation order is unchanged.
// Round 3: the rows are cut into gridDim.y chunks of rows_per (a multiple of 256) rows, workgroup (v, c) writes the unscaled sum of ITS rows
// to partial[v][c][E] and embed_bwd_fold_kernel adds the chunks up in ascending order — <pad> is ~45 % of a batch, and ONE workgroup
// walking its 4 500 rows was 0.58 ms of the step.  partial == nullptr (gridDim.y == 1): the single-stage form, straight into demb.
static __global__ __launch_bounds__(256)
void embed_bwd_kernel(const float* __restrict__ dcontent, const int* __restrict__ tok, int ldt, int B, int L, int E, float scale,
                      float* __restrict__ demb, float* __restrict__ partial, int rows_per) {
    __shared__ unsigned long long hits[4];
    const int v = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = min(B * L, (int)(blockIdx.y + 1) * rows_per);
    float acc[3] = {0.f, 0.f, 0.f};                              // E <= 768
    for (int base = blockIdx.y * rows_per; base < n; base += 256) {
        const int i = base + tid;
        bool hit = false;
        if (i < n) { const int b = i / L, j = i - b * L; hit = tok[b * ldt + j] == v; }
        const unsigned long long m = __ballot(hit);
        if (lane == 0) hits[wave] = m;
        __syncthreads();
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            unsigned long long mm = hits[w];                      // the same in every thread
            // eight hits at a time: their row loads go out back to back (a popular id — <pad> is ~45 % of a batch of short labels — used
            // to pay one full memory round trip per row: 2 ms per step), the additions stay in ascending row order
            while (mm) {
                int bit[8];
                int nb = 0;
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    bit[q] = mm ? __ffsll((long long)mm) - 1 : -1;
                    if (mm) { mm &= mm - 1; ++nb; }
                }
                float rv[8][3];
#pragma unroll
                for (int q = 0; q < 8; ++q) {
                    const float* row = dcontent + (size_t)(base + w * 64 + (bit[q] < 0 ? bit[0] : bit[q])) * E;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const int c = tid + 256 * k;
                        rv[q][k] = c < E ? row[c] : 0.f;
                    }
                }
#pragma unroll
                for (int q = 0; q < 8; ++q)
                    if (q < nb) {
#pragma unroll
                        for (int k = 0; k < 3; ++k) acc[k] += rv[q][k];
                    }
            }
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int c = tid + 256 * k;
        if (c >= E) continue;
        if (partial) partial[((size_t)v * gridDim.y + blockIdx.y) * E + c] = acc[k];
        else demb[(size_t)v * E + c] += scale * acc[k];
    }
}
// d emb[v] += scale * (the chunks of embed_bwd_kernel in ascending order); one workgroup per token id
static __global__ __launch_bounds__(256)
void embed_bwd_fold_kernel(const float* __restrict__ partial, int chunks, int E, float scale, float* __restrict__ demb) {
    const int v = blockIdx.x;
    for (int c = threadIdx.x; c < E; c += 256) {
        float t = 0.f;
        for (int q = 0; q < chunks; ++q) t += partial[((size_t)v * chunks + q) * E + c];
        demb[(size_t)v * E + c] += scale * t;
    }
}

// d(total loss) / d logits, in place: kept rows (softmax - onehot) * inv_total, ignored rows 0.  One wave per row.
static __global__ __launch_bounds__(256)
void ce_bwd_kernel(float* __restrict__ logits, const int* __restrict__ targets, int rows, int C, int ignore_index, float inv_total) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    float* row = logits + (size_t)r * C;
    const int tgt = targets[r];
    if (tgt == ignore_index) {
        for (int c = lane; c < C; c += 64) row[c] = 0.f;
        return;
    }
    float mx = -INFINITY;
    for (int c = lane; c < C; c += 64) mx = fmaxf(mx, row[c]);
    mx = wave_max(mx);
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(row[c] - mx);
    sum = wave_sum(sum);
    const float k = inv_total / sum;
    for (int c = lane; c < C; c += 64) row[c] = expf(row[c] - mx) * k - (c == tgt ? inv_total : 0.f);
}

// loss = sum_k n_k * loss_k / sum_k n_k   (system.py:189-196)
static __global__ void loss_combine_kernel(const float* __restrict__ losses, const int* __restrict__ counts, int K, float* __restrict__ out) {
    if (threadIdx.x || blockIdx.x) return;
    float num = 0.f; int den = 0;
    for (int k = 0; k < K; ++k) { num += losses[k] * (float)counts[k]; den += counts[k]; }
    *out = num / (float)den;
}

// -------------------------------------------------------------------------------------------------------------------
// Dropout (configs/model/parseq.yaml:21, p = 0.1: model.py:99-102 on the embeddings and the queries, modules.py:33-43,70-79
// inside both attentions, after both attention projections, inside and after the MLP).  A mask is never stored: element `idx`
// of site `site` is kept iff hash(seed, site, idx) >= p * 2^32, a counter-based generator (two rounds of a 32-bit integer
// mixer) that the backward kernels re-evaluate and that oracle/decoder_backward.py restates bit for bit.  The stream differs
// from torch's Philox, so training parity with the reference under dropout is statistical; given the same masks it is exact.
// -------------------------------------------------------------------------------------------------------------------
struct DropSpec {
    unsigned seed_lo, seed_hi;
    unsigned thresh;             // keep iff hash >= thresh; 0 = dropout off
    float scale;                 // 1 / (1 - p)
};

__host__ __device__ __forceinline__ unsigned drop_mix(unsigned x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
// multiplier of element idx of site: 0 (dropped) or 1 / (1 - p)
__host__ __device__ __forceinline__ float drop_factor(const DropSpec& d, unsigned site, unsigned long long idx) {
    if (d.thresh == 0u) return 1.0f;
    unsigned h = drop_mix((unsigned)idx ^ d.seed_lo);
    h = drop_mix(h + (unsigned)(idx >> 32) * 0x9e3779b9u + site * 0x85ebca6bu + d.seed_hi);
    return h >= d.thresh ? d.scale : 0.0f;
}

// y[i] = (R ? R[i] : 0) + drop(x[i]) (x == y allowed) and y[m][e] = drop(table[m % L][e]) (element index m * E + e: the decoder queries
// pos_queries[:, :L] expanded over the batch), over `passes` permutation passes laid out one after the other ([passes][n_pass] elements):
// pass p draws site `site + 8 p` on the element index WITHIN the pass — what a launch of its own per pass would draw — so that a step may
// run its K passes as one batch of K * B images without changing a single mask bit.  x_shared: x holds one pass ([n_pass]) that every pass reads.
// grid: (ceil(n_pass / 256), passes)
static __global__ __launch_bounds__(256)
void dropout_passes_kernel(const float* x, int x_shared, const float* R, float* y, size_t n_pass, DropSpec d, unsigned site) {
    const size_t li = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= n_pass) return;
    const size_t i = (size_t)blockIdx.y * n_pass + li;
    const float v = x[x_shared ? li : i] * drop_factor(d, site + 8u * blockIdx.y, li);
    y[i] = R ? R[i] + v : v;
}
static __global__ __launch_bounds__(256)
void dropout_rows_passes_kernel(const float* __restrict__ table, int L, int E, float* __restrict__ y, size_t n_pass, DropSpec d, unsigned site) {
    const size_t li = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= n_pass) return;
    const size_t m = li / E, e = li % E;
    y[(size_t)blockIdx.y * n_pass + li] = table[(m % L) * E + e] * drop_factor(d, site + 8u * blockIdx.y, li);
}
// dpre = drop(dact) * gelu'(pre) over [passes][n_pass] elements (grid (ceil(n_pass / 1024), passes), n_pass % 4 == 0): the dropout inside the MLP
// (site `site + 8 p`, element index within the pass — the mask dropout_passes_kernel drew in the forward) and the GELU backward in one pass
static __global__ __launch_bounds__(256)
void gelu_bwd_drop_passes_kernel(const float* __restrict__ pre, const float* dact, float* dpre, size_t n_pass, DropSpec d, unsigned site) {
    const size_t li = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (li >= n_pass) return;
    const size_t i = (size_t)blockIdx.y * n_pass + li;
    const unsigned st = site + 8u * blockIdx.y;
    const float4 v = *reinterpret_cast<const float4*>(pre + i), g = *reinterpret_cast<const float4*>(dact + i);
    *reinterpret_cast<float4*>(dpre + i) = make_float4(g.x * drop_factor(d, st, li) * gelu_grad(v.x), g.y * drop_factor(d, st, li + 1) * gelu_grad(v.y),
                                                       g.z * drop_factor(d, st, li + 2) * gelu_grad(v.z), g.w * drop_factor(d, st, li + 3) * gelu_grad(v.w));
}
// y[li] (+)= sum over the passes, in ascending order, of drop(x[p][li]) (d.thresh == 0: a plain sum of the passes)
static __global__ __launch_bounds__(256)
void dropout_sum_passes_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n_pass, int passes, DropSpec d, unsigned site, int accumulate) {
    const size_t li = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (li >= n_pass) return;
    float t = accumulate ? y[li] : 0.f;
    for (int p = 0; p < passes; ++p) t += x[(size_t)p * n_pass + li] * drop_factor(d, site + 8u * (unsigned)p, li);
    y[li] = t;
}
// y[i] (+)= sum over the passes of x[p][i], four elements per thread (n_pass a multiple of 4, 16-byte aligned)
static __global__ __launch_bounds__(256)
void sum_passes_kernel(const float* __restrict__ x, float* __restrict__ y, size_t n_pass, int passes, int accumulate) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= n_pass) return;
    float4 t = accumulate ? *reinterpret_cast<const float4*>(y + i) : make_float4(0.f, 0.f, 0.f, 0.f);
    for (int p = 0; p < passes; ++p) {
        const float4 v = *reinterpret_cast<const float4*>(x + (size_t)p * n_pass + i);
        t.x += v.x; t.y += v.y; t.z += v.z; t.w += v.w;
    }
    *reinterpret_cast<float4*>(y + i) = t;
}

// im2col of the patch embedding: row (b, gy, gx), column (c, ky, kx) = img[b][c][gy * ph + ky][gx * pw + kx]   (fp32)
static __global__ __launch_bounds__(256)
void patches_kernel(const float* __restrict__ img, int H, int W, int ph, int pw, float* __restrict__ out) {
    const int gw = W / pw, gh = H / ph, pk = 3 * ph * pw;
    const int row = blockIdx.x, b = row / (gh * gw), gy = (row / gw) % gh, gx = row % gw;
    for (int col = threadIdx.x; col < pk; col += 256) {
        const int c = col / (ph * pw), ky = (col / pw) % ph, kx = col % pw;
        out[(size_t)row * pk + col] = img[(((size_t)b * 3 + c) * H + gy * ph + ky) * W + gx * pw + kx];
    }
}

// The same im2col from raw uint8 pixels (parseq_train_encoder_forward_ex, PARSEQ_U8): out = norm[img byte], norm the 256 values of
// ToTensor + Normalize(0.5, 0.5) (strhub/data/module.py:78-81).  `table` != nullptr: the caller's 256 floats (the Python side builds them
// with the very torch expression its float path uses, so the switch changes no bit whatever way torch rounds it); nullptr: the IEEE
// expression of the inference loaders (gemm.h norm_u8).  One thread per patch-row SEGMENT (row, c, ky): its PW bytes are contiguous in the
// image and its PW floats contiguous in the row, so a lane makes one 8- / 16-byte load and PW / 4 16-byte stores, and consecutive lanes
// write consecutive segments — there is no column loop to outgrow 256 columns (patch16-224: 48 segments of 16).  PW == 0: any patch width,
// byte by byte.  The image base must be PW-aligned (W is a multiple of pw, so every segment then is).
template <int PW>
static __global__ __launch_bounds__(256)
void patches_u8_kernel(const uint8_t* __restrict__ img, const float* __restrict__ table, int H, int W, int ph, int pw, size_t segments,
                       float* __restrict__ out) {
    __shared__ float norm[256];
    norm[threadIdx.x] = table ? table[threadIdx.x] : ((float)threadIdx.x / 255.0f - 0.5f) / 0.5f;
    __syncthreads();
    const size_t seg = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (seg >= segments) return;
    const int gw = W / pw, gh = H / ph, per_row = 3 * ph;
    const size_t row = seg / per_row;
    const int within = (int)(seg - row * per_row), c = within / ph, ky = within - c * ph;
    const size_t b = row / ((size_t)gh * gw);
    const int gy = (int)((row / gw) % gh), gx = (int)(row % gw);
    const uint8_t* src = img + ((b * 3 + c) * H + (size_t)gy * ph + ky) * W + (size_t)gx * pw;
    float* dst = out + seg * pw;                                  // row * pk + (c * ph + ky) * pw
    if constexpr (PW == 8 || PW == 16) {
        unsigned wds[PW / 4];
        if constexpr (PW == 8) { const uint2 v = *reinterpret_cast<const uint2*>(src); wds[0] = v.x; wds[1] = v.y; }
        else { const uint4 v = *reinterpret_cast<const uint4*>(src); wds[0] = v.x; wds[1] = v.y; wds[2] = v.z; wds[3] = v.w; }
#pragma unroll
        for (int q = 0; q < PW / 4; ++q)
            *reinterpret_cast<float4*>(dst + 4 * q) = make_float4(norm[wds[q] & 255u], norm[(wds[q] >> 8) & 255u], norm[(wds[q] >> 16) & 255u], norm[wds[q] >> 24]);
    } else {
        for (int kx = 0; kx < pw; ++kx) dst[kx] = norm[src[kx]];
    }
}

// Stochastic weight averaging over the flat master weights (torch.optim.swa_utils.AveragedModel's default rule): n == 0: avg = w, else
// avg += (w - avg) / (n + 1) — a subtraction, an IEEE division and an addition per element, nothing to contract.  Grid-stride over
// 16-byte pieces when both pointers allow it, the tail (and an unaligned pair) one by one; every element has one owner: deterministic.
constexpr int AVERAGE_BLOCKS = 1024;
static __global__ __launch_bounds__(256)
void weights_average_kernel(const float* __restrict__ w, float* __restrict__ avg, size_t n, int first, float count, int vec) {
    const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, threads = (size_t)gridDim.x * 256;
    const size_t n4 = vec ? n / 4 : 0;
    for (size_t i = tid; i < n4; i += threads) {
        const float4 x = reinterpret_cast<const float4*>(w)[i];
        if (first) { reinterpret_cast<float4*>(avg)[i] = x; continue; }
        float4 a = reinterpret_cast<const float4*>(avg)[i];
        a.x = a.x + (x.x - a.x) / count; a.y = a.y + (x.y - a.y) / count; a.z = a.z + (x.z - a.z) / count; a.w = a.w + (x.w - a.w) / count;
        reinterpret_cast<float4*>(avg)[i] = a;
    }
    for (size_t i = n4 * 4 + tid; i < n; i += threads) avg[i] = first ? w[i] : avg[i] + (w[i] - avg[i]) / count;
}

// -------------------------------------------------------------------------------------------------------------------
// optimiser step over the flat parameter / gradient buffers (timm create_optimizer_v2('adamw') = torch.optim.AdamW;
// gradient clipping = torch.nn.utils.clip_grad_norm_, what Lightning's gradient_clip_val applies; configs/main.yaml:39)
// -------------------------------------------------------------------------------------------------------------------
constexpr int SUMSQ_BLOCKS = 1024;

// partial[block] = sum of g[i]^2 over the block's grid-stride slice (fixed order: deterministic)
static __global__ __launch_bounds__(256)
void sumsq_partial_kernel(const float* __restrict__ g, size_t n, float* __restrict__ partial) {
    __shared__ float red[256];
    float s = 0.f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)SUMSQ_BLOCKS * 256) s = fmaf(g[i], g[i], s);
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) partial[blockIdx.x] = red[0];
}
static __global__ __launch_bounds__(256)
void sumsq_final_kernel(const float* __restrict__ partial, float* __restrict__ norm_out) {
    __shared__ float red[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < SUMSQ_BLOCKS; i += 256) s += partial[i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) *norm_out = sqrtf(red[0]);
}

// torch.optim.AdamW (single-tensor path), with the clip coefficient min(1, max_norm / (norm + 1e-6)) applied to the gradient
// on the fly when `norm` is given:   p *= 1 - lr wd;  m = lerp(m, g, 1 - b1);  v = b2 v + (1 - b2) g^2;
//                                    p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
static __global__ __launch_bounds__(256)
void adamw_kernel(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v, size_t n, float lr,
                  float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2_sqrt, const float* __restrict__ norm, float max_norm) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float coef = 1.f;
    if (norm) coef = fminf(max_norm / (*norm + 1e-6f), 1.0f);
    const float grad = g[i] * coef;
    float param = p[i] * (1.0f - lr * weight_decay);
    const float mi = m[i] + (grad - m[i]) * (1.0f - beta1);
    const float vi = v[i] * beta2 + (1.0f - beta2) * grad * grad;
    const float denom = sqrtf(vi) / bc2_sqrt + eps;
    param -= (lr / bc1) * (mi / denom);
    p[i] = param; m[i] = mi; v[i] = vi;
}

}  // namespace pq
