// Long text lines: a line is read as K <= 64 overlapping windows, every window a row of an ordinary batch, and this
// kernel stitches the rows' characters into one reading by position.  One workgroup per line; a window owns 32 consecutive lanes (L <= 32),
// so a wave carries two windows and one ballot gives both their masks.  Everything that decides is fp64 with separately rounded products
// and sums (no contraction), comparisons only, and every thread writes words of its own: the result depends on neither grid nor stream.
#pragma once
#include "common.h"

namespace pq {

constexpr int LINE_MAX_WINDOWS = 64;
constexpr int LINE_MAX_L = 32;
constexpr int LINE_MAX_OUT = 2048;         // = LINE_MAX_WINDOWS * LINE_MAX_L: more cannot survive
constexpr int LINE_THREADS = 256;          // 8 windows per pass

struct LineStitchArgs {
    const int* tokens; const int* lengths; const float* probs; const float* centres; const float* boxes;      // [rows][L], [rows], [rows][L], [rows][L][2], [rows][L][4]
    int rows, L, C;
    const int* win;                        // [rows][3]: x0, ww, h
    int img_h, img_w;
    const int* line_first;                 // [lines + 1]
    const double* min_sep;                 // [lines]
    int max_out;
    int* len_out; int* tokens_out; float* probs_out; float* boxes_out; double* x_out; int* src_out; float* confidence_out;
};

// source coordinate of a model-input coordinate v: origin + v * scale, the product and the sum rounded one after the other
static __device__ __forceinline__ double line_map(double origin, float v, double scale) { return __dadd_rn(origin, __dmul_rn((double)v, scale)); }

static __global__ __launch_bounds__(LINE_THREADS)
void line_stitch_kernel(const LineStitchArgs a) {
    __shared__ double sX[LINE_MAX_WINDOWS][LINE_MAX_L];          // 16 KiB: every candidate's centre in source pixels
    __shared__ double sq[LINE_MAX_WINDOWS];                      // a window's product of surviving probabilities
    __shared__ double scut[LINE_MAX_WINDOWS];                    // cut k, between windows k and k + 1
    __shared__ int stok[LINE_MAX_WINDOWS][LINE_MAX_L];           // 8 KiB
    __shared__ float sp[LINE_MAX_WINDOWS][LINE_MAX_L];           // 8 KiB
    __shared__ int sx0[LINE_MAX_WINDOWS], sww[LINE_MAX_WINDOWS], sh[LINE_MAX_WINDOWS], slen[LINE_MAX_WINDOWS];
    __shared__ unsigned own[LINE_MAX_WINDOWS], drop_a[LINE_MAX_WINDOWS], drop_b[LINE_MAX_WINDOWS];      // bit i = position i
    __shared__ int soff[LINE_MAX_WINDOWS + 1];

    const int l = blockIdx.x, t = threadIdx.x, L = a.L;
    // the line's rows, every index kept inside [0, rows) whatever the table holds
    long long r0 = a.line_first[l], r1 = a.line_first[l + 1];
    r0 = r0 < 0 ? 0 : (r0 > a.rows ? a.rows : r0);
    long long kk = r1 - r0;
    kk = kk < 0 ? 0 : (kk > LINE_MAX_WINDOWS ? LINE_MAX_WINDOWS : kk);
    if (kk > a.rows - r0) kk = a.rows - r0;
    const int K = (int)kk;
    const size_t row0 = (size_t)r0;
    const double sep = a.min_sep[l], delta = sep * 0.5;

    if (t < LINE_MAX_WINDOWS) {
        drop_a[t] = 0; drop_b[t] = 0; own[t] = 0;
        if (t < K) {
            const int* w = a.win + (row0 + t) * 3;
            sx0[t] = w[0]; sww[t] = w[1]; sh[t] = w[2];
            const int n = a.lengths[row0 + t];
            slen[t] = n < 0 ? 0 : (n > L ? L : n);
        }
    }
    __syncthreads();
    if (t + 1 < K) scut[t] = ((double)sx0[t + 1] + (double)((long long)sx0[t] + (long long)sww[t])) * 0.5;
    __syncthreads();

    // 1, 2: candidates and ownership — window k on lanes 32 (k & 1) .. of wave (k >> 1) & 3, pass k >> 3
    const int i = t & 31;
    for (int k = t >> 5; k < ((K + 7) & ~7); k += LINE_THREADS / 32) {
        bool keep = false;
        if (k < K && i < L) {
            const size_t e = (row0 + k) * L + i;
            const int tok = a.tokens[e];
            const double X = line_map((double)sx0[k], a.centres[e * 2], (double)sww[k] / (double)a.img_w);
            stok[k][i] = tok; sp[k][i] = a.probs[e]; sX[k][i] = X;
            const bool cand = i < slen[k] && tok >= 0 && tok < a.C;
            const double lo = k == 0 ? -INFINITY : scut[k - 1] - delta, hi = k == K - 1 ? INFINITY : scut[k] + delta;
            keep = cand && lo <= X && X < hi;      // a NaN fails both, +inf fails the second even at the open end
        }
        const unsigned long long m = __ballot(keep);
        if (k < K && i == 0) own[k] = (unsigned)(m >> ((t & 32) ? 32 : 0));
    }
    __syncthreads();

    // 3: a lane per seam (k, k + 1), on the lists ownership left; it alone writes drop_a[k] and drop_b[k + 1]
    if (t + 1 < K && sep > 0.0) {
        const int k = t;
        const unsigned left = own[k];
        unsigned matched = 0, da = 0, db = 0;
        for (unsigned mb = own[k + 1]; mb; mb &= mb - 1) {
            const int b = __builtin_ctz(mb);
            const int tb = stok[k + 1][b];
            const double xb = sX[k + 1][b];
            int best = -1; double bd = 0.0;
            for (unsigned ma = left & ~matched; ma; ma &= ma - 1) {
                const int c = __builtin_ctz(ma);
                if (stok[k][c] != tb) continue;
                const double d = fabs(sX[k][c] - xb);
                if (d < sep && (best < 0 || d < bd)) { best = c; bd = d; }
            }
            if (best >= 0) {
                matched |= 1u << best;
                if (!(sp[k + 1][b] > sp[k][best])) db |= 1u << b; else da |= 1u << best;
            }
        }
        drop_a[k] = da; drop_b[k + 1] = db;
    }
    __syncthreads();

    // survivors, their counts, the exclusive scan of the counts (wave 0) and every window's product in position order
    if (t < LINE_MAX_WINDOWS) {
        const unsigned s = t < K ? own[t] & ~drop_a[t] & ~drop_b[t] : 0u;
        int inc = __builtin_popcount(s);
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int v = __shfl_up(inc, o, 64);
            if (t >= o) inc += v;
        }
        soff[t + 1] = inc;
        if (t == 0) soff[0] = 0;
        own[t] = s;                              // from here on: the survivors
        double q = 1.0;
        for (unsigned m = s; m; m &= m - 1) q *= (double)sp[t][__builtin_ctz(m)];
        sq[t] = q;
    }
    __syncthreads();
    const int total = soff[K];
    if (t == 0) {
        double c = 1.0;
        for (int k = 0; k < K; ++k) c *= sq[k];
        double pe = 1.0;
        if (K > 0 && slen[K - 1] < L) pe = (double)sp[K - 1][slen[K - 1]];
        a.confidence_out[l] = (float)(c * pe);
        a.len_out[l] = total;
    }

    // 4, 6: compacted stores in (window, position) order, then the padding
    const size_t out0 = (size_t)l * a.max_out;
    for (int k = t >> 5; k < K; k += LINE_THREADS / 32) {
        const unsigned s = own[k];
        if (i < L && (s >> i & 1u)) {
            const int r = soff[k] + __builtin_popcount(s & ((1u << i) - 1u));
            if (r < a.max_out) {
                const size_t o = out0 + r, e = (row0 + k) * L + i;
                const double sx = (double)sww[k] / (double)a.img_w, sy = (double)sh[k] / (double)a.img_h, ox = (double)sx0[k];
                a.tokens_out[o] = stok[k][i];
                a.probs_out[o] = sp[k][i];
                a.x_out[o] = sX[k][i];
                a.src_out[o * 2] = k; a.src_out[o * 2 + 1] = i;
                const float* bx = a.boxes + e * 4;
                a.boxes_out[o * 4] = (float)line_map(ox, bx[0], sx);
                a.boxes_out[o * 4 + 1] = (float)line_map(0.0, bx[1], sy);
                a.boxes_out[o * 4 + 2] = (float)line_map(ox, bx[2], sx);
                a.boxes_out[o * 4 + 3] = (float)line_map(0.0, bx[3], sy);
            }
        }
    }
    for (int r = total + t; r < a.max_out; r += LINE_THREADS) {
        const size_t o = out0 + r;
        a.tokens_out[o] = -1; a.probs_out[o] = 0.f; a.x_out[o] = 0.0;
        a.src_out[o * 2] = -1; a.src_out[o * 2 + 1] = -1;
        a.boxes_out[o * 4] = 0.f; a.boxes_out[o * 4 + 1] = 0.f; a.boxes_out[o * 4 + 2] = 0.f; a.boxes_out[o * 4 + 3] = 0.f;
    }
}

}  // namespace pq
