// Scoring of given readings: rows b N .. b N + N - 1 of a batch are the candidates of crop b, every row attends to
// its crop's memory, and per decoding order one teacher-forced decoder pass leaves logits [rows][L][C].  Three kernels live here: the
// staging of the candidates into the plan's token rows, the per-row log-probabilities of one order, and the per-crop combination and rank.
#pragma once
#include "common.h"

namespace pq {

constexpr int SCORE_MAX_N = 16;           // PARSEQ_SCORE_MAX_CANDIDATES: candidates of a crop, a thread each in score_rank_kernel
constexpr int SCORE_MAX_ORDERS = 16;      // PARSEQ_SCORE_MAX_ORDERS
constexpr int SCORE_MAX_L = 64;           // positions of a candidate: a lane each in score_seed_kernel
constexpr int SCORE_MEAN = 1;             // PARSEQ_SCORE_MEAN (0: PARSEQ_SCORE_MIX)
constexpr int SCORE_LENGTH_NORM = 2;      // PARSEQ_SCORE_LENGTH_NORM

// One wave per row, a lane per position.  cand [rows][L]: c_0 .. c_{n-1}, <eos>, then <pad>; a first entry of <pad> is an absent row.
// A row is valid when its first <eos> is at n < L, every entry before it is a class in [0, C) and every entry after it is <pad>.
//   tok [rows][ldt]     <bos>, c_0 .. c_{n-1}, <pad> ... up to ldt entries; an absent or invalid row is <bos>, <pad> ... — no id outside
//                       the embedding table ever reaches the decoder
//   kpm [rows][ldk]     1 where tok is <pad> (tok holds no <eos>: the slot of the <eos> input is <pad>, which is key-padded all the same)
//   target [rows][L]    cand[i] for i <= n of a valid row, -1 elsewhere
//   length, valid [rows]    n and 1, or 0 and 0
static __global__ __launch_bounds__(256)
void score_seed_kernel(const int* __restrict__ cand, int rows, int L, int C, int bos_id, int eos_id, int pad_id, int* __restrict__ tok, int ldt,
                       unsigned char* __restrict__ kpm, int ldk, int* __restrict__ target, int* __restrict__ length, unsigned char* __restrict__ valid) {
    const int lane = threadIdx.x & 63;
    const size_t r = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= (size_t)rows) return;      // wave-uniform
    const int* row = cand + r * L;
    const int t = lane < L ? row[lane] : pad_id;
    const unsigned long long eos_lanes = __ballot(lane < L && t == eos_id);
    const int n = eos_lanes ? (int)__builtin_ctzll(eos_lanes) : -1;
    const bool bad = lane < L && (lane < n ? (t < 0 || t >= C) : (lane > n && t != pad_id));
    const bool ok = row[0] != pad_id && n >= 0 && __ballot(bad) == 0ull;
    if (lane < ldt) {
        const bool ch = ok && lane >= 1 && lane - 1 < n;      // lane - 1 < n < L: inside the row
        tok[r * ldt + lane] = lane == 0 ? bos_id : (ch ? row[lane - 1] : pad_id);
        if (lane < ldk) kpm[r * ldk + lane] = (lane == 0 || ch) ? 0 : 1;
    }
    if (lane < L) target[r * L + lane] = (ok && lane <= n) ? t : -1;
    if (lane == 0) { length[r] = ok ? n : 0; valid[r] = ok ? 1 : 0; }
}

// One workgroup per row, its four waves one position each in turn, over the logits [rows][L][C] of order k of K.  With
// lp = log_softmax(logits[r][i]) exactly as beam_refine_stats_kernel / beam_step_kernel compute it ((x - max) - logf(sum expf(x - max)), lane
// c % 64 adding classes c, c + 64, .. in that order, the partial sums combined by wave_sum — dword loads a wave coalesces into 256-byte
// runs; a wider load per lane would move classes between lanes and with them the bits):
//   char_lp [rows][K][L] (may be null)   lp[target[r][i]] for i <= length[r] of a valid row (-inf where the target is no class), 0 elsewhere
//   order_score [rows][K]                their fp32 sum from 0 in ascending i, as beam_refine_select_kernel adds; a sum that is not a number is
//                                        -inf; -inf for a row that is not valid
// Every output has one writer: no atomics, the same bits on any stream.
static __global__ __launch_bounds__(256)
void score_rows_kernel(const float* __restrict__ logits, int L, int C, const int* __restrict__ target, const int* __restrict__ length,
                       const unsigned char* __restrict__ valid, int K, int k, float* __restrict__ order_score, float* __restrict__ char_lp) {
    __shared__ float s_lp[SCORE_MAX_L];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t r = blockIdx.x;
    const bool live = valid[r] != 0;
    const int n = live ? min(max(length[r], 0), L - 1) : -1;      // block-uniform
    for (int i = wave; i <= n; i += 4) {
        const float* row = logits + (r * L + i) * (size_t)C;
        float m = -INFINITY;
        for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
        m = wave_max(m);
        float sum = 0.f;
        for (int c = lane; c < C; c += 64) sum += expf(row[c] - m);
        const float lg = logf(wave_sum(sum));
        if (lane == 0) {
            const int t = target[r * L + i];
            s_lp[i] = (t >= 0 && t < C) ? (row[t] - m) - lg : -INFINITY;
        }
    }
    __syncthreads();
    if (char_lp && tid < L) char_lp[(r * K + k) * L + tid] = tid <= n ? s_lp[tid] : 0.f;
    if (tid == 0) {
        float s = -INFINITY;
        if (live) {
            s = 0.f;
            for (int i = 0; i <= n; ++i) s += s_lp[i];
            if (s == 0.f) s = 0.f;
            if (s != s) s = -INFINITY;
        }
        order_score[r * K + k] = s;
    }
}

// One workgroup (a wave) per crop, thread j its candidate j < N.  From order_score [B N][K], in fp64 with k ascending (NaN read as -inf):
//   mix:  m = max_k s_k;  combined = m + log(sum_k exp(s_k - m)) - log(K)   (-inf when m is; K = 1: m + 0 - 0, the single order's bits)
//   mean: combined = (sum_k s_k) / K
// score [B][N] = (float)combined, -inf for a row that is not valid or whose combination is not a number.  The key is (double)score, under
// SCORE_LENGTH_NORM divided by (length + 1).  rank [B][N]: the candidates best first — higher key, then the lower index — so rows of
// score -inf come last in index order and every rank row is a permutation of 0 .. N-1.
static __global__ __launch_bounds__(64)
void score_rank_kernel(const float* __restrict__ order_score, const int* __restrict__ length, const unsigned char* __restrict__ valid, int N, int K,
                       int flags, float* __restrict__ score, int* __restrict__ rank) {
    __shared__ double s_key[SCORE_MAX_N];
    const int j = threadIdx.x;
    const size_t r = (size_t)blockIdx.x * N + j;
    if (j < N) {
        double c = -INFINITY;
        if (valid[r]) {
            const float* s = order_score + r * K;
            if (flags & SCORE_MEAN) {
                double acc = 0.0;
                for (int k = 0; k < K; ++k) { const double v = (double)s[k]; acc += v != v ? -INFINITY : v; }
                c = acc / (double)K;
            } else {
                double m = -INFINITY;
                for (int k = 0; k < K; ++k) { const double v = (double)s[k]; if (v > m) m = v; }      // a NaN never compares greater
                if (m > -INFINITY) {
                    double acc = 0.0;
                    for (int k = 0; k < K; ++k) { const double v = (double)s[k]; acc += v != v ? 0.0 : exp(v - m); }
                    c = m + log(acc) - log((double)K);
                }
            }
        }
        float f = (float)c;
        if (f != f) f = -INFINITY;
        score[r] = f;
        double key = (double)f;
        if ((flags & SCORE_LENGTH_NORM) && f > -INFINITY) key /= (double)(max(length[r], 0) + 1);
        s_key[j] = key;
    }
    __syncthreads();
    if (j < N) {
        const double mine = s_key[j];
        int ahead = 0;
        for (int v = 0; v < N; ++v) ahead += (s_key[v] > mine || (s_key[v] == mine && v < j)) ? 1 : 0;
        rank[(size_t)blockIdx.x * N + ahead] = j;
    }
}

}  // namespace pq
