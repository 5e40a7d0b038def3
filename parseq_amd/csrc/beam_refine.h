// Cloze refinement of the beams of a finished search.  The decoder pass itself is forward's refinement run on every
// beam row; what lives here is the selection after it, split in two: a row-statistics kernel over all B * W * L logit rows (a wave each),
// and a per-image kernel that cuts the refined readings at <eos>, sums the scores, removes duplicates, ranks the W rows and re-parents
// every field of the beam state in place.
#pragma once
#include "beam.h"

namespace pq {

constexpr int BEAM_REFINE_SCORE = 1;      // PARSEQ_BEAM_REFINE_SCORE: rescore the hypotheses as they are
constexpr int BEAM_REFINE_EDIT = 2;       // PARSEQ_BEAM_REFINE_EDIT: replace every hypothesis by the arg-max reading of its refinement
constexpr int BEAM_REFINE_MAX_L = 64;     // positions of a reading: a lane each

// dynamic LDS of beam_refine_select_kernel: the image's W history rows
static inline size_t beam_refine_lds(int W, int ldt) { return (size_t)W * ldt * sizeof(int); }

// Token i of beam row r: position i + 1 of its history, or the last pick where the row has no such position (i + 1 == ldt).
__device__ __forceinline__ int beam_token(const int* __restrict__ tok, int ldt, const int* __restrict__ picked, size_t r, int i) {
    return i + 1 < ldt ? tok[r * ldt + i + 1] : picked[r];
}

// One wave per (row, position) of the refinement logits [rows][L][C].  With lp = log_softmax(logits[r][i]) as beam_step_kernel computes it
// ((x - max) - logf(sum expf(x - max)), the lane-strided partial sums combined by wave_sum):
//   lp_tok[r][i] = lp[t[i]] for the row's own token (-inf where that is no class: pad_id in a slot past the <eos>)
//   amax[r][i]   = the arg-max class under argmax_take's rule,   lp_max[r][i] = its lp
static __global__ __launch_bounds__(256)
void beam_refine_stats_kernel(const float* __restrict__ logits, int rows, int L, int C, const int* __restrict__ tok, int ldt,
                              const int* __restrict__ picked, float* __restrict__ lp_tok, int* __restrict__ amax, float* __restrict__ lp_max) {
    const int lane = threadIdx.x & 63;
    const size_t idx = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (idx >= (size_t)rows * L) return;
    const size_t r = idx / (size_t)L;
    const int i = (int)(idx - r * L);
    const float* row = logits + idx * (size_t)C;
    float m = -INFINITY, best = -INFINITY; int bi = ARGMAX_NONE;
    for (int c = lane; c < C; c += 64) {
        const float v = row[c];
        m = fmaxf(m, v);
        if (argmax_take(v, c, best, bi)) { best = v; bi = c; }
    }
    m = wave_max(m);
    wave_argmax(best, bi);
    bi = argmax_final(bi, C);
    float sum = 0.f;
    for (int c = lane; c < C; c += 64) sum += expf(row[c] - m);
    const float lg = logf(wave_sum(sum));
    if (lane == 0) {
        const int t = beam_token(tok, ldt, picked, r, i);
        lp_tok[idx] = (t >= 0 && t < C) ? (row[t] - m) - lg : -INFINITY;
        amax[idx] = bi;
        lp_max[idx] = (row[bi] - m) - lg;
    }
}

// One image per workgroup, after beam_refine_stats_kernel; the W beams in place.  A row whose score is -inf is dead and stays dead.
//   score mode: new score = sum_{i <= last} lp_tok[i], last = length for a finished row, L - 1 otherwise; everything else is kept.
//   edit mode:  t'[i] = amax[i] up to and including the first <eos>, pad_id after it; length' = its index (L without one), finished' = there
//               is one; new score = sum_{i <= last'} lp_max[i].  Of live rows with the same new reading the one with the higher new score
//               stays (then the lower row), the others become dead.
// fp32 sums in ascending i.  A sum that is not a number (a summed position's logits hold a NaN or a +inf, or nothing but -inf) is -inf: the
// row becomes dead, so no NaN enters the ranking below.  Then the rows are ranked on (beam_ordered(new score), ~row): higher score first, then the lower row, dead rows
// last in their order, and every field moves with its row: history, picked, length, finished, node, word (either may be null) and ar_score.
// A dead row comes out as score -inf, length 0, finished 0, word -1, pad_id in picked and in every history slot after <bos>.
// Everything is loaded into LDS before the first barrier and written after the last (the race of section 18).
static __global__ __launch_bounds__(BEAM_THREADS)
void beam_refine_select_kernel(int mode, int W, int L, const float* __restrict__ lp_tok, const int* __restrict__ amax,
                               const float* __restrict__ lp_max, int* __restrict__ tok, int ldt, float* __restrict__ score,
                               unsigned char* __restrict__ finished, int* __restrict__ length, int* __restrict__ picked, int* __restrict__ node,
                               int* __restrict__ word, float* __restrict__ ar_score, int eos_id, int pad_id) {
    extern __shared__ int refine_hist[];      // [W][ldt]
    __shared__ float s_lp[BEAM_MAX_W][BEAM_REFINE_MAX_L];
    __shared__ float s_old[BEAM_MAX_W], s_new[BEAM_MAX_W], s_ar[BEAM_MAX_W];
    __shared__ int s_len[BEAM_MAX_W], s_picked[BEAM_MAX_W], s_node[BEAM_MAX_W], s_word[BEAM_MAX_W], s_last[BEAM_MAX_W], s_src[BEAM_MAX_W];
    __shared__ unsigned char s_fin[BEAM_MAX_W], s_kill[BEAM_MAX_W];
    int* hist = refine_hist;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row0 = (size_t)blockIdx.x * W;
    if (tid < W) {
        s_old[tid] = score[row0 + tid]; s_fin[tid] = finished[row0 + tid]; s_len[tid] = length[row0 + tid]; s_picked[tid] = picked[row0 + tid];
        s_node[tid] = node ? node[row0 + tid] : -1; s_word[tid] = word ? word[row0 + tid] : -1; s_ar[tid] = ar_score[row0 + tid];
        s_kill[tid] = 0;
    }
    for (int i = tid; i < W * ldt; i += BEAM_THREADS) hist[i] = tok[row0 * ldt + i];
    __syncthreads();

    // a wave per row, a lane per position: the terms of the sum, and in edit mode the new reading into the row's own history
    for (int w = wave; w < W; w += BEAM_THREADS / 64) {
        const size_t r = row0 + w;
        const bool alive = s_old[w] > -INFINITY;
        if (mode == BEAM_REFINE_EDIT) {
            const int a = lane < L ? amax[r * L + lane] : -1;
            const unsigned long long eos_lanes = __ballot(lane < L && a == eos_id);
            const int e = eos_lanes ? (int)__builtin_ctzll(eos_lanes) : L;
            if (alive && lane < L) {
                s_lp[w][lane] = lp_max[r * L + lane];
                const int t = lane <= e ? a : pad_id;
                if (lane + 1 < ldt) hist[w * ldt + lane + 1] = t;
                if (lane == L - 1) s_picked[w] = t;
            }
            if (alive && lane == 0) { s_len[w] = e; s_fin[w] = e < L ? 1 : 0; s_last[w] = e < L ? e : L - 1; }
        } else {
            if (alive && lane < L) s_lp[w][lane] = lp_tok[r * L + lane];
            if (alive && lane == 0) { const int last = s_fin[w] ? s_len[w] : L - 1; s_last[w] = last < 0 ? 0 : (last > L - 1 ? L - 1 : last); }
        }
    }
    __syncthreads();
    if (tid < W) {
        float s = -INFINITY;
        if (s_old[tid] > -INFINITY) {
            s = 0.f;
            const int last = s_last[tid];
            for (int i = 0; i <= last; ++i) s += s_lp[tid][i];
            if (s == 0.f) s = 0.f;      // one zero: the ordering below is on the bits
            if (s != s) s = -INFINITY;  // a summed position whose log-sum is no number (a NaN or +inf logit, a row of -inf): no score, a dead row
        }
        s_new[tid] = s;
    }
    __syncthreads();

    // duplicates (edit mode): thread (w, v) tests whether live row v has row w's reading and beats it
    if (mode == BEAM_REFINE_EDIT && tid < W * W) {
        const int w = tid / W, v = tid - w * W;
        const float sw = s_new[w], sv = s_new[v];
        if (v != w && sw > -INFINITY && sv > -INFINITY && (sv > sw || (sv == sw && v < w))) {
            bool same = s_len[w] == s_len[v] && s_fin[w] == s_fin[v] && (L < ldt || s_picked[w] == s_picked[v]);
            const int n = L < ldt ? L : ldt - 1;
            for (int j = 1; same && j <= n; ++j) same = hist[w * ldt + j] == hist[v * ldt + j];
            if (same) s_kill[w] = 1;
        }
    }
    __syncthreads();
    if (tid < W && s_kill[tid]) s_new[tid] = -INFINITY;
    __syncthreads();
    if (tid < W) {
        const unsigned long long mine = ((unsigned long long)beam_ordered(s_new[tid]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)tid);
        int rank = 0;
        for (int v = 0; v < W; ++v) {
            const unsigned long long k = ((unsigned long long)beam_ordered(s_new[v]) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)v);
            rank += k > mine ? 1 : 0;
        }
        s_src[rank] = tid;
    }
    __syncthreads();

    for (int i = tid; i < W * ldt; i += BEAM_THREADS) {
        const int r = i / ldt, j = i - r * ldt;
        const int src = s_src[r];
        const bool dead = !(s_new[src] > -INFINITY);
        tok[row0 * ldt + i] = (dead && j > 0) ? pad_id : hist[src * ldt + j];
    }
    if (tid < W) {
        const int src = s_src[tid];
        const bool dead = !(s_new[src] > -INFINITY);
        score[row0 + tid] = s_new[src];
        finished[row0 + tid] = dead ? 0 : s_fin[src];
        length[row0 + tid] = dead ? 0 : s_len[src];
        picked[row0 + tid] = dead ? pad_id : s_picked[src];
        if (node) node[row0 + tid] = s_node[src];
        if (word) word[row0 + tid] = dead ? -1 : s_word[src];
        ar_score[row0 + tid] = s_ar[src];
    }
}

}  // namespace pq
