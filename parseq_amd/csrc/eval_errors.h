// Error analysis on the device: for every sample the canonical edit script between the adapted prediction and
// the label, and integer tables of what went wrong — operation totals, accuracy by label length, errors by position, a confusion
// matrix over the test charset's symbols.  The front of a row is eval_row_front (eval_metrics.h), so the strings compared ARE the ones
// eval_rows_kernel compares; the recurrence is the same call, eval_wave_distance, in its mode that keeps every column.
#pragma once

#include "eval_metrics.h"

namespace pq {

constexpr int EVAL_MAX_SYMBOLS = 512;                                  // T: distinct code points a prediction can consist of
constexpr int EVAL_SCRIPT_WIDTH = EVAL_MAX_GT + EVAL_MAX_PRED;        // codes of one script: every step consumes a character
constexpr int EVAL_LEN_BINS = 33;                                      // by_length / by_position rows: 0 .. 31, then "32 and more"
constexpr int EVAL_ERR_HEAD = 8;                                       // int64 words: samples, matches, substitutions, insertions, deletions, exact, 0, 0
constexpr int EVAL_ERR_BY_LENGTH = EVAL_ERR_HEAD;                      // [33][4]: samples, exact, distance, label characters
constexpr int EVAL_ERR_BY_POSITION = EVAL_ERR_BY_LENGTH + EVAL_LEN_BINS * 4;      // [33][4]: label characters, substitutions, deletions, insertions
constexpr int EVAL_ERR_CONFUSION = EVAL_ERR_BY_POSITION + EVAL_LEN_BINS * 4;      // [T + 2][T + 2]: row = label symbol, column = predicted symbol
enum : int { EVAL_OP_MATCH = 0, EVAL_OP_SUBSTITUTION = 1, EVAL_OP_INSERTION = 2, EVAL_OP_DELETION = 3 };

static inline size_t eval_errors_accum_words(int T) { return (size_t)EVAL_ERR_CONFUSION + (size_t)(T + 2) * (size_t)(T + 2); }

// Index of code point `cp` in the ascending `symbols[0 .. T)`, T ("other") if it is not there.
static __device__ __forceinline__ int eval_symbol_index(const int* __restrict__ symbols, int T, int cp) {
    int lo = 0, hi = T;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (symbols[mid] < cp) lo = mid + 1; else hi = mid;
    }
    return (lo < T && symbols[lo] == cp) ? lo : T;
}

// D[i][j] of the Levenshtein table from the stored column j: bit r of `col.x` / `col.y` says D[r + 1][j] - D[r][j] is +1 / -1, D[0][j] = j.
static __device__ __forceinline__ int eval_table_entry(uint2 col, int i, int j) {
    const unsigned mask = i >= 32 ? 0xffffffffu : ((1u << i) - 1u);
    return j + __popc(col.x & mask) - __popc(col.y & mask);
}

static __device__ __forceinline__ void eval_add64(long long* p, long long v) {
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// One wave per sample, four samples per workgroup; every wave of the workgroup takes every barrier (a wave past the batch idles between them).
//   phase 1  eval_row_front, then eval_wave_distance<true>: the label and the low 32 bits of every column's (Pv, Mv) kept in LDS
//   phase 2  the trace back from (m, n): the first rule of {diagonal, up, left} that explains D[i][j], at most m + n wave-uniform steps
//            on two stored columns each; the operations go to LDS in reverse order as code | prediction index << 2 | position << 8
//   phase 3  lanes write the forward script (coalesced bytes) and add their operations to the tables: the confusion cell straight to
//            global memory (64-bit integer atomics: the cells are spread, and integer adds commute, so totals are bit-identical whatever
//            the order), positions and operation totals to the workgroup's LDS copy first
//   phase 4  the workgroup's position table and totals go to global memory, one atomic per non-zero cell
static __global__ __launch_bounds__(256)
void eval_errors_kernel(const int* __restrict__ ids, const int* __restrict__ lengths, int B, int L, int C, const int* __restrict__ table,
                        const int* __restrict__ symbols, int T, const int* __restrict__ gt, const int* __restrict__ gt_len, int G,
                        signed char* __restrict__ script, int* __restrict__ script_len, int* __restrict__ rows, long long* __restrict__ acc) {
    __shared__ int spred[4][64];
    __shared__ int sgt[4][EVAL_MAX_GT];
    __shared__ uint2 scol[4][EVAL_MAX_GT + 1];
    __shared__ int sops[4][EVAL_SCRIPT_WIDTH];
    __shared__ int stab[EVAL_ERR_HEAD + EVAL_LEN_BINS * 4];             // head, then by_position, of this workgroup
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + w;
    const bool active = b < B;
    if (threadIdx.x < EVAL_ERR_HEAD + EVAL_LEN_BINS * 4) stab[threadIdx.x] = 0;
    const EvalRow r = eval_row_front(ids + (size_t)(active ? b : 0) * L, active ? lengths[b] : 0, L, C, table, active ? gt_len[b] : 0, G, active,
                                     spred[w], lane);                          // holds a barrier: stab is zero after it
    const int m = r.m, n = r.n;

    // ---- phase 1: the recurrence, columns and label kept (an empty prediction: n deletions; the columns are not read then)
    const int dist = active ? eval_wave_distance<true>(r.pc, m, gt + (size_t)b * G, n, lane, scol[w], sgt[w]) : 0;
    __syncthreads();

    // ---- phase 2: the trace back (every lane computes the same steps; lane 0 records them)
    int nops = 0;
    if (active) {
        int i = m, j = n, d = dist;
        while ((i > 0 || j > 0) && nops < EVAL_SCRIPT_WIDTH) {
            int code = EVAL_OP_DELETION, pos = j - 1, pi = 0;
            bool taken = false;
            if (i > 0 && j > 0) {
                const int dd = eval_table_entry(scol[w][j - 1], i - 1, j - 1);
                const int ne = spred[w][i - 1] != sgt[w][j - 1];
                if (dd + ne == d) { code = ne; pi = i - 1; d = dd; taken = true; --i; --j; }
            }
            if (!taken && i > 0) {
                const int du = eval_table_entry(scol[w][j], i - 1, j);
                if (du + 1 == d || j == 0) { code = EVAL_OP_INSERTION; pos = j; pi = i - 1; d = du; taken = true; --i; }
            }
            if (!taken) { --d; --j; }                        // j > 0 here: with j == 0 the insertion above was taken
            if (lane == 0) sops[w][nops] = code | (pi << 2) | (pos << 8);
            ++nops;
        }
    }
    __syncthreads();

    // ---- phase 3: the script and the tables
    if (active) {
        signed char* out = script + (size_t)b * EVAL_SCRIPT_WIDTH;
        for (int f = lane; f < EVAL_SCRIPT_WIDTH; f += 64) out[f] = f < nops ? (signed char)(sops[w][nops - 1 - f] & 3) : (signed char)-1;
        int count[4] = {0, 0, 0, 0};
        int* bypos = stab + EVAL_ERR_HEAD;
        long long* confusion = acc + EVAL_ERR_CONFUSION;
        for (int base = 0; base < nops; base += 64) {
            const int k = base + lane;
            const bool valid = k < nops;
            const int op = valid ? sops[w][k] : 0;
            const int code = valid ? (op & 3) : -1, pi = (op >> 2) & 31, pos = op >> 8;
            if (valid) {
                const int row = code == EVAL_OP_INSERTION ? T + 1 : eval_symbol_index(symbols, T, sgt[w][min(pos, EVAL_MAX_GT - 1)]);
                const int col = code == EVAL_OP_DELETION ? T + 1 : eval_symbol_index(symbols, T, spred[w][pi]);
                eval_add64(confusion + (size_t)row * (T + 2) + col, 1);
                int* cell = bypos + min(pos, EVAL_LEN_BINS - 1) * 4;
                if (code != EVAL_OP_INSERTION) atomicAdd(cell, 1);
                if (code == EVAL_OP_SUBSTITUTION) atomicAdd(cell + 1, 1);
                if (code == EVAL_OP_DELETION) atomicAdd(cell + 2, 1);
                if (code == EVAL_OP_INSERTION) atomicAdd(cell + 3, 1);
            }
#pragma unroll
            for (int c = 0; c < 4; ++c) count[c] += __popcll(__ballot(code == c));
        }
        const int exact = dist == 0;
        if (lane < 6) atomicAdd(stab + lane, lane == 0 ? 1 : lane == 1 ? count[0] : lane == 2 ? count[1] : lane == 3 ? count[2] : lane == 4 ? count[3] : exact);
        if (lane < 4) {
            eval_add64(acc + EVAL_ERR_BY_LENGTH + min(n, EVAL_LEN_BINS - 1) * 4 + lane, lane == 0 ? 1 : lane == 1 ? exact : lane == 2 ? dist : n);
            rows[(size_t)b * 4 + lane] = lane == 0 ? m : lane == 1 ? n : lane == 2 ? dist : exact;
        }
        if (lane == 0) script_len[b] = nops;
    }
    __syncthreads();

    // ---- phase 4: this workgroup's share of head and by_position
    if (threadIdx.x < EVAL_ERR_HEAD + EVAL_LEN_BINS * 4) {
        const int v = stab[threadIdx.x];
        if (v) eval_add64(acc + (threadIdx.x < EVAL_ERR_HEAD ? (int)threadIdx.x : EVAL_ERR_BY_POSITION + (int)threadIdx.x - EVAL_ERR_HEAD), v);
    }
}

}  // namespace pq
