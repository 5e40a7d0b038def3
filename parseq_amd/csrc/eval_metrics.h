// Evaluation metrics on the device: the per-sample loop of BaseSystem._eval_step (strhub/models/base.py:132-143) after the greedy decode —
// `pred = charset_adapter(pred)`, `edit_distance(pred, gt) / max(len(pred), len(gt))`, `pred == gt`, `len(pred)`, `prob.prod()` summed over
// the batch — without moving a string to the host.  parseq_eval_metrics (lib_ops.hip) runs postprocess_kernel (rowops.h) first, so ids,
// lengths and confidence ARE parseq_postprocess's; the two kernels here read them.
//
// What every evaluation kernel shares is stated here once: the front of a row (eval_row_front: clamps and adapter), the distance of a
// wave (eval_wave_distance: myers.h's step over the label, with or without the columns kept) and the fold of a batch into an
// accumulator (eval_fold).  eval_beams.h and eval_errors.h take all three.
#pragma once

#include "common.h"
#include "myers.h"

namespace pq {

constexpr int EVAL_MAX_PRED = 32;     // characters of a prediction: L <= DEC_MAXL positions, one lane each
constexpr int EVAL_MAX_GT = 256;      // code points of a ground-truth label

// The running totals of one evaluation (test.py:115-126 of the reference keeps them as Python numbers): 40 bytes of device memory.
struct EvalAccum {
    long long num_samples, correct, label_length;
    double ned, confidence;
};
static_assert(sizeof(EvalAccum) == 40, "the binding views the accumulator as 3 x int64 + 2 x float64");

// The steps of a row.  One wave per row, four rows per workgroup, lane j < plen owns character j.
//   adapter: table[id] is the code point CharsetAdapter (strhub/data/utils.py:26-43) turns train token `id` into, or -1 if it drops it;
//            the kept characters are compacted to lanes 0 .. m-1 through LDS (order preserved).  EVERY wave of the block calls this (it
//            holds the block's one barrier), a wave without a row with plen = 0.  Returns m; `pc` is the adapted character `lane`, -1 past m.
static __device__ __forceinline__ int eval_adapt_row(const int* __restrict__ ids_row, int plen, int C, const int* __restrict__ table, int* spred_w,
                                                     int lane, int& pc) {
    int cp = -1;
    if (lane < plen) {
        const int id = ids_row[lane];
        if (id >= 0 && id < C) cp = table[id];
    }
    const unsigned long long kept = __ballot(cp >= 0);
    const int m = __popcll(kept);
    spred_w[lane] = -1;
    if (cp >= 0) spred_w[__popcll(kept & ((1ull << lane) - 1ull))] = cp;      // kept lanes < 32, so the shift is defined
    __syncthreads();
    pc = spred_w[lane];
    return m;
}

//   front:   the length of a label on the device (the hosts refuse G > EVAL_MAX_GT; the cap is what the LDS of eval_errors.h is sized by),
static __device__ __forceinline__ int eval_label_length(int raw, int G) { return min(max(raw, 0), min(G, EVAL_MAX_GT)); }

//            and a wave's (m, n, pc) from the raw lengths of its row: both clamps and the adapter.  `live` is wave-uniform; a wave without
//            a row, or with a dead beam slot, adapts nothing (m = n = 0) but calls this all the same: eval_adapt_row's barrier is in here.
struct EvalRow { int m, n, pc; };
static __device__ __forceinline__ EvalRow eval_row_front(const int* __restrict__ ids_row, int plen, int L, int C, const int* __restrict__ table,
                                                         int glen, int G, bool live, int* spred_w, int lane) {
    EvalRow r;
    r.m = eval_adapt_row(ids_row, live ? min(max(plen, 0), min(L, EVAL_MAX_PRED)) : 0, C, table, spred_w, lane, r.pc);
    r.n = live ? eval_label_length(glen, G) : 0;
    return r;
}

//   distance: myers_step over the label, pattern = adapted prediction (m <= 32 bits of a 64-bit word), text = ground truth in chunks of
//            64 characters.  The match mask of a text character is a 64-lane ballot, everything else is wave-uniform integer arithmetic.
//            Called by whole waves only (all 64 lanes take part in the ballots and shuffles); m and n are wave-uniform.  An empty
//            prediction gives n.  KEEP (eval_errors.h) also stores, in LDS, the label's characters in `text` — whatever m is — and the
//            low 32 bits of every column's (Pv, Mv) in `cols`: column 0 is (Pv0, 0), lane i of a chunk stores column base + i + 1.
template <bool KEEP>
static __device__ __forceinline__ int eval_wave_distance(int pc, int m, const int* __restrict__ gt_row, int n, int lane, uint2* cols = nullptr,
                                                         int* text = nullptr) {
    if (!KEEP && m == 0) return n;
    unsigned long long Pv = m > 0 ? (1ull << m) - 1ull : 0ull, Mv = 0ull;      // m <= 32
    const unsigned long long top = m > 0 ? 1ull << (m - 1) : 0ull;
    if (KEEP && lane == 0) cols[0] = make_uint2((unsigned)Pv, 0u);
    int dist = m;
    for (int base = 0; base < n; base += 64) {
        const int mine = (base + lane < n) ? gt_row[base + lane] : -2;
        const int cnt = min(64, n - base);
        uint2 keep = make_uint2(0u, 0u);
        for (int i = 0; i < cnt; ++i) {
            const int c = __shfl(mine, i, 64);
            myers_step<unsigned long long>(__ballot(lane < m && pc == c), top, Pv, Mv, dist);
            if (KEEP && lane == i) keep = make_uint2((unsigned)Pv, (unsigned)Mv);
        }
        if (KEEP && lane < cnt) { cols[base + lane + 1] = keep; text[base + lane] = mine; }
    }
    return m == 0 ? n : dist;
}

//   rows[b] = {m, n, distance, pred == gt};  row_ned[b] = distance / max(m, n, 1) in double, summed by eval_reduce_kernel.
static __global__ __launch_bounds__(256)
void eval_rows_kernel(const int* __restrict__ ids, const int* __restrict__ lengths, int B, int L, int C, const int* __restrict__ table,
                      const int* __restrict__ gt, const int* __restrict__ gt_len, int G, int* __restrict__ rows, double* __restrict__ row_ned) {
    __shared__ int spred[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + w;
    const bool active = b < B;                               // a wave past the batch only keeps the barrier company
    const EvalRow r = eval_row_front(ids + (size_t)(active ? b : 0) * L, active ? lengths[b] : 0, L, C, table, active ? gt_len[b] : 0, G, active,
                                     spred[w], lane);
    if (!active) return;
    const int dist = eval_wave_distance<false>(r.pc, r.m, gt + (size_t)b * G, r.n, lane);
    if (lane == 0) {
        int* o = rows + (size_t)b * 4;
        o[0] = r.m; o[1] = r.n; o[2] = dist; o[3] = dist == 0;
        row_ned[b] = (double)dist / (double)max(max(r.m, r.n), 1);
    }
}

// The deterministic fold of a batch, for ONE workgroup of 256 threads: thread t sums rows t, t + 256, ... in order (`row(r)` adds row r to
// `ti` / `td`, which start at zero), then a fixed 128 -> 1 tree with one barrier per level — no atomics, so two runs over the same batches
// leave bit-identical totals.  True on thread 0 alone, whose `ti` / `td` then hold the batch's totals: it adds them to the accumulator.
// Calls on one stream are ordered, which is what makes that read-modify-write safe.
template <int NI, int ND, typename Row>
static __device__ __forceinline__ bool eval_fold(int B, long long (&ti)[NI], double (&td)[ND], Row row) {
    __shared__ long long si[NI][256];
    __shared__ double sd[ND][256];
    const int t = threadIdx.x;
#pragma unroll
    for (int k = 0; k < NI; ++k) ti[k] = 0;
#pragma unroll
    for (int k = 0; k < ND; ++k) td[k] = 0.0;
    for (int r = t; r < B; r += 256) row(r);
#pragma unroll
    for (int k = 0; k < NI; ++k) si[k][t] = ti[k];
#pragma unroll
    for (int k = 0; k < ND; ++k) sd[k][t] = td[k];
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) {
#pragma unroll
            for (int k = 0; k < NI; ++k) si[k][t] += si[k][t + o];
#pragma unroll
            for (int k = 0; k < ND; ++k) sd[k][t] += sd[k][t + o];
        }
        __syncthreads();
    }
    if (t != 0) return false;
#pragma unroll
    for (int k = 0; k < NI; ++k) ti[k] = si[k][0];
#pragma unroll
    for (int k = 0; k < ND; ++k) td[k] = sd[k][0];
    return true;
}

// One workgroup adds the batch to the accumulator.
static __global__ __launch_bounds__(256)
void eval_reduce_kernel(const int* __restrict__ rows, const double* __restrict__ row_ned, const float* __restrict__ conf, int B,
                        EvalAccum* __restrict__ acc) {
    long long ti[2];                                         // correct, label_length
    double td[2];                                            // ned, confidence
    if (eval_fold(B, ti, td, [&](int r) {
            ti[0] += rows[(size_t)r * 4 + 3]; ti[1] += rows[(size_t)r * 4];
            td[0] += row_ned[r]; td[1] += (double)conf[r];
        })) {
        acc->num_samples += B; acc->correct += ti[0]; acc->label_length += ti[1];
        acc->ned += td[0]; acc->confidence += td[1];
    }
}

}  // namespace pq
