// Evaluation metrics on the device: the per-sample loop of BaseSystem._eval_step (strhub/models/base.py:132-143) after the greedy decode —
// `pred = charset_adapter(pred)`, `edit_distance(pred, gt) / max(len(pred), len(gt))`, `pred == gt`, `len(pred)`, `prob.prod()` summed over
// the batch — without moving a string to the host.  parseq_eval_metrics (lib_ops.hip) runs postprocess_kernel (rowops.h) first, so ids,
// lengths and confidence ARE parseq_postprocess's; the two kernels here read them.
#pragma once

#include "common.h"

namespace pq {

constexpr int EVAL_MAX_PRED = 32;     // characters of a prediction: L <= DEC_MAXL positions, one lane each
constexpr int EVAL_MAX_GT = 256;      // code points of a ground-truth label

// The running totals of one evaluation (test.py:115-126 of the reference keeps them as Python numbers): 40 bytes of device memory.
struct EvalAccum {
    long long num_samples, correct, label_length;
    double ned, confidence;
};
static_assert(sizeof(EvalAccum) == 40, "the binding views the accumulator as 3 x int64 + 2 x float64");

// The two steps of a row, shared by eval_rows_kernel and the N-best kernel of eval_beams.h.  One wave per row, lane j < plen owns character j.
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

//   distance: Myers' bit-vector recurrence in Hyyro's form for the global (Levenshtein) distance, pattern = adapted prediction (m <= 32
//            bits of a 64-bit word), text = ground truth.  The match mask of a text character is a 64-lane ballot, everything else is
//            wave-uniform integer arithmetic: len(gt) short steps, unit costs, no transpositions (nltk.edit_distance defaults).
//            Called by whole waves only (all 64 lanes take part in the ballots and shuffles); m and n are wave-uniform.
static __device__ __forceinline__ int eval_row_distance(int pc, int m, const int* __restrict__ gt_row, int n, int lane) {
    int dist = n;                                            // empty prediction: n insertions
    if (m > 0) {
        unsigned long long Pv = (1ull << m) - 1ull, Mv = 0ull;      // m <= 32
        const unsigned long long top = 1ull << (m - 1);
        dist = m;
        for (int base = 0; base < n; base += 64) {
            const int mine = (base + lane < n) ? gt_row[base + lane] : -2;
            const int cnt = min(64, n - base);
            for (int i = 0; i < cnt; ++i) {
                const int c = __shfl(mine, i, 64);
                const unsigned long long Eq = __ballot(lane < m && pc == c);
                const unsigned long long Xv = Eq | Mv;
                const unsigned long long Xh = (((Eq & Pv) + Pv) ^ Pv) | Eq;
                unsigned long long Ph = Mv | ~(Xh | Pv);
                unsigned long long Mh = Pv & Xh;
                dist += (Ph & top) ? 1 : 0;
                dist -= (Mh & top) ? 1 : 0;
                Ph = (Ph << 1) | 1ull;                       // row 0 of the table grows by one per text character (global distance)
                Mh <<= 1;
                Pv = Mh | ~(Xv | Ph);
                Mv = Ph & Xv;
            }
        }
    }
    return dist;
}

//   rows[b] = {m, n, distance, pred == gt};  row_ned[b] = distance / max(m, n, 1) in double, summed by eval_reduce_kernel.
static __global__ __launch_bounds__(256)
void eval_rows_kernel(const int* __restrict__ ids, const int* __restrict__ lengths, int B, int L, int C, const int* __restrict__ table,
                      const int* __restrict__ gt, const int* __restrict__ gt_len, int G, int* __restrict__ rows, double* __restrict__ row_ned) {
    __shared__ int spred[4][64];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int b = blockIdx.x * 4 + w;
    const bool active = b < B;                               // a wave past the batch only keeps the barrier company
    const int plen = active ? min(max(lengths[b], 0), min(L, EVAL_MAX_PRED)) : 0;
    int pc;
    const int m = eval_adapt_row(ids + (size_t)(active ? b : 0) * L, plen, C, table, spred[w], lane, pc);
    if (!active) return;
    const int n = min(max(gt_len[b], 0), G);
    const int dist = eval_row_distance(pc, m, gt + (size_t)b * G, n, lane);
    if (lane == 0) {
        int* r = rows + (size_t)b * 4;
        r[0] = m; r[1] = n; r[2] = dist; r[3] = dist == 0;
        row_ned[b] = (double)dist / (double)max(max(m, n), 1);
    }
}

// One workgroup adds the batch to the accumulator: each thread sums rows tid, tid + 256, ... in order, then a fixed tree — no atomics, so two
// runs over the same batches leave bit-identical totals.  Calls on one stream are ordered, which is what makes the read-modify-write safe.
static __global__ __launch_bounds__(256)
void eval_reduce_kernel(const int* __restrict__ rows, const double* __restrict__ row_ned, const float* __restrict__ conf, int B,
                        EvalAccum* __restrict__ acc) {
    __shared__ double sned[256], sconf[256];
    __shared__ long long scorrect[256], slen[256];
    double ned = 0.0, cf = 0.0;
    long long correct = 0, len = 0;
    for (int r = threadIdx.x; r < B; r += 256) {
        ned += row_ned[r]; cf += (double)conf[r];
        correct += rows[(size_t)r * 4 + 3]; len += rows[(size_t)r * 4];
    }
    sned[threadIdx.x] = ned; sconf[threadIdx.x] = cf; scorrect[threadIdx.x] = correct; slen[threadIdx.x] = len;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sned[threadIdx.x] += sned[threadIdx.x + o]; sconf[threadIdx.x] += sconf[threadIdx.x + o];
            scorrect[threadIdx.x] += scorrect[threadIdx.x + o]; slen[threadIdx.x] += slen[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        acc->num_samples += B; acc->correct += scorrect[0]; acc->label_length += slen[0];
        acc->ned += sned[0]; acc->confidence += sconf[0];
    }
}

}  // namespace pq
