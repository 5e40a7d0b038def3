// Evaluation of an N-best on the device: the reference's metrics (strhub/models/base.py:132-143) for the first live
// hypothesis of every image, plus what only a search has — at which rank the truth stands, and how near the nearest hypothesis comes —
// for any BeamResult (beam.h, lexicon_match.h), without moving a string to the host.  Two launches, no atomics:
//   eval_beam_rows_kernel    one wave per hypothesis (row b * W + w): eval_row_front and eval_wave_distance of eval_metrics.h;
//   eval_beam_images_kernel  ONE workgroup: thread t folds the W rows of images t, t + 256, ... and eval_fold (eval_metrics.h) sums
//                            them in that order, then over its fixed tree, into the accumulator.
#pragma once

#include "eval_metrics.h"

namespace pq {

constexpr int EVAL_MAX_BEAMS = 17;          // W: the 16 candidates of a lexicon match plus the reading (keep_reading)
constexpr int EVAL_BEAM_IMAGE_ROW = 8;      // int32 words of an image row
constexpr int EVAL_BEAM_NO_HIT = -1;        // image row: no live hypothesis equals the label / no live slot
constexpr int EVAL_BEAM_DEAD = -1;          // m, n and distance of a dead slot's hypothesis row (exact 0, ned -1.0)

struct BeamEvalAccum {
    long long num_samples, correct, label_length, top1_distance, oracle_correct, oracle_distance, live, miss, first_hit[EVAL_MAX_BEAMS];
    double ned, confidence, oracle_ned;
};
static_assert(sizeof(BeamEvalAccum) == 224, "the binding views the accumulator as 25 x int64 + 3 x float64");

// A slot is live iff its score is not -inf (tokenizer.decode_beams' rule; a NaN is live).
static __device__ __forceinline__ bool eval_beam_live(float score) { return score != -__builtin_huge_valf(); }

// rows[r] = {m, n, distance, exact} of hypothesis r = b * W + w against the label of image b;  hyp_ned[r] = distance / max(m, n, 1).
static __global__ __launch_bounds__(256)
void eval_beam_rows_kernel(const int* __restrict__ tokens, const float* __restrict__ scores, const int* __restrict__ lengths, int rows_total, int W,
                           int T, int C, const int* __restrict__ table, const int* __restrict__ gt, const int* __restrict__ gt_len, int G,
                           int* __restrict__ rows, double* __restrict__ hyp_ned) {
    __shared__ int spred[4][64];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int r = blockIdx.x * 4 + wv;
    const bool active = r < rows_total;                      // wave-uniform: a wave past the rows only keeps the barrier company
    const bool live = active && eval_beam_live(scores[r]);   // wave-uniform too: a dead slot adapts nothing and writes the sentinel
    const int b = r / W;
    const EvalRow row = eval_row_front(tokens + (size_t)(live ? r : 0) * T, live ? lengths[r] : 0, T, C, table, live ? gt_len[b] : 0, G, live,
                                       spred[wv], lane);
    if (!active) return;
    if (!live) {
        if (lane == 0) {
            int* o = rows + (size_t)r * 4;
            o[0] = EVAL_BEAM_DEAD; o[1] = EVAL_BEAM_DEAD; o[2] = EVAL_BEAM_DEAD; o[3] = 0;
            hyp_ned[r] = -1.0;
        }
        return;
    }
    const int dist = eval_wave_distance<false>(row.pc, row.m, gt + (size_t)b * G, row.n, lane);
    if (lane == 0) {
        int* o = rows + (size_t)r * 4;
        o[0] = row.m; o[1] = row.n; o[2] = dist; o[3] = dist == 0;
        hyp_ned[r] = (double)dist / (double)max(max(row.m, row.n), 1);
    }
}

// image_rows[b] = {m, n, distance, exact of the top-1 (the first live slot), first_hit, oracle_distance, live, top-1's slot};
// img[0 .. B) = top-1 ned, img[B .. 2B) = oracle ned, img[2B .. 3B) = confidence.  An image without a live slot reads as the empty string.
static __global__ __launch_bounds__(256)
void eval_beam_images_kernel(const int* __restrict__ rows, const double* __restrict__ hyp_ned, const float* __restrict__ scores,
                             const float* __restrict__ conf_scores, int B, int W, const int* __restrict__ gt_len, int G,
                             int* __restrict__ image_rows, double* __restrict__ img, BeamEvalAccum* __restrict__ acc) {
    long long ti[6 + EVAL_MAX_BEAMS];                        // correct, label_length, top1_distance, oracle_distance, live, miss, first_hit[]
    double td[3];                                            // ned, confidence, oracle_ned
    // eval_fold's LDS is 46 KiB + 6 KiB here: the one workgroup has the compute unit to itself
    const bool first = eval_fold(B, ti, td, [&](int b) {
        const int n = eval_label_length(gt_len[b], G);
        int top = -1, hit = EVAL_BEAM_NO_HIT, live = 0, odist = 0;
        double oned = 0.0;
        for (int w = 0; w < W; ++w) {
            const int r = b * W + w;
            if (!eval_beam_live(scores[r])) continue;
            const int d = rows[(size_t)r * 4 + 2];
            const double e = hyp_ned[r];
            if (live == 0) { top = w; odist = d; oned = e; }
            else { odist = min(odist, d); oned = e < oned ? e : oned; }
            if (hit == EVAL_BEAM_NO_HIT && d == 0) hit = live;
            ++live;
        }
        int m = 0, dist = n, exact = 0;
        double ned = (double)n / (double)max(n, 1), conf = 0.0;
        if (top >= 0) {
            const int r = b * W + top;
            m = rows[(size_t)r * 4]; dist = rows[(size_t)r * 4 + 2]; exact = rows[(size_t)r * 4 + 3];
            ned = hyp_ned[r];
            conf = exp((double)conf_scores[r]);
        } else {
            odist = n; oned = ned;
        }
        int* o = image_rows + (size_t)b * EVAL_BEAM_IMAGE_ROW;
        o[0] = m; o[1] = n; o[2] = dist; o[3] = exact; o[4] = hit; o[5] = odist; o[6] = live; o[7] = top;
        img[b] = ned; img[(size_t)B + b] = oned; img[2 * (size_t)B + b] = conf;
        ti[0] += exact; ti[1] += m; ti[2] += dist; ti[3] += odist; ti[4] += live; ti[5] += hit == EVAL_BEAM_NO_HIT;
#pragma unroll
        for (int k = 0; k < EVAL_MAX_BEAMS; ++k) ti[6 + k] += hit == k;
        td[0] += ned; td[1] += conf; td[2] += oned;
    });
    if (first) {
        acc->num_samples += B; acc->correct += ti[0]; acc->label_length += ti[1]; acc->top1_distance += ti[2];
        acc->oracle_correct += (long long)B - ti[5]; acc->oracle_distance += ti[3]; acc->live += ti[4]; acc->miss += ti[5];
#pragma unroll
        for (int k = 0; k < EVAL_MAX_BEAMS; ++k) acc->first_hit[k] += ti[6 + k];
        acc->ned += td[0]; acc->confidence += td[1]; acc->oracle_ned += td[2];
    }
}

}  // namespace pq
