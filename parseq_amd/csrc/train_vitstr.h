// ViTSTR's pieces of the training step (strhub/models/vitstr/system.py:75-79, base.py:194-204): the class-token assembly in front of
// the encoder, the row gathers of the patch-embedding gradient and of the per-token head.  One workgroup per output row, E columns.
#pragma once

#include "common.h"

// timm VisionTransformer._pos_embed: x[b, 0] = cls + pos[0], x[b, 1 + p] = proj[b, p] + pos[1 + p]   (proj: [B * (S - 1), E], bias included)
static __global__ __launch_bounds__(256)
void vitstr_tokens_kernel(const float* __restrict__ proj, const float* __restrict__ cls, const float* __restrict__ pos, float* __restrict__ x, int S, int E) {
    const int row = blockIdx.x, b = row / S, t = row % S;
    const float* src = t == 0 ? cls : proj + ((size_t)b * (S - 1) + t - 1) * E;
    for (int c = threadIdx.x; c < E; c += 256) x[(size_t)row * E + c] = src[c] + pos[(size_t)t * E + c];
}

// out[b, r] = in[b, r0 + r] for r < n_out: rows [r0, r0 + n_out) of every image of in ([B * n_in, E]) -> [B * n_out, E]
static __global__ __launch_bounds__(256)
void gather_image_rows_kernel(const float* __restrict__ in, int n_in, int r0, float* __restrict__ out, int n_out, int E) {
    const int row = blockIdx.x, b = row / n_out, r = row % n_out;
    const float* src = in + ((size_t)b * n_in + r0 + r) * E;
    for (int c = threadIdx.x; c < E; c += 256) out[(size_t)row * E + c] = src[c];
}

// the inverse with zero fill: out[b, t] = in[b, t - r0] for t in [r0, r0 + n_in), 0 elsewhere; out [B * n_out, E]
static __global__ __launch_bounds__(256)
void scatter_image_rows_kernel(const float* __restrict__ in, int n_in, int r0, float* __restrict__ out, int n_out, int E) {
    const int row = blockIdx.x, b = row / n_out, t = row % n_out;
    if (t < r0 || t >= r0 + n_in) {
        for (int c = threadIdx.x; c < E; c += 256) out[(size_t)row * E + c] = 0.f;
        return;
    }
    const float* src = in + ((size_t)b * n_in + (t - r0)) * E;
    for (int c = threadIdx.x; c < E; c += 256) out[(size_t)row * E + c] = src[c];
}
