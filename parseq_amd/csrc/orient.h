// The choice among K turned views of a crop: rows b K .. b K + K - 1 of a batch are the views of crop b,
// postprocess_kernel (rowops.h) has left every row's ids, first-<eos> index, per-position probabilities and confidence in the workspace,
// and one workgroup per crop computes the K keys, finds the winner through LDS and copies the winner's rows out.
#pragma once
#include "common.h"

namespace pq {

constexpr int ORIENT_MAX_VIEWS = 8;
constexpr int ORIENT_THREADS = 256;
enum { ORIENT_MEAN = 0, ORIENT_SUM = 1 };

// n bytes from src to dst by the whole workgroup.  W = the widest of 16, 8, 4, 1 bytes at which the two addresses are congruent; the at
// most W - 1 bytes ahead of the first W-aligned address and the at most W - 1 behind the last go one byte per thread.  (L C is odd for
// the usual shapes, so consecutive logits rows alternate between 8- and 4-byte offsets; a u8 crop has no alignment at all.)
template <typename V>
static __device__ __forceinline__ void orient_copy_as(unsigned char* __restrict__ dst, const unsigned char* __restrict__ src, size_t n) {
    constexpr size_t W = sizeof(V);
    size_t head = (size_t)(-(intptr_t)reinterpret_cast<uintptr_t>(src)) & (W - 1);
    if (head > n) head = n;
    const size_t body = (n - head) / W, tail0 = head + body * W;
    for (size_t i = threadIdx.x; i < head; i += ORIENT_THREADS) dst[i] = src[i];
    const V* s = reinterpret_cast<const V*>(src + head);
    V* d = reinterpret_cast<V*>(dst + head);
    for (size_t i = threadIdx.x; i < body; i += ORIENT_THREADS) d[i] = s[i];
    for (size_t i = tail0 + threadIdx.x; i < n; i += ORIENT_THREADS) dst[i] = src[i];
}

static __device__ __forceinline__ void orient_copy(void* dst_, const void* src_, size_t n) {
    unsigned char* dst = static_cast<unsigned char*>(dst_);
    const unsigned char* src = static_cast<const unsigned char*>(src_);
    const uintptr_t x = reinterpret_cast<uintptr_t>(dst) ^ reinterpret_cast<uintptr_t>(src);
    if ((x & 15) == 0) orient_copy_as<uint4>(dst, src, n);
    else if ((x & 7) == 0) orient_copy_as<uint2>(dst, src, n);
    else if ((x & 3) == 0) orient_copy_as<unsigned>(dst, src, n);
    else orient_copy_as<unsigned char>(dst, src, n);
}

// key of view k = s or s / n, s = sum_{i < n} log((double)p_i) added in position order, n = min(len + 1, L); + prior[k]; NaN = -inf.
// The winner is the first k of the largest key (view 0 when every key is -inf).  ids / lens / probs / confs: what postprocess_kernel wrote
// for the B K rows.  images / images_out may be null; image_bytes = bytes of one crop.
static __global__ __launch_bounds__(ORIENT_THREADS)
void orient_select_kernel(const float* __restrict__ logits, const int* __restrict__ ids, const int* __restrict__ lens, const float* __restrict__ probs,
                          const float* __restrict__ confs, const void* __restrict__ images, size_t image_bytes, int K, int L, int C, int criterion,
                          const float* __restrict__ prior, int* __restrict__ view_out, double* __restrict__ keys_out, float* __restrict__ logits_out,
                          int* __restrict__ ids_out, int* __restrict__ lens_out, float* __restrict__ conf_out, void* __restrict__ images_out) {
    __shared__ double logp[ORIENT_MAX_VIEWS][64];
    __shared__ double key[ORIENT_MAX_VIEWS];
    __shared__ int winner;
    const size_t b = blockIdx.x;
    const int t = threadIdx.x;
    // every log on a thread of its own (K L <= 512 of them), then thread k adds view k's in position order
    for (int i = t; i < K * L; i += ORIENT_THREADS) {
        const int k = i / L, l = i - k * L;
        logp[k][l] = log((double)probs[(b * K + k) * L + l]);
    }
    __syncthreads();
    if (t < K) {
        const int n = min(lens[b * K + t] + 1, L);
        double s = 0.0;
        for (int i = 0; i < n; ++i) s += logp[t][i];
        if (criterion == ORIENT_MEAN) s /= (double)n;
        if (prior) s += (double)prior[t];
        if (s != s) s = -INFINITY;
        key[t] = s;
        keys_out[b * K + t] = s;
    }
    __syncthreads();
    if (t == 0) {
        int w = 0;
        double best = -INFINITY;
        for (int k = 0; k < K; ++k)
            if (key[k] > best) { best = key[k]; w = k; }
        winner = w;
        view_out[b] = w;
    }
    __syncthreads();
    const size_t row = b * K + winner;
    if (t < L) ids_out[b * L + t] = ids[row * L + t];
    if (t == 0) { lens_out[b] = lens[row]; conf_out[b] = confs[row]; }
    const size_t lbytes = (size_t)L * C * sizeof(float);
    orient_copy(reinterpret_cast<unsigned char*>(logits_out) + b * lbytes, reinterpret_cast<const unsigned char*>(logits) + row * lbytes, lbytes);
    if (images_out)
        orient_copy(static_cast<unsigned char*>(images_out) + b * image_bytes, static_cast<const unsigned char*>(images) + row * image_bytes, image_bytes);
}

}  // namespace pq
