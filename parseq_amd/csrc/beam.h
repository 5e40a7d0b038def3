// Beam search over the AR decoder: the per-step selection kernel, the replication of the encoder memory over the
// beams of an image, and the small init / write-out kernels.  A beam is a token history (a row of the plan's pitched token array), a
// score, a finished flag and a length; at decoder depth 1 the self-attention keys are table lookups by (token id, position), so
// re-parenting a beam is a copy of its history row and nothing else.  Under a lexicon a beam also carries the trie node
// its history has reached and, once finished, the id of the word it spelled.  Under a weighted automaton the table
// has a weight per arc, a beam also carries the sum of the weights along its path, and the ranking is by the fused value.
#pragma once
#include <type_traits>
#include "common.h"

namespace pq {

constexpr int BEAM_MAX_W = 16;         // beams per image
constexpr int BEAM_THREADS = 256;      // four waves per image
constexpr size_t BEAM_LDS_MAX = 60 * 1024;      // dynamic LDS of the step kernel (64 KiB a workgroup with its static arrays)

// dynamic LDS of beam_step_kernel: the candidates [W][C] f32, the W finished carries, the image's W history rows [W][ldt] int
static inline size_t beam_step_lds(int W, int C, int ldt) { return ((size_t)W * C + W) * sizeof(float) + (size_t)W * ldt * sizeof(int); }

// A float as an unsigned integer of the same order (-inf lowest; NaN never gets here).
__device__ __forceinline__ unsigned beam_ordered(float v) {
    const unsigned u = __float_as_uint(v);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// The lexicon of a constrained step: the dense trie table next [nodes][C] (a negative entry: not allowed; the <eos> column holds word ids)
// and, per beam row and in place, the node reached and the word finished (-1: none).  Unused by the unconstrained instantiation.
struct BeamLex { const int* next; int nodes; int* node; int* word; };
// The automaton of a weighted step: BeamLex's members with `nodes` the number of states, then the arc weights weight [nodes][C] (natural
// log; a non-finite one: not allowed), per beam row and in place the sum of the weights along its path, the prior weight alpha and the
// per-character bonus beta, and fused [rows] (may be null): where each new beam's fused value goes.
struct BeamAut { const int* next; int nodes; int* node; int* word; const float* weight; float* wsum; float alpha, beta; float* fused; };

// The fused value of a hypothesis of model score m, weight sum ws and k characters: m + (alpha ws + beta k), every operation rounded on
// its own — the pragma forbids contraction into an fma, which the compiler's default allows — so that the step, the carry and the write-out
// give the same bits from the same (m, ws, k).  A finite alpha can still overflow a product: a value that is not finite comes back as -inf,
// "no candidate", so neither +inf nor NaN ever enters the ranking.
__device__ __forceinline__ float beam_fused(float m, float ws, int k, float alpha, float beta) {
#pragma clang fp contract(off)
    const float f = m + (alpha * ws + beta * (float)k);
    if (!(f - f == 0.f)) return -INFINITY;
    return f == 0.f ? 0.f : f;      // one zero, as for the scores
}

// One selection step of one image per workgroup.  In: logits [B * W][C] of the step, and the image's W beams in place — history rows
// tok[(b W + w) ldt ..], score, finished, length.  Candidates: every live unfinished beam w offers (w, c) at score[w] +
// log_softmax(logits[w])[c], every finished beam itself at its score (class -1), a dead beam (score -inf) nothing.  The W best become the
// new beams in rank order: higher score first, then the lower parent, then the lower class.  A slot left without a candidate is dead:
// score -inf, parent -1, its own row's history kept.  Position step + 1 of a new history holds the picked class (pad_id for a carry or
// a dead slot); picked[] repeats it for a caller whose rows have no such position (step + 1 == ldt).
// The histories are re-parented through LDS: every row of the image is loaded before the barrier and written after it.
// LEX: a live unfinished beam at node n offers (w, c) only where next[n][c] >= 0 (and, for a character, < nodes: the table is the caller's
// device data, a child id past it is treated as not allowed, as is every class of a beam whose own node is outside [0, nodes)).  The scores
// are the unconstrained ones: the log-soft-max runs over all C classes.  A new beam's node is next[node_parent][c]; picking <eos> keeps the
// node and records word = next[node][eos_id]; a carry keeps both; a dead slot holds -1 / -1.  Nodes and words are re-parented like the
// histories: all W loaded before the first barrier, written after the last.
// WGT (with LEX; lx is then a BeamAut): the candidate array holds the fused value f = m + (alpha (wsum[w] + weight[n][c]) + beta k), m the
// score above and k the characters the hypothesis would have (step + 1, step for <eos>); a finished beam carries at score + (alpha wsum +
// beta length).  An arc whose weight, or whose sum with the beam's wsum, is not finite is not allowed, so no product sees an infinity;
// alpha and beta are finite (the entries refuse others), and a candidate or carry whose f overflows all the same is not allowed either
// (beam_fused).  The ranking, the ties and the keys are the same, on f.  score[] stays the
// model's sum: for a picked candidate it is RECOMPUTED from the row's kept maximum and log-sum (two floats per beam in LDS, one logit read
// per new beam) by the expression that made the candidate, which gives the same bits, rather than kept in a second [W][C] array that would
// double the LDS.  wsum is re-parented like node and word: loaded before the first barrier, written after the last; a dead slot holds 0.
// f is never carried: the next step and the write-out recompute it from (score, wsum, length).
template <bool LEX, bool WGT = false>
static __global__ __launch_bounds__(BEAM_THREADS)
void beam_step_kernel(const float* __restrict__ logits, int W, int C, int step, int* __restrict__ tok, int ldt, float* __restrict__ score,
                      unsigned char* __restrict__ finished, int* __restrict__ length, int* __restrict__ parent_out, int* __restrict__ picked,
                      int eos_id, int pad_id, std::conditional_t<WGT, BeamAut, BeamLex> lx) {
    static_assert(LEX || !WGT, "a weighted step walks a table");
    extern __shared__ float beam_smem[];
    float* cand = beam_smem;                                       // [W * C] fresh candidates, then [W] carries
    int* hist = reinterpret_cast<int*>(beam_smem + (size_t)W * C + W);
    __shared__ float s_score[BEAM_MAX_W], sel_score[BEAM_MAX_W];
    __shared__ int s_len[BEAM_MAX_W], sel_parent[BEAM_MAX_W], sel_cls[BEAM_MAX_W];
    __shared__ unsigned char s_fin[BEAM_MAX_W];
    __shared__ int s_node[LEX ? BEAM_MAX_W : 1], s_word[LEX ? BEAM_MAX_W : 1];
    __shared__ float s_wsum[WGT ? BEAM_MAX_W : 1], s_rmax[WGT ? BEAM_MAX_W : 1], s_rlg[WGT ? BEAM_MAX_W : 1];
    __shared__ unsigned long long s_wkey[BEAM_THREADS / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t row0 = (size_t)blockIdx.x * W;
    if (tid < W) { s_score[tid] = score[row0 + tid]; s_fin[tid] = finished[row0 + tid]; s_len[tid] = length[row0 + tid]; }
    if constexpr (LEX) { if (tid < W) { s_node[tid] = lx.node[row0 + tid]; s_word[tid] = lx.word[row0 + tid]; } }
    if constexpr (WGT) { if (tid < W) s_wsum[tid] = lx.wsum[row0 + tid]; }
    for (int i = tid; i < W * ldt; i += BEAM_THREADS) hist[i] = tok[row0 * ldt + i];
    __syncthreads();

    // log-soft-max of every live row (a wave per row), candidates into LDS
    for (int w = wave; w < W; w += BEAM_THREADS / 64) {
        const float sc = s_score[w];
        const bool fin = s_fin[w] != 0, alive = sc > -INFINITY;
        float* out = cand + (size_t)w * C;
        if (alive && !fin) {
            const float* row = logits + (row0 + w) * C;
            float m = -INFINITY;
            for (int c = lane; c < C; c += 64) m = fmaxf(m, row[c]);
            m = wave_max(m);
            float sum = 0.f;
            for (int c = lane; c < C; c += 64) sum += expf(row[c] - m);
            const float lg = logf(wave_sum(sum));
            const int* allowed = nullptr;      // LEX: the node's row of the table, null for a node outside it
            if constexpr (LEX) { const int nd = s_node[w]; if (nd >= 0 && nd < lx.nodes) allowed = lx.next + (size_t)nd * C; }
            const float* wrow = nullptr;       // WGT: the node's row of the weights, null with `allowed`
            if constexpr (WGT) {
                if (allowed) wrow = lx.weight + (size_t)s_node[w] * C;
                if (lane == 0) { s_rmax[w] = m; s_rlg[w] = lg; }
            }
            for (int c = lane; c < C; c += 64) {
                float v = sc + ((row[c] - m) - lg);
                if (v == 0.f) v = 0.f;      // one zero: the ordering below is on the bits
                if constexpr (LEX) {
                    const int t = allowed ? allowed[c] : -1;
                    if (t < 0 || (c != eos_id && t >= lx.nodes)) v = -INFINITY;
                }
                if constexpr (WGT) {
                    if (v > -INFINITY) {      // an allowed arc, so wrow is set
                        const float ws = s_wsum[w] + wrow[c];
                        v = (ws - ws == 0.f) ? beam_fused(v, ws, c == eos_id ? step : step + 1, lx.alpha, lx.beta) : -INFINITY;
                    }
                }
                out[c] = v;
            }
        } else {
            for (int c = lane; c < C; c += 64) out[c] = -INFINITY;
        }
        if constexpr (WGT) { if (lane == 0) cand[(size_t)W * C + w] = (alive && fin) ? beam_fused(sc, s_wsum[w], s_len[w], lx.alpha, lx.beta) : -INFINITY; }
        else if (lane == 0) cand[(size_t)W * C + w] = (alive && fin) ? (sc == 0.f ? 0.f : sc) : -INFINITY;
    }
    __syncthreads();

    // W rounds of a block-wide arg-max over (score, parent, class) keys; a taken candidate becomes -inf
    const int total = W * C + W;
    const unsigned cls_span = (unsigned)C + 1u;
    for (int r = 0; r < W; ++r) {
        unsigned long long best = 0;      // 0 = no candidate (a real key has a non-zero score half)
        for (int idx = tid; idx < total; idx += BEAM_THREADS) {
            const float v = cand[idx];
            if (v > -INFINITY) {
                unsigned order;
                if (idx < W * C) { const unsigned par = (unsigned)idx / (unsigned)C; order = par * cls_span + ((unsigned)idx - par * (unsigned)C) + 1u; }
                else order = (unsigned)(idx - W * C) * cls_span;
                const unsigned long long key = ((unsigned long long)beam_ordered(v) << 32) | (unsigned long long)(0xFFFFFFFFu - order);
                best = key > best ? key : best;
            }
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const unsigned long long o = __shfl_xor(best, d, 64);
            best = o > best ? o : best;
        }
        if (lane == 0) s_wkey[wave] = best;
        __syncthreads();
        if (tid == 0) {
            unsigned long long k = s_wkey[0];
            for (int i = 1; i < BEAM_THREADS / 64; ++i) k = s_wkey[i] > k ? s_wkey[i] : k;
            if (k == 0) { sel_parent[r] = -1; sel_cls[r] = -1; sel_score[r] = -INFINITY; }
            else {
                const unsigned order = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
                const int par = (int)(order / cls_span), cls = (int)(order % cls_span) - 1;
                const int idx = cls < 0 ? W * C + par : par * C + cls;
                sel_parent[r] = par; sel_cls[r] = cls; sel_score[r] = cand[idx];
                cand[idx] = -INFINITY;
            }
        }
        __syncthreads();
    }

    // the new beams
    for (int i = tid; i < W * ldt; i += BEAM_THREADS) {
        const int r = i / ldt, j = i - r * ldt;
        const int par = sel_parent[r];
        int v = hist[(par >= 0 ? par : r) * ldt + j];
        if (j == step + 1) v = sel_cls[r] >= 0 ? sel_cls[r] : pad_id;
        tok[row0 * ldt + i] = v;
    }
    if (tid < W) {
        const int par = sel_parent[tid], cls = sel_cls[tid];
        const bool dead = par < 0, carry = !dead && cls < 0;
        if constexpr (!WGT) score[row0 + tid] = sel_score[tid];
        finished[row0 + tid] = dead ? 0 : (carry || cls == eos_id ? 1 : 0);
        length[row0 + tid] = dead ? 0 : (carry ? s_len[par] : (cls == eos_id ? step : step + 1));
        picked[row0 + tid] = cls >= 0 ? cls : pad_id;
        if (parent_out) parent_out[row0 + tid] = par;
        if constexpr (LEX) {
            int nd = -1, wd = -1;
            if (carry) { nd = s_node[par]; wd = s_word[par]; }
            else if (!dead) {      // a picked class was allowed, so the parent's node is inside the table
                nd = s_node[par];
                const int t = lx.next[(size_t)nd * C + cls];
                if (cls == eos_id) wd = t; else nd = t;
            }
            lx.node[row0 + tid] = nd; lx.word[row0 + tid] = wd;
        }
        if constexpr (WGT) {
            float ms = -INFINITY, ws = 0.f;
            if (carry) { ms = s_score[par]; ws = s_wsum[par]; }
            else if (!dead) {      // the candidate's own expressions again: the same bits
                ms = s_score[par] + ((logits[(row0 + par) * C + cls] - s_rmax[par]) - s_rlg[par]);
                ws = s_wsum[par] + lx.weight[(size_t)s_node[par] * C + cls];
            }
            score[row0 + tid] = ms == 0.f ? 0.f : ms;
            lx.wsum[row0 + tid] = ws;
            if (lx.fused) lx.fused[row0 + tid] = sel_score[tid];
        }
    }
}

// dst [B * W][per_img] = src [B][per_img] with row b W + w a copy of image b; 16-byte accesses (per_img4 float4 per image).
static __global__ __launch_bounds__(256)
void beam_replicate_kernel(const float4* __restrict__ src, float4* __restrict__ dst, size_t per_img4, int W, size_t total4) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total4) return;
    const size_t row = i / per_img4, off = i - row * per_img4;
    dst[i] = src[(row / (size_t)W) * per_img4 + off];
}

// The start of a search: beam 0 of every image is [<bos>] at score 0, the others are dead; histories in the layout of ar_init_kernel.
static __global__ void beam_init_kernel(int* __restrict__ tok, int ldt, int rows, int W, int bos_id, int pad_id, float* __restrict__ score,
                                        unsigned char* __restrict__ finished, int* __restrict__ length, int* __restrict__ picked) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * ldt) tok[i] = (i % ldt == 0) ? bos_id : pad_id;
    if (i < rows) { score[i] = (i % W == 0) ? 0.f : -INFINITY; finished[i] = 0; length[i] = 0; picked[i] = pad_id; }
}

// The start under a lexicon, after beam_init_kernel: beam 0 of image b stands at roots[b] (0 without roots), the others at -1; an image whose
// root is outside [0, nodes) starts with every beam dead.
static __global__ void beam_init_lexicon_kernel(int rows, int W, const int* __restrict__ roots, int nodes, float* __restrict__ score,
                                                int* __restrict__ node, int* __restrict__ word) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    int nd = -1;
    if (i % W == 0) {
        nd = roots ? roots[i / W] : 0;
        if (nd < 0 || nd >= nodes) { nd = -1; score[i] = -INFINITY; }
    }
    node[i] = nd; word[i] = -1;
}

// The write-out under a lexicon, beside beam_finish_kernel: words_out [rows], the word id of a finished hypothesis, -1 otherwise.
static __global__ void beam_finish_lexicon_kernel(int rows, const float* __restrict__ score, const unsigned char* __restrict__ finished,
                                                  const int* __restrict__ word, int* __restrict__ words_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) words_out[i] = (score[i] > -INFINITY && finished[i]) ? word[i] : -1;
}

// The start under a weighted automaton, after beam_init_lexicon_kernel: every beam's weight sum is 0.
static __global__ void beam_init_automaton_kernel(int rows, float* __restrict__ wsum) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows) wsum[i] = 0.f;
}

// The write-out under a weighted automaton, after beam_finish_kernel: scores_out [rows] becomes the fused value the ranking used, recomputed
// from the carried (score, wsum, length); model_scores_out the carried score, priors_out the weight sum (-inf, -inf and 0 for a dead beam).
static __global__ void beam_finish_automaton_kernel(int rows, const float* __restrict__ score, const float* __restrict__ wsum,
                                                    const int* __restrict__ length, float alpha, float beta, float* __restrict__ scores_out,
                                                    float* __restrict__ model_scores_out, float* __restrict__ priors_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows) return;
    const bool dead = !(score[i] > -INFINITY);
    scores_out[i] = dead ? -INFINITY : beam_fused(score[i], wsum[i], length[i], alpha, beta);
    model_scores_out[i] = score[i]; priors_out[i] = dead ? 0.f : wsum[i];
}

// The write-out: the beams are in rank order after every step, so this only drops <bos> and the pitch.  tokens_out [rows][num_steps];
// a dead beam's tokens are all pad_id.
static __global__ void beam_finish_kernel(const int* __restrict__ tok, int ldt, int rows, int num_steps, int pad_id, const float* __restrict__ score,
                                          const unsigned char* __restrict__ finished, const int* __restrict__ length, const int* __restrict__ picked,
                                          int* __restrict__ tokens_out, float* __restrict__ scores_out, int* __restrict__ lengths_out,
                                          unsigned char* __restrict__ finished_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < rows * num_steps) {
        const int r = i / num_steps, j = i - r * num_steps;
        const bool dead = !(score[r] > -INFINITY);
        tokens_out[i] = dead ? pad_id : (j + 1 < ldt ? tok[(size_t)r * ldt + j + 1] : picked[r]);
    }
    if (i < rows) { scores_out[i] = score[i]; lengths_out[i] = length[i]; finished_out[i] = finished[i]; }
}

}  // namespace pq
