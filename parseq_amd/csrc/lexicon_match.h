// Lexicon matching: the N words of a list nearest to every reading in Levenshtein distance, and the kernel that
// seeds the beam state with them.  All integer arithmetic; the result does not depend on the grid.
//
// The list is a table of 32-byte rows, one per entered word in ascending word id: bytes 0 .. 30 the class ids, byte 31 the length (1 .. 31).
// A thread owns a word and walks a tile of LM_TC crops: the distance is Hyyro's bit-parallel form of Myers' algorithm (myers_step,
// myers.h: the one the evaluation kernels take too) with the READING as the pattern — a reading has at most 32 characters, so its column of the DP fits one 32-bit word — and the word's characters as the text.
// The per-crop pattern masks peq[c][t] (bit i: character i of crop t's reading is class c) live in LDS with the crop index innermost, so
// one 16-byte LDS read gives a word character's masks for the whole tile.
//
// Selection in two steps on keys (distance << 26) | row, which order by (distance, row) = (distance, word id): every wave writes the N
// smallest keys of its 64 words in order (ballots over ascending distance: lanes are rows in order, so a prefix count is the rank), and a
// merge kernel per crop picks the N smallest of all chunks.  No atomics anywhere.
#pragma once
#include <climits>
#include "common.h"
#include "myers.h"

namespace pq {

constexpr int LM_ROW_BYTES = 32;            // a word's row
constexpr int LM_MAX_WORD = 31;             // characters of a word
constexpr int LM_MAX_READING = 32;          // characters of a reading (one bit each)
constexpr int LM_MAX_CLASSES = 256;         // a class id is a byte of the row
constexpr int LM_THREADS = 256;             // four waves: 256 words per workgroup
constexpr int LM_TC = 4;                    // crops per tile: one ds_read_b128 per word character
constexpr int LM_CHUNK = 64;                // words per partial list: a wave
constexpr int LM_KEY_SHIFT = 26;            // rows < 2^26, distances <= 32
constexpr unsigned LM_KEY_DEAD = 0xFFFFFFFFu;
constexpr int LM_DEAD_DISTANCE = 0x7FFFFFFF;      // PARSEQ_LEXICON_MATCH_DEAD: the distance of a slot beyond the list

static inline int lm_chunks(int nrows) { return (nrows + LM_CHUNK - 1) / LM_CHUNK; }

// grid (ceil(nrows / 256), crop groups); a workgroup walks the crops [blockIdx.y * crops_per_block, ...) in tiles of LM_TC.
//   readings [B][ldt] (ldt <= 32), lengths [B] or null; a reading ends before its first <eos> and at its length
//   rows     the table, nrows rows;   ranges [B][2] or null: crop b matches rows [begin, end) only (clipped to the table)
//   fold     [C] or null: the reading's classes go through it (the rows of a folded table already did)
//   partial  [B][chunks][N]: per crop and 64-word chunk the N smallest keys ascending, LM_KEY_DEAD beyond.  With ranges only the chunks
//            a crop's range touches are written (the merge reads no others).
static __global__ __launch_bounds__(LM_THREADS)
void lexicon_match_kernel(const int* __restrict__ readings, int ldt, const int* __restrict__ lengths, int B, const unsigned* __restrict__ rows,
                          int nrows, const int* __restrict__ ranges, const int* __restrict__ fold, int C, int eos_id, int N,
                          unsigned* __restrict__ partial, int chunks, int crops_per_block) {
    __shared__ uint4 s_peq[LM_MAX_CLASSES];                // [c] the masks of the tile's LM_TC crops
    __shared__ int s_rd[LM_TC][LM_MAX_READING];
    __shared__ int s_m[LM_TC], s_lo[LM_TC], s_hi[LM_TC];
    __shared__ int s_any;
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = blockIdx.x * LM_THREADS + tid;
    const int blk_lo = blockIdx.x * LM_THREADS, blk_hi = min(blk_lo + LM_THREADS, nrows);
    const bool have = w < nrows;
    const unsigned* rp = rows + (size_t)(have ? w : 0) * (LM_ROW_BYTES / 4);
    const unsigned last = have ? rp[7] : 0u;
    const int len = have ? min((int)(last >> 24), LM_MAX_WORD) : 0;
    const int chunk = w / LM_CHUNK;      // wave-uniform
    const bool chunk_live = chunk < chunks;
    const int crop_lo = blockIdx.y * crops_per_block, crop_hi = min(crop_lo + crops_per_block, B);

    for (int c0 = crop_lo; c0 < crop_hi; c0 += LM_TC) {
        __syncthreads();      // the previous tile's masks are no longer read
        if (tid < LM_TC * LM_MAX_READING) {
            const int t = tid / LM_MAX_READING, i = tid - t * LM_MAX_READING, crop = c0 + t;
            int v = INT_MIN;      // the end of the reading
            if (crop < crop_hi && i < ldt) {
                const int r = readings[(size_t)crop * ldt + i];
                if (r != eos_id) v = (fold && r >= 0 && r < C) ? fold[r] : r;
            }
            s_rd[t][i] = v;
        }
        if (tid == 0) s_any = 0;
        __syncthreads();
        if (tid < LM_TC) {
            const int crop = c0 + tid;
            int m = 0, lo = 0, hi = 0;
            if (crop < crop_hi) {
                int cap = lengths ? lengths[crop] : ldt;
                cap = cap < 0 ? 0 : (cap > ldt ? ldt : cap);
                while (m < cap && s_rd[tid][m] != INT_MIN) ++m;
                lo = ranges ? max(ranges[2 * crop], 0) : 0;
                hi = ranges ? min(ranges[2 * crop + 1], nrows) : nrows;
                if (lo < blk_hi && hi > blk_lo) s_any = 1;      // (every writer stores the same value)
            }
            s_m[tid] = m; s_lo[tid] = lo; s_hi[tid] = hi;
        }
        __syncthreads();
        if (!s_any) continue;      // no crop of the tile matches a word of this workgroup: nothing to write either
        for (int idx = tid; idx < C * LM_TC; idx += LM_THREADS) {
            const int c = idx / LM_TC, t = idx - c * LM_TC, m = s_m[t];
            unsigned mask = 0;
            for (int i = 0; i < m; ++i) mask |= (s_rd[t][i] == c ? 1u : 0u) << i;
            reinterpret_cast<unsigned*>(s_peq)[idx] = mask;
        }
        __syncthreads();

        int m[LM_TC]; unsigned hb[LM_TC], pv[LM_TC], mv[LM_TC]; int sc[LM_TC];
#pragma unroll
        for (int t = 0; t < LM_TC; ++t) { m[t] = s_m[t]; hb[t] = m[t] > 0 ? 1u << (m[t] - 1) : 0u; pv[t] = ~0u; mv[t] = 0u; sc[t] = m[t]; }
        for (int k = 0; k < LM_ROW_BYTES / 4; ++k) {
            if (!__any(4 * k < len)) break;
            const unsigned dw = k == 7 ? last : (have ? rp[k] : 0u);
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                if (4 * k + i < len) {
                    const unsigned c = (dw >> (8 * i)) & 255u;
                    const uint4 eq = s_peq[c];      // (a class id >= C: the row is not of this charset; its masks are whatever — refused on the host)
                    myers_step(eq.x, hb[0], pv[0], mv[0], sc[0]);
                    myers_step(eq.y, hb[1], pv[1], mv[1], sc[1]);
                    myers_step(eq.z, hb[2], pv[2], mv[2], sc[2]);
                    myers_step(eq.w, hb[3], pv[3], mv[3], sc[3]);
                }
            }
        }

        // per crop: the wave's N smallest keys in order
#pragma unroll
        for (int t = 0; t < LM_TC; ++t) {
            const int crop = c0 + t;
            if (crop >= crop_hi || !chunk_live) continue;      // wave-uniform
            const int lo = s_lo[t], hi = s_hi[t];
            const int ch_lo = chunk * LM_CHUNK;
            if (!(lo < ch_lo + LM_CHUNK && hi > ch_lo)) continue;      // the crop's range does not touch this chunk
            const bool ok = have && w >= lo && w < hi;
            const int dist = m[t] == 0 ? len : sc[t];      // an empty reading: every character is an insertion
            const int d = ok ? dist : 63;
            int dmin = d;
#pragma unroll
            for (int o = 32; o >= 1; o >>= 1) dmin = min(dmin, __shfl_xor(dmin, o, 64));
            unsigned* out = partial + ((size_t)crop * chunks + chunk) * N;
            const unsigned key = ((unsigned)dist << LM_KEY_SHIFT) | (unsigned)w;
            int taken = 0;
            for (int dd = dmin; dd <= LM_MAX_READING && taken < N; ++dd) {
                const unsigned long long mk = __ballot(d == dd);
                if (d == dd) {
                    const int rank = taken + __popcll(mk & ((1ull << lane) - 1ull));
                    if (rank < N) out[rank] = key;
                }
                taken += __popcll(mk);
            }
            if (lane >= taken && lane < N) out[lane] = LM_KEY_DEAD;
        }
    }
}

// One crop per workgroup: the N smallest keys of the crop's chunks, ascending, by N rounds of a block-wide minimum over the keys above the
// previous round's (keys are distinct: each holds its row).  word_ids_out [B][N] = row_ids[row] (the row itself without row_ids),
// distances_out [B][N], rows_out [B][N] (may be null); a slot beyond the list: -1, LM_DEAD_DISTANCE, -1.
static __global__ __launch_bounds__(LM_THREADS)
void lexicon_match_merge_kernel(const unsigned* __restrict__ partial, int chunks, int nrows, const int* __restrict__ ranges, const int* __restrict__ row_ids,
                                int N, int* __restrict__ word_ids_out, int* __restrict__ distances_out, int* __restrict__ rows_out) {
    __shared__ unsigned s_best[LM_THREADS / 64];
    const int crop = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int lo = 0, hi = nrows;
    if (ranges) { lo = max(ranges[2 * crop], 0); hi = min(ranges[2 * crop + 1], nrows); }
    const int c_lo = lo < hi ? lo / LM_CHUNK : 0, c_hi = lo < hi ? (hi - 1) / LM_CHUNK + 1 : 0;
    const unsigned* keys = partial + ((size_t)crop * chunks + c_lo) * N;
    const int nkeys = (c_hi - c_lo) * N;
    unsigned prev = 0; bool first = true;
    for (int r = 0; r < N; ++r) {
        unsigned best = LM_KEY_DEAD;
        if (first || prev != LM_KEY_DEAD) {
            for (int i = tid; i < nkeys; i += LM_THREADS) {
                const unsigned k = keys[i];
                if ((first || k > prev) && k < best) best = k;
            }
        }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, 64));
        __syncthreads();      // the previous round's s_best has been read
        if (lane == 0) s_best[wave] = best;
        __syncthreads();
        best = min(min(s_best[0], s_best[1]), min(s_best[2], s_best[3]));
        if (tid == 0) {
            const bool dead = best == LM_KEY_DEAD;
            const int row = dead ? -1 : (int)(best & ((1u << LM_KEY_SHIFT) - 1u));
            const size_t o = (size_t)crop * N + r;
            word_ids_out[o] = dead ? -1 : (row_ids ? row_ids[row] : row);
            distances_out[o] = dead ? LM_DEAD_DISTANCE : (int)(best >> LM_KEY_SHIFT);
            if (rows_out) rows_out[o] = row;
        }
        prev = best; first = false;
    }
}

// The beam state of a match (section 23): rows = B * W hypotheses, W = N (+ 1 with keep_reading), one thread per (row, position of its
// history).  Slot s of crop b is candidate s of the match, in (distance, id) order; with keep_reading the reading itself comes first (word -1,
// distance 0) when no word has distance 0, and otherwise the last slot is dead.  A live hypothesis: <bos>, its characters, <eos>, pad_id;
// score 0, finished, its length — the reading without an <eos> in its L positions: L characters, unfinished.  The characters of a word are
// its own ids (`rows`, the unfolded table).  A dead slot (beyond the list, or a word of more than L - 1 characters, for which L positions
// have no <eos>): score -inf, length 0, word -1, pad_id.  `dist` [rows] carries the distances (LM_DEAD_DISTANCE for a dead slot).
static __global__ void lexicon_seed_kernel(int B, int N, int keep_reading, int L, const unsigned char* __restrict__ rows, const int* __restrict__ match_rows,
                                           const int* __restrict__ match_ids, const int* __restrict__ match_dist, const int* __restrict__ reading,
                                           const int* __restrict__ reading_len, int bos_id, int eos_id, int pad_id, int* __restrict__ tok, int ldt,
                                           float* __restrict__ score, unsigned char* __restrict__ finished, int* __restrict__ length, int* __restrict__ picked,
                                           int* __restrict__ word, int* __restrict__ dist, float* __restrict__ ar_score) {
    const int W = N + (keep_reading ? 1 : 0);
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)B * W * ldt) return;
    const int r = (int)(i / ldt), j = (int)(i - (size_t)r * ldt);
    const int b = r / W, s = r - b * W;
    const bool reading_live = keep_reading && match_dist[(size_t)b * N] != 0;
    const bool is_reading = reading_live && s == 0;
    const int cand = s - (reading_live ? 1 : 0);      // the match's slot
    int len = 0, wid = -1, d = LM_DEAD_DISTANCE; bool live = false, fin = true;
    const unsigned char* chars = nullptr;
    if (is_reading) {
        len = min(max(reading_len[b], 0), L); live = true; fin = len < L; d = 0;
    } else if (cand < N) {
        const int row = match_rows[(size_t)b * N + cand];
        if (row >= 0) {
            chars = rows + (size_t)row * LM_ROW_BYTES;
            len = min((int)chars[LM_ROW_BYTES - 1], LM_MAX_WORD);
            live = len <= L - 1;
            if (live) { wid = match_ids[(size_t)b * N + cand]; d = match_dist[(size_t)b * N + cand]; }
        }
    }
    // token k of the hypothesis
    const auto token = [&](int k) {
        if (!live) return pad_id;
        if (k < len) return is_reading ? reading[(size_t)b * L + k] : (int)chars[k];
        return (k == len && fin) ? eos_id : pad_id;
    };
    tok[i] = j == 0 ? bos_id : token(j - 1);
    if (j == 0) {
        score[r] = live ? 0.f : -INFINITY;
        finished[r] = live && fin ? 1 : 0;
        length[r] = live ? len : 0;
        picked[r] = token(L - 1);
        word[r] = wid;
        dist[r] = d;
        if (ar_score) ar_score[r] = live ? 0.f : -INFINITY;
    }
}

}  // namespace pq
