// libparseq_hip.so — launch orchestration of the decoder passes, the AR loop, refinement and parseq_forward.
#include "lib_internal.h"
#include "decoder_tile_loop.h"
#include "beam.h"
#include "beam_refine.h"
#include "attn_map.h"
#include "lexicon_match.h"
#include "orient.h"
#include "line_stitch.h"
#include "score.h"

// -------------------------------------------------------------------------------------------------------------------
// what a call runs on: storage type and width, the decoder's parameters, the pass, the route of the single-query step
// -------------------------------------------------------------------------------------------------------------------
// f(TE<T, E>{}) with the plan's storage type (bf16_t, or float for fp32 and bf16x3) and embed_dim as template arguments; dispatch_t
// where only the type matters (E = 0).
template <typename T_, int E_> struct TE { using T = T_; static constexpr int E = E_; };
template <typename F>
static int dispatch_t(const parseq_plan* p, F&& f) { return p->precision == PARSEQ_BF16 ? f(TE<bf16_t, 0>{}) : f(TE<float, 0>{}); }
template <typename F>
static int dispatch_te(const parseq_plan* p, F&& f) {
    return dispatch_t(p, [&](auto t) {
        using T = typename decltype(t)::T;
        switch (p->m->cfg.embed_dim) {
            case 192: return f(TE<T, 192>{});
            case 384: return f(TE<T, 384>{});
            default:  return f(TE<T, 768>{});
        }
    });
}

// The decoder's parameters, resolved once per call (on the stack: the master may be uploaded again between calls): GEMM weights in
// the storage type, everything else fp32 from the master.
struct LnW { const float *g, *b; };
template <typename T> struct DecLayerW {
    LnW norm_q, norm_c, norm1, norm2;
    const T *sa_in, *sa_out, *ca_in, *ca_out, *lin1, *lin2;
    const float *sa_in_b, *sa_out_b, *ca_in_b, *ca_out_b, *lin1_b, *lin2_b;
};
template <typename T> struct DecW {
    DecLayerW<T> layer[PARSEQ_DEC_DEPTH_MAX];
    LnW norm; const T* head; const float* head_b;      // decoder.norm, head
    const float *pos_queries, *text_embed;
};
static std::string dec_layer_key(int l) { return "decoder.layers." + std::to_string(l) + "."; }
// the cross-attention in-projection of the layer with key prefix d (rows 0 .. E: q; rows E .. 3E: k | v of memory) — all that parseq_set_memory reads
template <typename T>
static void ca_in_proj(const Weights<T>& W, const std::string& d, const T*& w, const float*& b) {
    w = W.w(d + "cross_attn.in_proj_weight"); b = W.m->p(d + "cross_attn.in_proj_bias");
}
template <typename T>
static DecW<T> dec_weights(const parseq_plan* p) {
    const parseq_model* m = p->m;
    const Weights<T> W = weights_of<T>(p);
    DecW<T> w{};
    for (int l = 0; l < m->cfg.dec_depth; ++l) {
        const std::string d = dec_layer_key(l);
        DecLayerW<T>& y = w.layer[l];
        y.norm_q = {m->p(d + "norm_q.weight"), m->p(d + "norm_q.bias")}; y.norm_c = {m->p(d + "norm_c.weight"), m->p(d + "norm_c.bias")};
        y.norm1 = {m->p(d + "norm1.weight"), m->p(d + "norm1.bias")}; y.norm2 = {m->p(d + "norm2.weight"), m->p(d + "norm2.bias")};
        y.sa_in = W.w(d + "self_attn.in_proj_weight"); y.sa_in_b = m->p(d + "self_attn.in_proj_bias");
        y.sa_out = W.w(d + "self_attn.out_proj.weight"); y.sa_out_b = m->p(d + "self_attn.out_proj.bias");
        ca_in_proj(W, d, y.ca_in, y.ca_in_b);
        y.ca_out = W.w(d + "cross_attn.out_proj.weight"); y.ca_out_b = m->p(d + "cross_attn.out_proj.bias");
        y.lin1 = W.w(d + "linear1.weight"); y.lin1_b = m->p(d + "linear1.bias");
        y.lin2 = W.w(d + "linear2.weight"); y.lin2_b = m->p(d + "linear2.bias");
    }
    w.norm = {m->p("decoder.norm.weight"), m->p("decoder.norm.bias")};
    w.head = W.w("head.weight"); w.head_b = m->p("head.bias");
    w.pos_queries = m->p("pos_queries"); w.text_embed = m->p("text_embed.embedding.weight");
    return w;
}

// One pass of the decoder (model.decode + head, modules.py:55-124): queries pos_queries[i0 : i0 + Lq] of every image — or the caller's
// `user_query` [B, Lq, E] — against the content tokens p->tok[:, :Lk].  Writes logits[b][i0 + qi][:] for qi < Lq into a [B][Ltot][C] tensor.
struct DecPass {
    int B = 0, Lk = 1, i0 = 0, Lq = 1;
    int c0 = 0;      // dec_depth > 1: the first content row this pass computes (an AR step: Lk - 1, the rows before it are cached in kvself)
    const unsigned char* qmask = nullptr;      // [npos][LDT] attention mask of the query stream, rows by absolute position; True = masked
    const unsigned char* cmask = nullptr;      // the same for the content stream (read at dec_depth > 1 only)
    const unsigned char* kpm = nullptr;        // [B][LDT] key padding of both streams
    float* logits = nullptr; int Ltot = 0;      // null: the pass ends before decoder.norm and the head (the attention map's pass without logits)
    int argmax_mode = 0;      // Lq == 1: greedy pick of position i0 into tok[:, i0 + 1] with the EOS bookkeeping (2: testing, all rows run on)
    const float* user_query = nullptr;
    bool fused_step_allowed = false;      // a single unmasked query may take dec_step_pre / post, which leave no query stream in p->t
    // A pass writes logits[b][i0 + qi] of a [B][Ltot][C] tensor (the forward's layout).  `out` holds the rows of this pass alone,
    // [B][Lq][C] with row qi (a decode entry's output, one beam step's logits): hand over the base shifted back by i0 rows, so that the
    // rows written are exactly [b * Lq + qi] (writing at b * Lq + i0 + qi ran i0 rows past the end of the buffer for i0 > 0).
    void logits_of_pass(float* out, int C) { logits = out - (size_t)i0 * C; Ltot = Lq; }
};

// The form a single-query (AR) step takes, decided once per parseq_forward / parseq_decode_* call:
//   STEP_DEEP    dec_depth > 1: the layer walk with the per-layer content cache (decoder_step.h holds depth-1 kernels)
//   STEP_FUSED   decoder_step.h.  parseq_forward's AR loop: mid / cross-attention / mlp launches, in bf16 or in the bf16x3 arithmetic on
//                f32 storage (ar_loop_fused).  A single unmasked query of any other bf16 pass: the pre / post pair (step_pre_post).
//   STEP_PER_OP  one launch per operation
// p->wstep[0] is set only where the fragment-packed weights exist (step_ok, lib_model.hip parseq_plan_create_ex): a PARSeq model,
// precision bf16 or bf16x3, embed_dim <= 384 and a multiple of 64, dec_mlp_ratio == 4 — none of which is asked again here.  Of the
// widths parseq_model_create admits (192, 384, 768) that leaves 192 and 384, the two the step kernels are built for; forward_impl
// and decoder_pass ask E <= 384 at compile time and keep the per-operation step otherwise.
// The step kernels' head holds up to 128 classes.  `qsplit`: the mid kernel's start half on DS_QS workgroups per row tile, see ar_loop_fused.
// `tile_loop`: the whole AR loop of parseq_forward as one launch in which a workgroup owns 16 images (decoder_tile_loop.h) — batches in
// flight (no PARSEQ_FLAG_LATENCY) of at least p->tile_loop_min images, in the one geometry that kernel is built for: bf16x3, embed_dim 384,
// 128 memory tokens held as 24-bit K / V rows (asked after the encoder has run: p->kv24 is what this call's encoder left).
enum DecStep { STEP_DEEP, STEP_FUSED, STEP_PER_OP };
struct DecRoute { DecStep step; bool qsplit; bool tile_loop; };
static DecRoute dec_route(const parseq_plan* p, bool latency, int batch = 0) {
    const parseq_model* m = p->m;
    if (m->cfg.dec_depth > 1) return {STEP_DEEP, false, false};
    if (!(p->wstep[0] && p->fused_step && m->classes <= 128)) return {STEP_PER_OP, false, false};
    const bool tile_loop = !latency && p->tile_loop && p->precision == PARSEQ_BF16X3 && m->cfg.embed_dim == 384 && m->tokens == 128 && p->kv24 &&
                           batch >= p->tile_loop_min;
    return {STEP_FUSED, latency && p->qsplit && m->tokens == 128 && m->cfg.max_label_length + 1 >= DS_QS + 2, tile_loop};
}

static float dec_scale() { return sqrtf(1.0f / (float)DEC_HD); }

// -------------------------------------------------------------------------------------------------------------------
// decoder
// -------------------------------------------------------------------------------------------------------------------
// Cross-attention of Lq queries per image against cached memory K / V: tuned kernels for 128 memory tokens (streaming AR kernels,
// MFMA multi-query kernels), the key-count-generic kernels otherwise.  `half`: bf16 storage.
enum CaKernel { CA_MFMA_N, CA_GENERIC, CA_AR24, CA_AR, CA_MULTI_MFMA, CA_MULTI_X3, CA_MULTI };
static int ca_route(bool half, int E, int NK, int Lq, bool kv24, int nsplit, CaKernel& kern) {
    if (nsplit && (nsplit != DS_QS || NK != 128 || Lq != 1)) return fail(PARSEQ_E_STATE, "cross-attention: split q-projection outside the AR step kernels");
    if (NK != 128) kern = half && (NK + 15) / 16 <= 16 ? CA_MFMA_N : CA_GENERIC;
    else if (Lq == 1) {
        if (kv24 && (half || E != 384)) return fail(PARSEQ_E_STATE, "cross-attention: 24-bit K / V rows but no kernel for this geometry");
        if (!kv24 && nsplit && E > 384) return fail(PARSEQ_E_STATE, "cross-attention: split q-projection at embed_dim %d", E);      // the split step exists for the fused AR loop's widths only
        kern = kv24 ? CA_AR24 : CA_AR;
    } else if (half) kern = CA_MULTI_MFMA;
    else if (g_split) kern = CA_MULTI_X3;      // bf16x3: the matrix-core kernel on bf16 pairs
    else if (kv24) return fail(PARSEQ_E_STATE, "cross-attention: 24-bit K / V rows outside the bf16x3 mode");
    else kern = CA_MULTI;
    return 0;
}

template <typename T, int E>
static int run_cross_attention(parseq_plan* p, hipStream_t s, int layer, int B, int Lq, T* ca, const QAsm& qa) {
    const int H = p->m->cfg.dec_heads, NK = p->m->tokens;
    // decoder layer `layer`'s K / V of memory (layers >= 1: dec_depth > 1, f32 / bf16 rows of the generic GEMM, never 24-bit)
    const T* kmem = reinterpret_cast<const T*>(layer ? p->kmem_l[layer] : p->kmem); const T* vmem = reinterpret_cast<const T*>(layer ? p->vmem_l[layer] : p->vmem);
    const bool kv24 = layer ? false : p->kv24;      // the 24-bit rows come from the one-launch bf16x3 encoder's tail
    const float* qc_ = p->qc;
    const float scale = dec_scale();
    constexpr bool half = sizeof(T) == 2;
    CaKernel kern;
    CHK(ca_route(half, E, NK, Lq, kv24, qa.nsplit, kern));
    // ca_route never picks a kernel that T, E or NK lacks; the `if constexpr` below only keep each kernel from being compiled for
    // a type or width it does not exist for, and their other arms (unreachable) report instead of returning without a launch
    const auto no_kernel = [&] { return fail(PARSEQ_E_STATE, "cross-attention: route %d has no kernel for this storage type, width or key count", (int)kern); };
    ProfScope ps_(&p->prof, T_DEC_CA, s);
    switch (kern) {
        case CA_MFMA_N:
            if constexpr (half) {
                const int nt16 = (NK + 15) / 16;
#define PQ_CAM_N(NT)                                                                                                                      \
                if (nt16 > NT - 2 && nt16 <= NT) {                                                                                       \
                    static LdsAttr attr_;                                                                                                \
                    HIPCHK(attr_.ensure(reinterpret_cast<const void*>(dec_cross_attn_mfma_n_kernel<NT>), dec_cross_attn_mfma_n_lds<NT>())); \
                    hipLaunchKernelGGL((dec_cross_attn_mfma_n_kernel<NT>), dim3((B * H + 1) / 2), dim3(128), dec_cross_attn_mfma_n_lds<NT>(), s, \
                                       qc_, kmem, vmem, H, Lq, NK, scale, ca, B * H);                                                  \
                } else
                PQ_CAM_N(2) PQ_CAM_N(4) PQ_CAM_N(6) PQ_CAM_N(8) PQ_CAM_N(10) PQ_CAM_N(12) PQ_CAM_N(14) PQ_CAM_N(16) return no_kernel();
#undef PQ_CAM_N
            } else return no_kernel();
            break;
        case CA_GENERIC: {
            const size_t lds = dec_cross_attn_generic_lds(NK);
            HIPCHK(hipFuncSetAttribute(reinterpret_cast<const void*>(dec_cross_attn_generic_kernel<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL((dec_cross_attn_generic_kernel<T>), dim3(B * H), dim3(128), lds, s, qc_, kmem, vmem, H, Lq, NK, scale, ca);
            break;
        }
        case CA_AR24:
            if constexpr (!half && E == 384) {
                const auto k = qa.nsplit ? dec_cross_attn_ar24_kernel<E, true> : dec_cross_attn_ar24_kernel<E, false>;
                return launch(k, dim3(B), dim3(E), 0, s, qc_, qa, reinterpret_cast<const unsigned char*>(p->kmem),
                              reinterpret_cast<const unsigned char*>(p->vmem), p->kv_plane_elems, scale, ca);
            } else return no_kernel();
        case CA_AR: {
            auto k = dec_cross_attn_ar_kernel<T, E, false>;
            if constexpr (E <= 384) { if (qa.nsplit) k = dec_cross_attn_ar_kernel<T, E, true>; }
            return launch(k, dim3(B), dim3(E), 0, s, qc_, qa, kmem, vmem, scale, ca);
        }
        case CA_MULTI_MFMA:
            if constexpr (half) return launch(dec_cross_attn_multi_mfma_kernel, dim3((B * H + 3) / 4), dim3(256), 0, s, qc_, kmem, vmem, H, Lq, scale, ca, B * H);
            else return no_kernel();
        case CA_MULTI_X3:      // K / V from the 24-bit rows, or from f32 rows
            if constexpr (half) return no_kernel();
            else if (kv24) return launch(dec_cross_attn_multi_mfma_x3_kernel<true>, dim3((B * H + 1) / 2), dim3(128), 0, s, qc_, kmem, vmem, H, Lq, scale, ca, B * H, p->kv_plane_elems);
            else return launch(dec_cross_attn_multi_mfma_x3_kernel<false>, dim3((B * H + 1) / 2), dim3(128), 0, s, qc_, kmem, vmem, H, Lq, scale, ca, B * H, (size_t)0);
        case CA_MULTI:
            if constexpr (half) return no_kernel();
            else return launch(dec_cross_attn_multi_kernel<T>, dim3(B * H), dim3(128), 0, s, qc_, kmem, vmem, H, Lq, scale, ca);
    }
    HIPCHK(hipGetLastError());      // of the two routes above that set their own dynamic-LDS attribute
    return 0;
}

// decoder.norm + head of the query stream in p->t (rows b * Lq + qi -> logits[b][i0 + qi]), and for an AR step (argmax_mode != 0)
// the greedy pick of position i0 into tok[:, i0 + 1] with the EOS bookkeeping
template <typename T, int E>
static int head_pass(parseq_plan* p, hipStream_t s, const DecW<T>& w, const DecPass& a) {
    const parseq_config& c = p->m->cfg;
    const int M = a.B * a.Lq, C = p->m->classes;
    // decoder.norm fused into the head's A operand
    { ProfScope ps_(&p->prof, T_DEC_GEMM, s); CHK((run_ln_gemm<T, E>(s, p->t, w.norm.g, w.norm.b, c.dec_ln_eps, w.head, M, C,
                     epi_store<float>(M, C, w.head_b, a.logits, C, 1.f, a.Lq, a.Ltot, a.i0), p->tn))); }
    if (a.argmax_mode) CHK(launch(ar_argmax_kernel, dim3((a.B + 3) / 4), dim3(256), 0, s, a.logits, a.Ltot, C, p->tok, LDT, a.i0, a.B, c.eos_id,
                                  p->eos_seen, p->counters, p->counters + 1, a.argmax_mode == 2 ? 1 : 0));
    return 0;
}

// A whole depth-1 pass of one unmasked query per image (bf16): two fused row-block kernels around the cross-attention
// (decoder_step.h), head and greedy pick included.
template <int E>
static int step_pre_post(parseq_plan* p, hipStream_t s, const DecW<bf16_t>& w, const DecPass& a) {
    const parseq_config& c = p->m->cfg;
    const DecLayerW<bf16_t>& y = w.layer[0];
    const int M = a.B, C = p->m->classes, npos = c.max_label_length + 1;
    bf16_t* ca = reinterpret_cast<bf16_t*>(p->ca);
    const dim3 grid((M + DS_ROWS - 1) / DS_ROWS), block(64 * DS_NW);
    static LdsAttr attr_pre, attr_post;
    HIPCHK(attr_pre.ensure(reinterpret_cast<const void*>(dec_step_pre_kernel<E>), dec_step_pre_lds<E>()));
    HIPCHK(attr_post.ensure(reinterpret_cast<const void*>(dec_step_post_kernel<E>), dec_step_post_lds<E>()));
    {
        ProfScope ps_(&p->prof, T_DEC_PRE, s);
        hipLaunchKernelGGL((dec_step_pre_kernel<E>), grid, block, dec_step_pre_lds<E>(), s, p->stab, reinterpret_cast<const bf16_t*>(p->kvtab),
                           p->tok, LDT, c.num_tokens, npos, a.Lk, a.i0, p->wstep[0], y.sa_out_b, w.pos_queries + (size_t)a.i0 * E, y.norm1.g, y.norm1.b,
                           c.dec_ln_eps, p->wstep[1], y.ca_in_b, p->t, p->qc, M);
        HIPCHK(hipGetLastError());
    }
    CHK((run_cross_attention<bf16_t, E>(p, s, 0, a.B, 1, ca, QAsm{})));
    {
        ProfScope ps_(&p->prof, T_DEC_POST, s);
        hipLaunchKernelGGL((dec_step_post_kernel<E>), grid, block, dec_step_post_lds<E>(), s, ca, p->t, p->wstep[2], y.ca_out_b, y.norm2.g, y.norm2.b,
                           p->wstep[3], y.lin1_b, p->wstep[4], y.lin2_b, w.norm.g, w.norm.b, c.dec_ln_eps, p->wstep[5], w.head_b, C, a.logits, a.Ltot,
                           a.i0, M, a.argmax_mode, p->tok, LDT, c.eos_id, p->eos_seen, p->counters, p->counters + 1);
        HIPCHK(hipGetLastError());
    }
    return 0;
}

// The table self-attention launch of <T, E>: a wave per row up to 512 columns in bf16 and (on the f32 tables) in bf16x3; a thread per
// column otherwise (fp32, embed_dim 768).
template <typename T, int E>
static int launch_self_attn_tables(parseq_plan* p, hipStream_t s, const DecPass& a, T* sa) {
    const parseq_config& c = p->m->cfg;
    const int M = a.B * a.Lq, npos = c.max_label_length + 1;
    const T* kvtab = reinterpret_cast<const T*>(p->kvtab);
    if constexpr (E <= 512) {
        if (sizeof(T) == 2 || g_split) {
            return launch(dec_self_attn_wave_kernel<E, T>, dim3((M + 3) / 4), dim3(256), 0, s, p->stab, kvtab, p->tok, LDT, c.num_tokens, npos,
                          a.qmask, LDT, a.kpm, LDT, a.Lk, a.i0, a.Lq, sa, M);
        }
    }
    return launch(dec_self_attn_kernel<T, E>, dim3(M), dim3(E), 0, s, p->stab, kvtab, p->tok, LDT, c.num_tokens, npos,
                  a.qmask, LDT, a.kpm, LDT, a.Lk, a.i0, a.Lq, sa, (const float*)nullptr);
}

// Layer 0's self-attention of the position queries, read from the tables (the keys are embeddings: a function of position and token id),
// out-projection, residual onto the raw position queries -> p->t.
template <typename T, int E>
static int self_attn_tables(parseq_plan* p, hipStream_t s, const DecW<T>& w, const DecPass& a) {
    const int M = a.B * a.Lq;
    T* sa = reinterpret_cast<T*>(p->sa);
    {
        ProfScope ps_(&p->prof, T_DEC_SA, s);
        CHK((launch_self_attn_tables<T, E>(p, s, a, sa)));
    }
    ProfScope ps_(&p->prof, T_DEC_GEMM, s);
    return run_gemm<T>(s, ARowMajor<T>{sa, E}, w.layer[0].sa_out, E, M, E, E, epi_table(M, E, w.layer[0].sa_out_b, p->t, E, w.pos_queries, E, a.Lq, a.i0));
}

// Self-attention of explicit queries (DecoderLayer.forward_stream, modules.py:55-65): x = xq + out_proj(attention(q_proj(norm(xq)))) over
// the M = B * Lq rows of the pass, norm_c for the content stream and norm_q for the query stream, keys j < Lk.  The keys are the K | V
// rows of the layer's content input (`kvself`, dec_depth > 1), or, without them, the content-key table: layer 0 with a caller's query
// (model.py:100-102), whose residual lands on the caller's query itself.
template <typename T, int E>
static int self_attn_queries(parseq_plan* p, hipStream_t s, const DecLayerW<T>& y, const DecPass& a, bool content, const void* kvself, const float* xq, float* x) {
    const parseq_config& c = p->m->cfg;
    const int M = a.B * a.Lq, npos = c.max_label_length + 1;
    const LnW& n = content ? y.norm_c : y.norm_q;
    T* sa = reinterpret_cast<T*>(p->sa);
    { ProfScope ps_(&p->prof, T_DEC_GEMM, s); CHK((run_ln_gemm<T, E>(s, xq, n.g, n.b, c.dec_ln_eps, y.sa_in, M, E,
                     epi_store<float>(M, E, y.sa_in_b, p->qc, E, dec_scale()), p->tn))); }
    {
        ProfScope ps_(&p->prof, T_DEC_SA, s);
        if (kvself) CHK(launch(dec_self_attn_kv_kernel<T, E>, dim3(M), dim3(E), 0, s, p->qc, reinterpret_cast<const T*>(kvself), npos,
                               a.qmask, LDT, a.kpm, LDT, a.Lk, a.i0, a.Lq, sa));
        else CHK(launch(dec_self_attn_kernel<T, E>, dim3(M), dim3(E), 0, s, p->stab, reinterpret_cast<const T*>(p->kvtab), p->tok, LDT,
                        c.num_tokens, npos, a.qmask, LDT, a.kpm, LDT, a.Lk, a.i0, a.Lq, sa, p->qc));
    }
    if (xq != x) HIPCHK(hipMemcpyAsync(x, xq, (size_t)M * E * sizeof(float), hipMemcpyDeviceToDevice, s));
    ProfScope ps_(&p->prof, T_DEC_GEMM, s);
    return run_gemm<T>(s, ARowMajor<T>{sa, E}, y.sa_out, E, M, E, E, epi_resid(M, E, y.sa_out_b, x, E));
}

// The rest of a stream of layer `l` (modules.py:66-76) over the M = B * Lq rows of x [M][E] f32, in place: cross-attention against the
// layer's memory K / V (head-split, cached in the plan; norm1 rides in the q-projection's A operand), MLP (norm2 in linear1's).
template <typename T, int E>
static int cross_mlp(parseq_plan* p, hipStream_t s, const DecLayerW<T>& y, int l, int B, int Lq, float* x) {
    const parseq_config& c = p->m->cfg;
    const int M = B * Lq, Fd = E * c.dec_mlp_ratio;
    T* ca = reinterpret_cast<T*>(p->ca); T* hdn = reinterpret_cast<T*>(p->hdn);
    { ProfScope ps_(&p->prof, T_DEC_GEMM, s); CHK((run_ln_gemm<T, E>(s, x, y.norm1.g, y.norm1.b, c.dec_ln_eps, y.ca_in, M, E,
                     epi_store<float>(M, E, y.ca_in_b, p->qc, E), p->tn))); }
    CHK((run_cross_attention<T, E>(p, s, l, B, Lq, ca, QAsm{})));
    { ProfScope ps_(&p->prof, T_DEC_GEMM, s); CHK((run_gemm<T>(s, ARowMajor<T>{ca, E}, y.ca_out, E, M, E, E, epi_resid(M, E, y.ca_out_b, x, E)))); }
    { ProfScope ps_(&p->prof, T_DEC_GEMM, s); CHK((run_ln_gemm<T, E>(s, x, y.norm2.g, y.norm2.b, c.dec_ln_eps, y.lin1, M, Fd,
                     epi_gelu<T>(M, Fd, y.lin1_b, hdn, Fd), p->tn))); }
    ProfScope ps_(&p->prof, T_DEC_GEMM, s);
    return run_gemm<T>(s, ARowMajor<T>{hdn, Fd}, y.lin2, Fd, M, E, Fd, epi_resid(M, E, y.lin2_b, x, E));
}

// -------------------------------------------------------------------------------------------------------------------
// the layer loop (modules.py:116-124)
// -------------------------------------------------------------------------------------------------------------------
// dec_depth > 1: layers 0 .. D-2 update the content stream (under the content mask), and layers 1 .. D-1 attend to that updated content,
// so from layer 1 on nothing is a function of (position, token id) and the tables do not apply.  The plan holds the content stream
// p->xc (f32, updated in place layer by layer) and, per layer l, the self-attention K | V rows of layer l's content input,
// p->kvself[l][b][pos][2E] (T).  Layer 0's query stream keeps the table-driven kernels.

// The content input of model.decode (model.py:95-97) for positions i0 .. i0 + Lc - 1 of every image into p->xc [B * Lc][E].
template <int E>
static int content_rows(parseq_plan* p, hipStream_t s, const float* text_embed, const float* pos_queries, int B, int Lc, int i0) {
    const size_t n = (size_t)B * Lc * E;
    return launch(content_embed_kernel<E>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, text_embed, pos_queries, p->tok, LDT, B, Lc, i0, p->xc);
}

// K | V of norm_c(xc) for layer l's self-attention (modules.py:115, 64): row r of p->xc [M][E] is image r / period at position
// offset + r % period, written to p->kvself[l][image][position][2E].
template <typename T, int E>
static int kv_rows(parseq_plan* p, hipStream_t s, const DecLayerW<T>& y, int l, int M, int period, int offset) {
    const parseq_config& c = p->m->cfg;
    ProfScope ps_(&p->prof, T_DEC_GEMM, s);
    return run_ln_gemm<T, E>(s, p->xc, y.norm_c.g, y.norm_c.b, c.dec_ln_eps, y.sa_in + (size_t)E * E, M, 2 * E,
                             epi_store<T>(M, 2 * E, y.sa_in_b + E, reinterpret_cast<T*>(p->kvself[l]), 2 * E, 1.f, period, c.max_label_length + 1, offset), p->tn);
}

// One pass (DecPass) through every layer, then decoder.norm and head.  At depth 1 that is the query stream of layer 0 alone.
// Deeper, the content stream runs beside it: rows c0 .. Lk-1 of every image under `cmask`.  A whole context (NAR, refinement, the
// decode entry points) has c0 = 0.  An AR step i (model.py:123-141) has c0 = i = Lk - 1: the AR loop's content mask is causal
// (tgt_mask[:j, :j]), so the content rows of positions < i are those of the previous steps; only row i is computed per layer — its
// K | V appended to kvself[l][:, i], its update carried to the next layer in xc [B][E] — and the query of position i runs through every
// layer: 3 D + 1 row-block passes per step (content row of layers 0 .. D-2, query of layers 0 .. D-1, K | V rows of every layer), no host sync.
template <typename T, int E>
static int decoder_pass(parseq_plan* p, hipStream_t s, const DecW<T>& w, const DecPass& a) {
    const int D = p->m->cfg.dec_depth;
    if constexpr (sizeof(T) == 2 && E <= 384) {
        if (a.fused_step_allowed && a.Lq == 1 && !a.qmask && !a.kpm && !a.user_query) return step_pre_post<E>(p, s, w, a);
    }
    DecPass cs = a; cs.i0 = a.c0; cs.Lq = a.Lk - a.c0; cs.qmask = a.cmask;      // the content stream's rows
    if (D > 1) CHK(content_rows<E>(p, s, w.text_embed, w.pos_queries, a.B, cs.Lq, cs.i0));
    for (int l = 0; l < D; ++l) {
        const DecLayerW<T>& y = w.layer[l];
        if (D > 1) CHK((kv_rows<T, E>(p, s, y, l, a.B * cs.Lq, cs.Lq, cs.i0)));      // K | V rows before the content update reads and overwrites xc
        if (l < D - 1) {
            CHK((self_attn_queries<T, E>(p, s, y, cs, true, p->kvself[l], p->xc, p->xc)));
            CHK((cross_mlp<T, E>(p, s, y, l, a.B, cs.Lq, p->xc)));
        }
        if (l > 0) CHK((self_attn_queries<T, E>(p, s, y, a, false, p->kvself[l], p->t, p->t)));
        else if (a.user_query) CHK((self_attn_queries<T, E>(p, s, y, a, false, nullptr, a.user_query, p->t)));
        else CHK((self_attn_tables<T, E>(p, s, w, a)));
        CHK((cross_mlp<T, E>(p, s, y, l, a.B, a.Lq, p->t)));
    }
    if (!a.logits) return 0;
    return head_pass<T, E>(p, s, w, a);
}

// The whole AR loop with the mid / cross-attention / mlp arrangement of decoder_step.h (bf16 or, X3, the bf16x3 arithmetic on f32
// storage; E <= 384): step i's logits are produced by the mid kernel of step i + 1 (and by one trailing finish-only launch after
// the last step).
template <int E, bool X3, typename TS = typename std::conditional<X3, float, bf16_t>::type>      // TS: storage type of kvtab, the memory K / V and ca
static int ar_loop_fused(parseq_plan* p, hipStream_t s, const DecW<TS>& w, int B, int num_steps, float* logits, bool testing, bool qsplit) {
    const parseq_config& c = p->m->cfg;
    const DecLayerW<TS>& y = w.layer[0];
    const int M = B, C = p->m->classes, npos = c.max_label_length + 1;
    int* eos_rows = p->counters; int* ar_len = p->counters + 1;
    TS* ca = reinterpret_cast<TS*>(p->ca);
    float* partial = reinterpret_cast<float*>(p->hdn);                    // linear2 partial sums [ds_split][M][E] f32 (the generic path's MLP hidden buffer is idle here)
    float* tq = p->qc;                                                    // t' lives in the q-projection buffer once the cross-attention has consumed it
    float* t = p->t;
    const dim3 grid((M + DS_ROWS - 1) / DS_ROWS), block(64 * DS_NW);
    static LdsAttr attr_mid, attr_midq, attr_mlp;
    HIPCHK(attr_mid.ensure(reinterpret_cast<const void*>(dec_step_mid_kernel<E, X3>), dec_step_mid_lds<E, X3>()));
    HIPCHK(attr_midq.ensure(reinterpret_cast<const void*>(dec_step_mid_kernel<E, X3, DS_QS>), dec_step_mid_lds<E, X3>()));
    HIPCHK(attr_mlp.ensure(reinterpret_cast<const void*>(dec_step_mlp_kernel<E, X3>), dec_step_mlp_lds<E, X3>()));
    // qsplit (dec_route): the start half of the mid kernel split over DS_QS workgroups per row tile (decoder_step.h): the q-projection arrives at the
    // cross-attention as partial sums behind t' in the q buffer ([M][E] t' | [DS_QS][M][E] partials | [DS_QS][M][2] column sums; the buffer
    // holds npos rows per image).  Only the two AR cross-attention kernels know how to read that (128 memory tokens).
    // Taken when the caller says this forward is alone on the device (PARSEQ_FLAG_LATENCY): the wider step is a shorter chain but costs
    // about twice the compute-unit time, which batches in flight on other streams would rather have (profiles/r04_ar_step_timers.md).
    float* qp = tq + (size_t)M * E;
    float* qstats = qp + (size_t)DS_QS * M * E;
    QAsm qa;
    if (qsplit) { qa.qp = qp; qa.stats = qstats; qa.cq = p->qfold + E; qa.bq2 = p->qfold + 2 * E; qa.nsplit = DS_QS; qa.M = M; qa.inv_e = 1.0f / (float)E; qa.eps = c.dec_ln_eps; }
    for (int i = 0; i <= num_steps; ++i) {
        const int do_finish = i > 0, do_start = i < num_steps;
        // the pick of position i - 1 feeds step i: needed while there is a step to start
        const int argmax_mode = do_start ? (testing ? 2 : 1) : 0;
        {
            ProfScope ps_(&p->prof, T_DEC_PRE, s);
            const auto mid = qsplit ? dec_step_mid_kernel<E, X3, DS_QS> : dec_step_mid_kernel<E, X3, 1>;
            hipLaunchKernelGGL(mid, dim3(grid.x * (qsplit ? DS_QS : 1)), block, (dec_step_mid_lds<E, X3>()), s, do_finish, do_start, i, M,
                               tq, partial, y.lin2_b, w.norm.g, w.norm.b, c.dec_ln_eps, p->wstep[5], w.head_b, C, logits, num_steps, argmax_mode,
                               c.eos_id, p->eos_seen, eos_rows, ar_len, p->stab, reinterpret_cast<const TS*>(p->kvtab), p->tok, LDT, c.num_tokens, npos,
                               p->wstep[0], y.sa_out_b, w.pos_queries, y.norm1.g, y.norm1.b, p->wstep[1], y.ca_in_b, t, qsplit ? qp : tq, p->qfold, qstats);
            HIPCHK(hipGetLastError());
        }
        if (!do_start) break;
        CHK((run_cross_attention<TS, E>(p, s, 0, B, 1, ca, qa)));
        {
            ProfScope ps_(&p->prof, T_DEC_POST, s);
            hipLaunchKernelGGL((dec_step_mlp_kernel<E, X3>), dim3(grid.x * ds_split<E>()), block, (dec_step_mlp_lds<E, X3>()), s, ca, t, p->wstep[2],
                               y.ca_out_b, y.norm2.g, y.norm2.b, c.dec_ln_eps, p->wstep[3], y.lin1_b, p->wstep[4], tq, partial, M);
            HIPCHK(hipGetLastError());
        }
    }
    return 0;
}

// The whole AR loop as one launch of decoder_tile_loop.h (dec_route: tile_loop): logits, p->tok and the EOS bookkeeping as ar_loop_fused leaves them,
// bit for bit.
template <int E>
static int ar_tile_loop(parseq_plan* p, hipStream_t s, const DecW<float>& w, int B, int num_steps, float* logits, bool testing) {
    const parseq_config& c = p->m->cfg;
    const DecLayerW<float>& y = w.layer[0];
    ArTileArgs a{};
    a.M = B; a.num_steps = num_steps; a.C = p->m->classes; a.testing = testing ? 1 : 0; a.eos_id = c.eos_id; a.ldt = LDT; a.ntok = c.num_tokens;
    a.npos = c.max_label_length + 1; a.eps = c.dec_ln_eps; a.scale = dec_scale();
    a.b2 = y.lin2_b; a.lnf_w = w.norm.g; a.lnf_b = w.norm.b; a.bh = w.head_b; a.Wh = p->wstep[5];
    a.logits = logits; a.eos_seen = p->eos_seen; a.eos_rows = p->counters; a.ar_len = p->counters + 1; a.ar_last = p->counters + 2;
    a.stab = p->stab; a.kvtab = reinterpret_cast<const float*>(p->kvtab); a.tok = p->tok;
    a.Wo = p->wstep[0]; a.Wq = p->wstep[1]; a.bo = y.sa_out_b; a.pos_queries = w.pos_queries; a.ln1_w = y.norm1.g; a.ln1_b = y.norm1.b; a.bq = y.ca_in_b;
    a.kmem = reinterpret_cast<const unsigned char*>(p->kmem); a.vmem = reinterpret_cast<const unsigned char*>(p->vmem); a.plane_elems = p->kv_plane_elems;
    a.Wco = p->wstep[2]; a.W1 = p->wstep[3]; a.W2 = p->wstep[4]; a.bco = y.ca_out_b; a.ln2_w = y.norm2.g; a.ln2_b = y.norm2.b; a.b1 = y.lin1_b;
    static LdsAttr attr_;
    HIPCHK(attr_.ensure(reinterpret_cast<const void*>(dec_ar_tile_loop_kernel<E, true>), dec_ar_tile_loop_lds<E>()));
    ProfScope ps_(&p->prof, T_DEC_LOOP, s);
    hipLaunchKernelGGL((dec_ar_tile_loop_kernel<E, true>), dim3((B + DS_ROWS - 1) / DS_ROWS), dim3(64 * DS_NW), dec_ar_tile_loop_lds<E>(), s, a);
    HIPCHK(hipGetLastError());
    return 0;
}

// The cloze pass of a refinement iteration (model.py:154-167) over rows x L positions: every position queried against the whole content
// in p->tok under the cloze mask, key padding in p->kpm.  `logits` [rows][L][C], or null for the attention map's pass (DecPass::logits).
// dec_depth > 1: the content stream runs under the same cloze-edited mask (model.py:117, 157: tgt_mask and query_mask are one tensor) over
// all L positions, those past a row's first EOS key-padded.  After an AR early exit at a length < L that is the reference with
// tgt_mask[:length, :length] (it raises there: an [L, L] mask against `length` content tokens)
static DecPass cloze_pass(const parseq_plan* p, int rows, int L, float* logits) {
    DecPass a; a.B = rows; a.Lk = a.Lq = L; a.qmask = a.cmask = p->cloze; a.kpm = p->kpm; a.logits = logits; a.Ltot = L;
    return a;
}

// The content and key padding of a refinement iteration from `logits` [rows][L][C]: tok[:, 0] = <bos>, tok[:, 1:] the arg-max of
// positions 0 .. L-2 (from_logits 0: tok[:, 1:] already holds them), keys past a row's first EOS padded.
static int refine_prep(parseq_plan* p, hipStream_t s, int rows, int L, const float* logits, int from_logits) {
    const parseq_config& c = p->m->cfg;
    return launch(refine_prep_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, L, p->m->classes, p->tok, LDT, p->kpm, LDT, rows, c.bos_id, c.eos_id, from_logits);
}

// One refinement iteration: logits [rows][L][C] -> their refinement, in place.
template <typename T, int E>
static int refine_iteration(parseq_plan* p, hipStream_t s, const DecW<T>& w, int rows, int L, float* logits, int from_logits) {
    CHK(refine_prep(p, s, rows, L, logits, from_logits));
    return decoder_pass<T, E>(p, s, w, cloze_pass(p, rows, L, logits));
}

template <typename T, int E>
static int forward_impl(parseq_plan* p, int B, int flags, int refine_iters, int num_steps, float* logits, int* out_len, hipStream_t s) {
    const parseq_config& c = p->m->cfg;
    const bool ar = flags & PARSEQ_FLAG_DECODE_AR, testing = flags & PARSEQ_FLAG_TESTING;
    const DecW<T> w = dec_weights<T>(p);
    const DecRoute route = dec_route(p, flags & PARSEQ_FLAG_LATENCY, B);
    DecPass a; a.B = B; a.logits = logits; a.Ltot = num_steps; a.fused_step_allowed = route.step == STEP_FUSED;
    CHK(launch(ar_init_kernel, dim3((B * LDT + 255) / 256), dim3(256), 0, s, p->tok, LDT, B, c.bos_id, c.pad_id, p->eos_seen, p->counters, 3, num_steps));
    // model.py:119-147.  All num_steps steps are always run (no per-step host sync); the step at which the reference
    // would have stopped is recorded on the device and only truncates the returned view.
    bool stepwise = ar;      // one decoder_pass per AR step, unless the fused loop runs them all
    if constexpr (E <= 384) {
        if (ar && route.step == STEP_FUSED) {
            bool looped = false;
            if constexpr (E == 384 && sizeof(T) == 4) {
                if (route.tile_loop) { CHK((ar_tile_loop<E>(p, s, w, B, num_steps, logits, testing))); looped = true; }
            }
            if (!looped) CHK((ar_loop_fused<E, sizeof(T) == 4>(p, s, w, B, num_steps, logits, testing, route.qsplit)));
            stepwise = false;
        }
    }
    for (int i = 0; stepwise && i < num_steps; ++i) {
        // greedy pick of position i into tok[:, i + 1] (+ EOS bookkeeping) rides on the step; the last step needs none
        a.Lk = i + 1; a.i0 = a.c0 = i; a.Lq = 1; a.argmax_mode = i + 1 < num_steps ? (testing ? 2 : 1) : 0;
        CHK((decoder_pass<T, E>(p, s, w, a)));
    }
    if (!ar) {
        // model.py:148-152: context is <bos> only, all positions queried at once
        a.Lk = 1; a.Lq = num_steps;
        CHK((decoder_pass<T, E>(p, s, w, a)));
    }
    for (int it = 0; it < refine_iters; ++it) {
        // the first refinement after an AR decode: tok[:, 1:] already holds the greedy picks of positions 0 .. L-2 (the loop computed
        // them from these very logits), so the 95-wide arg-max scan per position (30 us of strided reads at batch 512) is skipped
        CHK((refine_iteration<T, E>(p, s, w, B, num_steps, logits, (ar && it == 0) ? 0 : 1)));
    }
    int L = num_steps;
    if (ar && testing && refine_iters == 0) {
        // the reference stops after the first step at which EVERY row holds an EOS: the device recorded that step (num_steps if it
        // never happened)
        int cnt[2];
        HIPCHK(hipMemcpyAsync(cnt, p->counters, sizeof(cnt), hipMemcpyDeviceToHost, s));
        HIPCHK(hipStreamSynchronize(s));
        L = cnt[1];
    }
    if (out_len) *out_len = L;
    return 0;
}

// ViTSTR: strhub/models/vitstr/system.py:76-82 + vitstr/model.py:20-28.
extern "C" int parseq_vitstr_forward(parseq_plan* p, const void* images, int images_dtype, int batch, int num_steps, float* logits_out,
                                     void* stream) {
    CHK(check_call(p, batch, images_dtype));
    if (!p->m->vitstr) return fail(PARSEQ_E_INVALID, "parseq_vitstr_forward on a PARSeq model (arch 0)");
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    if (!images || !logits_out) return fail(PARSEQ_E_INVALID, "null images / logits_out");
    const parseq_model* m = p->m;
    const int npos = m->cfg.max_label_length + 1, N = m->tokens, C = m->classes, E = m->cfg.embed_dim;
    if (num_steps < 1 || num_steps > npos) return fail(PARSEQ_E_INVALID, "num_steps %d outside [1, %d]", num_steps, npos);
    hipStream_t s = (hipStream_t)stream;
    CHK(encode_dispatch(p, images, images_dtype, batch, nullptr, s));
    // model.forward(images, seqlen = num_steps + 1): head over the first seqlen tokens, then [:, 1:] drops the class-token position.
    // The head runs over every token row of the batch (one plain GEMM on the normalised features); the wanted rows are sliced out.
    float* all = reinterpret_cast<float*>(p->h);           // [batch * N][C] scratch (the MLP hidden buffer is idle here)
    const int M = batch * N;
    CHK(dispatch_t(p, [&](auto te) {
        using T = typename decltype(te)::T;
        return run_gemm<T>(s, ARowMajor<T>{reinterpret_cast<const T*>(p->xn), E}, weights_of<T>(p).w("head.weight"), E, M, C, E, epi_store<float>(M, C, m->p("head.bias"), all, C));
    }));
    HIPCHK(hipMemcpy2DAsync(logits_out, (size_t)num_steps * C * sizeof(float), all + (size_t)C, (size_t)N * C * sizeof(float),
                            (size_t)num_steps * C * sizeof(float), batch, hipMemcpyDeviceToDevice, s));
    return 0;
}

extern "C" int parseq_forward(parseq_plan* p, const void* images, int images_dtype, int batch, int flags, int refine_iters,
                              int num_steps, float* logits_out, int* out_len, void* stream) {
    CHK(check_call(p, batch, images_dtype));
    if (p->m->vitstr) return fail(PARSEQ_E_INVALID, "parseq_forward on a ViTSTR model: use parseq_vitstr_forward");
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    if (!images || !logits_out) return fail(PARSEQ_E_INVALID, "null images / logits_out");
    const int npos = p->m->cfg.max_label_length + 1;
    if (num_steps < 1 || num_steps > npos) return fail(PARSEQ_E_INVALID, "num_steps %d outside [1, %d]", num_steps, npos);
    if (refine_iters < 0) return fail(PARSEQ_E_INVALID, "refine_iters %d", refine_iters);
    hipStream_t s = (hipStream_t)stream;
    CHK(encode_dispatch(p, images, images_dtype, batch, nullptr, s));
    // (A decoder stream of its own with hipStreamCreateWithPriority(greatest), forked and joined by events, was measured and removed:
    // 121 -> 108 k img/s with two forwards in flight, 107 -> 58 k one at a time — profiles/r03_decoder_priority_stream_ab.md.)
    return dispatch_te(p, [&](auto te) { return forward_impl<typename decltype(te)::T, decltype(te)::E>(p, batch, flags, refine_iters, num_steps, logits_out, out_len, s); });
}

// A caller's context into the plan's pitched arrays: tokens [batch][ctx_len] -> p->tok (ids clamped to the embedding table), and the key
// padding [batch][ctx_len] -> p->kpm where there is one.
static int stage_context(parseq_plan* p, hipStream_t s, const int32_t* tokens, int batch, int ctx_len, const uint8_t* key_padding_mask) {
    HIPCHK(hipMemcpy2DAsync(p->tok, LDT * sizeof(int), tokens, ctx_len * sizeof(int), ctx_len * sizeof(int), batch, hipMemcpyDeviceToDevice, s));
    CHK(launch(clamp_tokens_kernel, dim3((batch * ctx_len + 255) / 256), dim3(256), 0, s, p->tok, LDT, batch, ctx_len, p->m->cfg.num_tokens));
    if (key_padding_mask) HIPCHK(hipMemcpy2DAsync(p->kpm, LDT, key_padding_mask, ctx_len, ctx_len, batch, hipMemcpyDeviceToDevice, s));
    return 0;
}

// What a parseq_decode_* entry asks of decode_entry: the arguments every entry has, then those only some have.  The masks, hidden_out,
// user_query and content_mask may be null.
struct DecodeCall {
    const int32_t* tokens; int batch, ctx_len; const uint8_t *query_mask, *key_padding_mask; float* logits_out; void* stream;
    int q_start = 0, q_len = 0;
    float* hidden_out = nullptr;
    const float* user_query = nullptr;
    const uint8_t* content_mask = nullptr;
};

static int decode_entry(parseq_plan* p, const DecodeCall& d) {
    if (!p || !d.tokens || !d.logits_out) return fail(PARSEQ_E_INVALID, "null argument");
    if (p->m->vitstr) return fail(PARSEQ_E_INVALID, "ViTSTR has no decoder");
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    const int batch = d.batch, ctx_len = d.ctx_len, q_start = d.q_start, q_len = d.q_len;
    if (batch <= 0 || batch > p->max_batch || batch != p->last_batch) return fail(PARSEQ_E_INVALID, "batch %d does not match the last parseq_encode (%d)", batch, p->last_batch);
    const int npos = p->m->cfg.max_label_length + 1;
    if (ctx_len < 1 || ctx_len > npos || q_start < 0 || q_len < 1 || q_start + q_len > npos) return fail(PARSEQ_E_INVALID, "bad context / query range");
    hipStream_t s = (hipStream_t)d.stream;
    CHK(stage_context(p, s, d.tokens, batch, ctx_len, d.key_padding_mask));
    DecPass a; a.B = batch; a.Lk = ctx_len; a.i0 = q_start; a.Lq = q_len; a.user_query = d.user_query;
    if (d.key_padding_mask) a.kpm = p->kpm;
    if (d.query_mask) {      // rows are relative to q_start; the kernel indexes by absolute query position
        HIPCHK(hipMemcpy2DAsync(p->qmask_user + (size_t)q_start * LDT, LDT, d.query_mask, ctx_len, ctx_len, q_len, hipMemcpyDeviceToDevice, s));
        a.qmask = p->qmask_user;
    }
    if (d.content_mask && p->m->cfg.dec_depth > 1) {      // depth 1 never updates the content stream, so the reference never reads its mask (modules.py:119-124)
        HIPCHK(hipMemcpy2DAsync(p->cmask_user, LDT, d.content_mask, ctx_len, ctx_len, ctx_len, hipMemcpyDeviceToDevice, s));
        a.cmask = p->cmask_user;
    }
    a.logits_of_pass(d.logits_out, p->m->classes);      // the caller's tensor is [batch][q_len][C]
    a.fused_step_allowed = dec_route(p, false).step == STEP_FUSED && !d.hidden_out;      // hidden_out reads the query stream in p->t
    return dispatch_te(p, [&](auto te) {
        using T = typename decltype(te)::T;
        constexpr int E = decltype(te)::E;
        const DecW<T> w = dec_weights<T>(p);
        CHK((decoder_pass<T, E>(p, s, w, a)));
        // model.decode's return value: decoder.norm of the query stream (modules.py:124), fp32
        if (d.hidden_out) CHK((run_layernorm<float>(s, p->t, w.norm.g, w.norm.b, d.hidden_out, nullptr, batch * q_len, E, p->m->cfg.dec_ln_eps)));
        return 0;
    });
}

extern "C" int parseq_decode_logits(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, int q_start, int q_len,
                                    const uint8_t* query_mask, const uint8_t* key_padding_mask, float* logits_out, void* stream) {
    DecodeCall d{tokens, batch, ctx_len, query_mask, key_padding_mask, logits_out, stream};
    d.q_start = q_start; d.q_len = q_len;
    return decode_entry(p, d);
}

extern "C" int parseq_decode_hidden(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, int q_start, int q_len,
                                    const uint8_t* query_mask, const uint8_t* key_padding_mask, float* hidden_out, float* logits_out,
                                    void* stream) {
    if (!hidden_out) return fail(PARSEQ_E_INVALID, "null hidden_out");
    DecodeCall d{tokens, batch, ctx_len, query_mask, key_padding_mask, logits_out, stream};
    d.q_start = q_start; d.q_len = q_len; d.hidden_out = hidden_out;
    return decode_entry(p, d);
}

extern "C" int parseq_decode_query(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, const float* query, int q_len,
                                   const uint8_t* query_mask, const uint8_t* key_padding_mask, float* hidden_out, float* logits_out,
                                   void* stream) {
    if (!query) return fail(PARSEQ_E_INVALID, "null query");
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    if (q_len < 1 || q_len > p->m->cfg.max_label_length + 1) return fail(PARSEQ_E_INVALID, "q_len %d outside [1, %d]", q_len, p->m->cfg.max_label_length + 1);
    DecodeCall d{tokens, batch, ctx_len, query_mask, key_padding_mask, logits_out, stream};
    d.q_len = q_len; d.hidden_out = hidden_out; d.user_query = query;
    return decode_entry(p, d);
}

extern "C" int parseq_decode_ex(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, int q_start, int q_len, const float* query,
                                const uint8_t* query_mask, const uint8_t* content_mask, const uint8_t* key_padding_mask, float* hidden_out,
                                float* logits_out, void* stream) {
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    if (query && q_start != 0) return fail(PARSEQ_E_INVALID, "q_start %d with a caller-supplied query (must be 0)", q_start);
    DecodeCall d{tokens, batch, ctx_len, query_mask, key_padding_mask, logits_out, stream};
    d.q_start = q_start; d.q_len = q_len; d.hidden_out = hidden_out; d.user_query = query; d.content_mask = content_mask;
    return decode_entry(p, d);
}

// The cross-attention K / V of a caller-supplied encoder output (model.decode's `memory` argument, model.py:89): replaces the
// K / V cached by the last parseq_encode on this plan.
template <typename T>
static int set_memory_impl(parseq_plan* p, const float* memory, int B, hipStream_t s) {
    const parseq_model* m = p->m;
    const parseq_config& c = m->cfg;
    const int E = c.embed_dim, N = m->tokens, M = B * N;
    const Weights<T> W = weights_of<T>(p);
    const T* a;
    if constexpr (sizeof(T) == 2) {
        const size_t n = (size_t)M * E;
        CHK(launch(cvt_f32_to_bf16_kernel, dim3((unsigned)((n / 4 + 255) / 256)), dim3(256), 0, s, memory, reinterpret_cast<bf16_t*>(p->xn), n));
        a = reinterpret_cast<const T*>(p->xn);
    } else {
        a = memory;
    }
    p->kv24 = false;      // rows in the storage type from the generic GEMM
    for (int l = 0; l < c.dec_depth; ++l) {      // every decoder layer's K / V
        const T* w_in; const float* b_in;
        ca_in_proj(W, dec_layer_key(l), w_in, b_in);
        EpiHeads<T> ek; static_cast<EpiBase&>(ek) = epi_base(M, 2 * E, b_in + E);
        ek.seg[0] = reinterpret_cast<T*>(l ? p->kmem_l[l] : p->kmem); ek.seg[1] = reinterpret_cast<T*>(l ? p->vmem_l[l] : p->vmem); ek.seg[2] = nullptr;
        ek.E = E; ek.heads = c.dec_heads; ek.hd = DEC_HD; ek.tokens = N; ek.tr_from = 2;
        ProfScope ps_(&p->prof, T_KVMEM, s);
        CHK((run_gemm<T>(s, ARowMajor<T>{a, E}, w_in + (size_t)E * E, E, M, 2 * E, E, ek, E % 128 != 0)));
    }
    p->last_batch = B;
    return 0;
}

extern "C" int parseq_set_memory(parseq_plan* p, const float* memory, int batch, void* stream) {
    if (!p || !memory) return fail(PARSEQ_E_INVALID, "null argument");
    if (p->m->vitstr) return fail(PARSEQ_E_INVALID, "ViTSTR has no decoder");
    if (batch <= 0 || batch > p->max_batch) return fail(PARSEQ_E_INVALID, "batch %d outside (0, %d]", batch, p->max_batch);
    if (p->packed_version != p->m->version) return fail(PARSEQ_E_STATE, "model parameters changed after the plan was packed; call parseq_plan_refresh");
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    return dispatch_t(p, [&](auto te) { return set_memory_impl<typename decltype(te)::T>(p, memory, batch, (hipStream_t)stream); });
}

// -------------------------------------------------------------------------------------------------------------------
// character localisation
// -------------------------------------------------------------------------------------------------------------------
static int attention_check(const parseq_plan* p, int L) {
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    const parseq_model* m = p->m;
    if (m->vitstr) return fail(PARSEQ_E_INVALID, "attention maps on a ViTSTR model: ViTSTR has no decoder");
    if (m->cfg.dec_depth != 1) return fail(PARSEQ_E_INVALID, "attention maps at dec_depth %d: only dec_depth 1", m->cfg.dec_depth);
    const int npos = m->cfg.max_label_length + 1;
    if (L < 2 || L > npos) return fail(PARSEQ_E_INVALID, "ctx_len %d outside [2, %d]", L, npos);
    if (m->tokens > AM_MAX_S) return fail(PARSEQ_E_INVALID, "attention maps over %d memory tokens: at most %d", m->tokens, AM_MAX_S);
    return 0;
}

// The cloze pass of forward_impl's refinement over the content rows in p->tok (key padding in p->kpm), then the map of its last layer's
// cross-attention: the per-operation pass leaves the projected, unscaled queries of all B * L rows in p->qc (cross_mlp), and the memory's K
// rows are in whichever form the call that filled the plan left them.
template <typename T, int E>
static int attention_pass(parseq_plan* p, hipStream_t s, int B, int L, float* attn_out, float* logits_out) {
    CHK((decoder_pass<T, E>(p, s, dec_weights<T>(p), cloze_pass(p, B, L, logits_out))));
    const int H = p->m->cfg.dec_heads, S = p->m->tokens;
    const dim3 grid(B, (L + AM_QB - 1) / AM_QB), block(64 * AM_WAVES);
    if constexpr (sizeof(T) == 2) return launch(dec_cross_attn_map_kernel<AM_K_BF16>, grid, block, 0, s, p->qc, p->kmem, (size_t)0, p->kpm, LDT, H, L, S, dec_scale(), attn_out);
    else if (p->kv24) return launch(dec_cross_attn_map_kernel<AM_K_F24>, grid, block, 0, s, p->qc, p->kmem, p->kv_plane_elems, p->kpm, LDT, H, L, S, dec_scale(), attn_out);
    else return launch(dec_cross_attn_map_kernel<AM_K_F32>, grid, block, 0, s, p->qc, p->kmem, (size_t)0, p->kpm, LDT, H, L, S, dec_scale(), attn_out);
}

static int launch_geometry(hipStream_t s, const float* attn, const int32_t* lengths, int batch, int L, int gh, int gw, int ph, int pw, float* centres,
                           float* boxes, int32_t* peak, float* peak_mass) {
    const int rows = batch * L;
    return launch(attn_geometry_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, attn, lengths, rows, L, gh * gw, gw, (float)ph, (float)pw,
                  (float)(gh * ph), (float)(gw * pw), centres, boxes, peak, peak_mass);
}

extern "C" int parseq_decode_attention(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, const uint8_t* key_padding_mask,
                                       float* attn_out, float* logits_out, void* stream) {
    if (!p || !tokens || !attn_out) return fail(PARSEQ_E_INVALID, "null plan / tokens / attn_out");
    CHK(attention_check(p, ctx_len));
    if (batch <= 0 || batch > p->max_batch || batch != p->last_batch) return fail(PARSEQ_E_INVALID, "batch %d does not match the last parseq_encode (%d)", batch, p->last_batch);
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    hipStream_t s = (hipStream_t)stream;
    const parseq_config& c = p->m->cfg;
    CHK(stage_context(p, s, tokens, batch, ctx_len, key_padding_mask));
    if (!key_padding_mask) CHK(launch(attn_prep_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, p->tok, LDT, batch, ctx_len, c.eos_id, c.pad_id, p->kpm, LDT, (int*)nullptr, (int*)nullptr));
    return dispatch_te(p, [&](auto te) { return attention_pass<typename decltype(te)::T, decltype(te)::E>(p, s, batch, ctx_len, attn_out, logits_out); });
}

extern "C" int parseq_op_attention_geometry(const float* attn, const int32_t* lengths, int batch, int L, int gh, int gw, int ph, int pw,
                                            float* centres, float* boxes, int32_t* peak, float* peak_mass, void* stream) {
    if (!attn || !lengths || !centres || !boxes || !peak || !peak_mass) return fail(PARSEQ_E_INVALID, "null argument");
    if (batch <= 0 || L < 1 || gh < 1 || gw < 1 || ph < 1 || pw < 1 || (long long)batch * L > 0x7fffffffLL / 4 || (long long)gh * gw > 0x7fffffffLL / 4)
        return fail(PARSEQ_E_INVALID, "bad shape: batch %d, L %d, grid %d x %d, patch %d x %d", batch, L, gh, gw, ph, pw);
    return launch_geometry((hipStream_t)stream, attn, lengths, batch, L, gh, gw, ph, pw, centres, boxes, peak, peak_mass);
}

// parseq_localize's workspace: the forward's logits [batch][npos][C]
extern "C" size_t parseq_localize_workspace_bytes(const parseq_plan* p, int batch) {
    if (!p) { fail(PARSEQ_E_INVALID, "null plan"); return 0; }
    if (attention_check(p, p->m->cfg.max_label_length + 1) != 0) return 0;
    if (batch <= 0 || batch > p->max_batch) { fail(PARSEQ_E_INVALID, "batch %d outside (0, %d]", batch, p->max_batch); return 0; }
    size_t off = 0;
    carve(off, (size_t)batch * (p->m->cfg.max_label_length + 1) * p->m->classes * sizeof(float));
    return off;
}

extern "C" int parseq_localize(parseq_plan* p, const void* images, int images_dtype, int batch, const int32_t* tokens_in, int flags, int refine_iters,
                               int32_t* tokens_out, int32_t* lengths_out, float* attn_out, float* centres_out, float* boxes_out, int32_t* peak_out,
                               float* peak_mass_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    const int L = p->m->cfg.max_label_length + 1;
    CHK(attention_check(p, L));
    CHK(check_call(p, batch, images_dtype));
    if (!images || !tokens_out || !lengths_out || !attn_out || !centres_out || !boxes_out || !peak_out || !peak_mass_out || !workspace)
        return fail(PARSEQ_E_INVALID, "null images / output / workspace");
    if (refine_iters < 0) return fail(PARSEQ_E_INVALID, "refine_iters %d", refine_iters);
    const size_t need = parseq_localize_workspace_bytes(p, batch);
    if (workspace_bytes < need) return fail(PARSEQ_E_INVALID, "localize workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(PARSEQ_E_INVALID, "localize workspace not 16-byte aligned");
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    hipStream_t s = (hipStream_t)stream;
    const parseq_config& c = p->m->cfg;
    float* logits = reinterpret_cast<float*>(workspace);
    CHK(encode_dispatch(p, images, images_dtype, batch, nullptr, s));
    return dispatch_te(p, [&](auto te) {
        using T = typename decltype(te)::T;
        constexpr int E = decltype(te)::E;
        if (tokens_in) {
            CHK(launch(attn_content_kernel, dim3((batch * L + 255) / 256), dim3(256), 0, s, tokens_in, batch, L, c.bos_id, p->tok, LDT));
            CHK(launch(clamp_tokens_kernel, dim3((batch * L + 255) / 256), dim3(256), 0, s, p->tok, LDT, batch, L, c.num_tokens));
            CHK(launch(attn_prep_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, p->tok, LDT, batch, L, c.eos_id, c.pad_id, p->kpm, LDT, tokens_out, lengths_out));
        } else {
            // the model's own reading: parseq_forward without the early exit (which only truncates the view), then the context the next
            // refinement iteration would run on — [<bos>, arg-max of the final logits], keys from the first <eos> on padded
            CHK((forward_impl<T, E>(p, batch, flags & ~PARSEQ_FLAG_TESTING, refine_iters, L, logits, nullptr, s)));
            CHK(refine_prep(p, s, batch, L, logits, 1));
            CHK(launch(attn_prep_kernel, dim3((batch + 255) / 256), dim3(256), 0, s, p->tok, LDT, batch, L, c.eos_id, c.pad_id, (unsigned char*)nullptr, LDT, tokens_out, lengths_out));
        }
        CHK((attention_pass<T, E>(p, s, batch, L, attn_out, nullptr)));
        return launch_geometry(s, attn_out, lengths_out, batch, L, c.img_h / c.patch_h, c.img_w / c.patch_w, c.patch_h, c.patch_w, centres_out, boxes_out,
                               peak_out, peak_mass_out);
    });
}

// -------------------------------------------------------------------------------------------------------------------
// beam search
// -------------------------------------------------------------------------------------------------------------------
// The beams' state over rows = batch * W beams, resolved once per call: from the caller's workspace (beam_ws) or from the caller's tensors
// (the parseq_op_beam_* entries).  A part the call does not have is null.
struct BeamState {
    int* tok = nullptr; int ldt = 0;                                                                          // the histories [rows][ldt]
    float* score = nullptr; unsigned char* finished = nullptr; int* length = nullptr; int* picked = nullptr;  // [rows]
    int *node = nullptr, *word = nullptr;      // under a lexicon (section 19): every beam's trie node and word id [rows]
    float* ar_score = nullptr;                 // a refined search (section 20): the search's own score [rows]
    float* lp_tok = nullptr; int* amax = nullptr; float* lp_max = nullptr;      // ... and the row statistics of an iteration [rows][L]
    float* wsum = nullptr;                     // under a weighted automaton (section 24): the sum of the arc weights along every beam's path [rows]

    static BeamState of_tensors(int32_t* tokens, int ldt, float* scores, uint8_t* finished, int32_t* lengths, int32_t* picked,
                                int32_t* nodes = nullptr, int32_t* words = nullptr, float* ar_scores = nullptr) {
        return BeamState{tokens, ldt, scores, finished, lengths, picked, nodes, words, ar_scores};
    }
};
// Where a search's results go, best first per image: tokens [batch][W][num_steps], the others [batch][W]; words under a lexicon, ar_scores
// of a refined search.
// Under a weighted automaton scores are the fused values, model_scores the model's own sums and priors the weight sums.
struct BeamOut { int32_t* tokens; float* scores; int32_t* lengths; uint8_t* finished; int32_t* words = nullptr; float* ar_scores = nullptr;
                 float* model_scores = nullptr; float* priors = nullptr; };
// The weights of an automaton over the table of a lexicon (section 24): weight [nodes][C], the prior weight and the per-character bonus
struct BeamWeights { const float* weight = nullptr; float alpha = 0.f, beta = 0.f; };
// What a search was asked for beyond the plain one: the per-step trace, a lexicon (the caller's table and roots; forward_beam refuses a
// null table, so past it trie_next is set exactly under a lexicon), a refinement (the mode, the iterations, its trace), the weights that
// make the table an automaton (weighted implies lexicon; forward_beam refuses null weights).
struct BeamCall {
    const parseq_beam_trace* trace = nullptr;
    bool lexicon = false; const int32_t* trie_next = nullptr; int trie_nodes = 0; const int32_t* roots = nullptr;
    bool refine = false; int refine_mode = 0, refine_iters = 0; const parseq_beam_refine_trace* refine_trace = nullptr;
    bool weighted = false; BeamWeights wt;
};

// The parts of a caller's workspace, in carve()'s 256-byte steps.  Over a null base only `off`, the size so far, means anything.
struct Carver {
    unsigned char* base; size_t off = 0;
    template <typename T> T* take(size_t count) {
        const size_t o = carve(off, count * sizeof(T));
        return base ? reinterpret_cast<T*>(base + o) : nullptr;
    }
};
static void take_refine_stats(Carver& cv, size_t n, BeamState& b) { b.lp_tok = cv.take<float>(n); b.amax = cv.take<int>(n); b.lp_max = cv.take<float>(n); }

// The caller's workspace: the encoder memory of the crops, its W-fold replication (set_memory_impl's operand), one step's logits and the
// beams' scores / lengths / last picks / flags.  The histories live in p->tok, where the self-attention kernels read them.
// Under a lexicon (section 19) two more parts follow: every beam's trie node and word id.
// A refined search (section 20) adds the refinement logits of all num_steps positions, the row statistics and the search's own scores.
// A weighted automaton (section 24) adds, last, every beam's weight sum.
struct BeamWs { float *memory, *memory_rep, *logits, *rlogits; BeamState st; size_t total; };
static BeamWs beam_ws(const parseq_plan* p, int batch, int W, bool lexicon, int refine_steps, void* workspace = nullptr, bool weighted = false) {
    const parseq_model* m = p->m;
    const size_t rows = (size_t)batch * W, img = (size_t)m->tokens * m->cfg.embed_dim;
    Carver cv{reinterpret_cast<unsigned char*>(workspace)};
    BeamWs o{}; BeamState& b = o.st;
    b.tok = p->tok; b.ldt = LDT;
    o.memory = cv.take<float>(batch * img);
    o.memory_rep = cv.take<float>(rows * img);
    o.logits = cv.take<float>(rows * m->classes);
    b.score = cv.take<float>(rows); b.length = cv.take<int>(rows); b.picked = cv.take<int>(rows); b.finished = cv.take<unsigned char>(rows);
    if (lexicon) { b.node = cv.take<int>(rows); b.word = cv.take<int>(rows); }
    if (refine_steps > 0) {
        o.rlogits = cv.take<float>(rows * refine_steps * m->classes);
        take_refine_stats(cv, rows * refine_steps, b);
        b.ar_score = cv.take<float>(rows);
    }
    if (weighted) b.wsum = cv.take<float>(rows);
    o.total = cv.off;
    return o;
}

static int beam_check(const parseq_plan* p, int batch, int W, int num_steps) {
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    const parseq_model* m = p->m;
    if (m->vitstr) return fail(PARSEQ_E_INVALID, "beam search on a ViTSTR model: it has no AR loop");
    if (m->cfg.dec_depth > 1) return fail(PARSEQ_E_INVALID, "beam search at dec_depth %d: only dec_depth 1 (a deeper decoder's per-layer content cache would need re-parenting)", m->cfg.dec_depth);
    if (W < 1 || W > PARSEQ_BEAM_MAX_WIDTH || W > m->classes) return fail(PARSEQ_E_INVALID, "beam_width %d outside [1, min(%d, %d classes)]", W, PARSEQ_BEAM_MAX_WIDTH, m->classes);
    if (batch <= 0 || (long long)batch * W > p->max_batch) return fail(PARSEQ_E_INVALID, "batch %d x beam_width %d rows outside (0, %d]", batch, W, p->max_batch);
    const int npos = m->cfg.max_label_length + 1;
    if (num_steps < 1 || num_steps > npos) return fail(PARSEQ_E_INVALID, "num_steps %d outside [1, %d]", num_steps, npos);
    if (beam_step_lds(W, m->classes, LDT) > BEAM_LDS_MAX) return fail(PARSEQ_E_INVALID, "beam_width %d x %d classes does not fit the step kernel's LDS", W, m->classes);
    return 0;
}

// One selection step on logits [batch * W][C] (beam.h); trie_next: null for the unconstrained step; wt: the weights of a weighted step,
// whose fused values go to fused_out (may be null)
static int launch_beam_step(hipStream_t s, const float* logits, int batch, int W, int C, int step, const BeamState& b, int* parent_out, int eos_id,
                            int pad_id, const int32_t* trie_next = nullptr, int trie_nodes = 0, const BeamWeights* wt = nullptr, float* fused_out = nullptr) {
    if (wt)
        return launch(beam_step_kernel<true, true>, dim3(batch), dim3(BEAM_THREADS), beam_step_lds(W, C, b.ldt), s, logits, W, C, step, b.tok, b.ldt, b.score,
                      b.finished, b.length, parent_out, b.picked, eos_id, pad_id,
                      BeamAut{trie_next, trie_nodes, b.node, b.word, wt->weight, b.wsum, wt->alpha, wt->beta, fused_out});
    const auto kernel = trie_next ? beam_step_kernel<true> : beam_step_kernel<false>;
    return launch(kernel, dim3(batch), dim3(BEAM_THREADS), beam_step_lds(W, C, b.ldt), s, logits, W, C, step, b.tok, b.ldt, b.score, b.finished,
                  b.length, parent_out, b.picked, eos_id, pad_id, trie_next ? BeamLex{trie_next, trie_nodes, b.node, b.word} : BeamLex{});
}

// The selection of one refinement iteration on logits [batch * W][L][C]: the row statistics, then the per-image kernel (beam_refine.h).
static int launch_beam_refine(hipStream_t s, const float* logits, int batch, int W, int C, int L, int mode, const BeamState& b, int eos_id, int pad_id) {
    const size_t waves = (size_t)batch * W * L;
    CHK(launch(beam_refine_stats_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, s, logits, batch * W, L, C, b.tok, b.ldt, b.picked, b.lp_tok,
               b.amax, b.lp_max));
    return launch(beam_refine_select_kernel, dim3(batch), dim3(BEAM_THREADS), beam_refine_lds(W, b.ldt), s, mode, W, L, b.lp_tok, b.amax, b.lp_max, b.tok,
                  b.ldt, b.score, b.finished, b.length, b.picked, b.node, b.word, b.ar_score, eos_id, pad_id);
}

template <typename T, int E>
static int beam_impl(parseq_plan* p, int B, int W, int num_steps, const BeamWs& ws, const BeamOut& out, const BeamCall& call, hipStream_t s) {
    const parseq_config& c = p->m->cfg;
    const int C = p->m->classes, rows = B * W;
    const BeamState& b = ws.st;
    // every beam of an image attends to that image's memory: W copies through the projection every caller-supplied memory takes
    const size_t per_img4 = (size_t)p->m->tokens * E / 4, total4 = per_img4 * rows;
    CHK(launch(beam_replicate_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(ws.memory),
               reinterpret_cast<float4*>(ws.memory_rep), per_img4, W, total4));
    CHK(set_memory_impl<T>(p, ws.memory_rep, rows, s));
    CHK(launch(beam_init_kernel, dim3((rows * LDT + 255) / 256), dim3(256), 0, s, b.tok, b.ldt, rows, W, c.bos_id, c.pad_id, b.score, b.finished, b.length, b.picked));
    if (call.lexicon) CHK(launch(beam_init_lexicon_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, rows, W, call.roots, call.trie_nodes, b.score, b.node, b.word));
    if (call.weighted) CHK(launch(beam_init_automaton_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, rows, b.wsum));
    const DecW<T> w = dec_weights<T>(p);
    const parseq_beam_trace* tr = call.trace;
    DecPass a; a.B = rows;      // the per-operation step, one query per beam, on every beam's history
    for (int i = 0; i < num_steps; ++i) {
        a.Lk = i + 1; a.i0 = a.c0 = i; a.logits_of_pass(ws.logits, C);      // one step's logits [rows][C]
        CHK((decoder_pass<T, E>(p, s, w, a)));
        if (tr && tr->logits) HIPCHK(hipMemcpyAsync(tr->logits + (size_t)i * rows * C, ws.logits, (size_t)rows * C * sizeof(float), hipMemcpyDeviceToDevice, s));
        if (tr && tr->tokens_in) HIPCHK(hipMemcpy2DAsync(tr->tokens_in + (size_t)i * rows * num_steps, num_steps * sizeof(int), b.tok, LDT * sizeof(int),
                                                         num_steps * sizeof(int), rows, hipMemcpyDeviceToDevice, s));
        // the traced score of a weighted step is the fused value, which the kernel writes itself (b.score stays the model's sum)
        float* trace_score = tr && tr->score ? tr->score + (size_t)i * rows : nullptr;
        CHK(launch_beam_step(s, ws.logits, B, W, C, i, b, tr && tr->parent ? tr->parent + (size_t)i * rows : nullptr, c.eos_id, c.pad_id, call.trie_next,
                             call.trie_nodes, call.weighted ? &call.wt : nullptr, trace_score));
        if (trace_score && !call.weighted) HIPCHK(hipMemcpyAsync(tr->score + (size_t)i * rows, b.score, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (call.refine) {
        // cloze refinement of every beam (section 20): forward_impl's refinement iteration on rows = B * W, then the selection
        const parseq_beam_refine_trace* rt = call.refine_trace;
        HIPCHK(hipMemcpyAsync(b.ar_score, b.score, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
        for (int it = 0; it < call.refine_iters; ++it) {
            CHK((refine_iteration<T, E>(p, s, w, rows, num_steps, ws.rlogits, 0)));
            if (rt && rt->tokens_in) HIPCHK(hipMemcpy2DAsync(rt->tokens_in + (size_t)it * rows * num_steps, num_steps * sizeof(int), b.tok, LDT * sizeof(int),
                                                             num_steps * sizeof(int), rows, hipMemcpyDeviceToDevice, s));
            if (rt && rt->logits) HIPCHK(hipMemcpyAsync(rt->logits + (size_t)it * rows * num_steps * C, ws.rlogits, (size_t)rows * num_steps * C * sizeof(float),
                                                        hipMemcpyDeviceToDevice, s));
            CHK(launch_beam_refine(s, ws.rlogits, B, W, C, num_steps, call.refine_mode, b, c.eos_id, c.pad_id));
        }
        HIPCHK(hipMemcpyAsync(out.ar_scores, b.ar_score, (size_t)rows * sizeof(float), hipMemcpyDeviceToDevice, s));
    }
    if (call.lexicon) CHK(launch(beam_finish_lexicon_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, rows, b.score, b.finished, b.word, out.words));
    CHK(launch(beam_finish_kernel, dim3((rows * num_steps + 255) / 256), dim3(256), 0, s, b.tok, b.ldt, rows, num_steps, c.pad_id, b.score, b.finished,
               b.length, b.picked, out.tokens, out.scores, out.lengths, out.finished));
    if (call.weighted) CHK(launch(beam_finish_automaton_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, rows, b.score, b.wsum, b.length, call.wt.alpha,
                                  call.wt.beta, out.scores, out.model_scores, out.priors));
    return 0;
}

// The three search entries: the refusals in one order, the encoder into the workspace, then beam_impl.
static int forward_beam(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps, const BeamOut& out,
                        const BeamCall& call, void* workspace, size_t workspace_bytes, void* stream) {
    CHK(beam_check(p, batch, beam_width, num_steps));
    CHK(check_call(p, batch, images_dtype));
    if (!images || !out.tokens || !out.scores || !out.lengths || !out.finished || !workspace) return fail(PARSEQ_E_INVALID, "null images / output / workspace");
    if (call.lexicon && (!call.trie_next || !out.words)) return fail(PARSEQ_E_INVALID, "null trie table / words output");
    if (call.lexicon && call.trie_nodes < 1) return fail(PARSEQ_E_INVALID, "trie_nodes %d: a trie has at least its root", call.trie_nodes);
    if (call.weighted) {
        if (!call.wt.weight || !out.model_scores || !out.priors) return fail(PARSEQ_E_INVALID, "null automaton weights / model_scores / priors output");
        if (!std::isfinite(call.wt.alpha) || !std::isfinite(call.wt.beta)) return fail(PARSEQ_E_INVALID, "alpha %g / beta %g: both must be finite", (double)call.wt.alpha, (double)call.wt.beta);
    }
    if (call.refine) {
        const int mode = call.refine_mode, iters = call.refine_iters;
        if (mode != PARSEQ_BEAM_REFINE_SCORE && mode != PARSEQ_BEAM_REFINE_EDIT) return fail(PARSEQ_E_INVALID, "refine_mode %d: neither PARSEQ_BEAM_REFINE_SCORE nor PARSEQ_BEAM_REFINE_EDIT", mode);
        if (iters < 1) return fail(PARSEQ_E_INVALID, "refine_iters %d: at least 1", iters);
        if (mode == PARSEQ_BEAM_REFINE_SCORE && iters != 1) return fail(PARSEQ_E_INVALID, "refine_iters %d in score mode: rescoring is idempotent, it runs once", iters);
        if (mode == PARSEQ_BEAM_REFINE_EDIT && call.lexicon) return fail(PARSEQ_E_INVALID, "edit refinement under a lexicon: an edited reading can leave the word list; use the score mode");
        if (!out.ar_scores) return fail(PARSEQ_E_INVALID, "null ar_scores_out");
    }
    const BeamWs ws = beam_ws(p, batch, beam_width, call.lexicon, call.refine ? num_steps : 0, workspace, call.weighted);
    if (workspace_bytes < ws.total) return fail(PARSEQ_E_INVALID, "beam workspace of %zu bytes, %zu needed", workspace_bytes, ws.total);
    if ((uintptr_t)workspace % 16) return fail(PARSEQ_E_INVALID, "beam workspace not 16-byte aligned");
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    hipStream_t s = (hipStream_t)stream;
    CHK(encode_dispatch(p, images, images_dtype, batch, ws.memory, s));
    return dispatch_te(p, [&](auto te) { return beam_impl<typename decltype(te)::T, decltype(te)::E>(p, batch, beam_width, num_steps, ws, out, call, s); });
}

extern "C" size_t parseq_beam_workspace_bytes(const parseq_plan* p, int batch, int beam_width, int num_steps) {
    if (beam_check(p, batch, beam_width, num_steps) != 0) return 0;
    return beam_ws(p, batch, beam_width, false, 0).total;
}

extern "C" int parseq_forward_beam(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps,
                                   int32_t* tokens_out, float* scores_out, int32_t* lengths_out, uint8_t* finished_out,
                                   const parseq_beam_trace* trace, void* workspace, size_t workspace_bytes, void* stream) {
    BeamCall call; call.trace = trace;
    return forward_beam(p, images, images_dtype, batch, beam_width, num_steps, {tokens_out, scores_out, lengths_out, finished_out}, call, workspace,
                        workspace_bytes, stream);
}

// lexicon-constrained beam search
extern "C" size_t parseq_beam_lexicon_workspace_bytes(const parseq_plan* p, int batch, int beam_width, int num_steps) {
    if (beam_check(p, batch, beam_width, num_steps) != 0) return 0;
    return beam_ws(p, batch, beam_width, true, 0).total;
}

extern "C" int parseq_forward_beam_lexicon(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps,
                                           int32_t* tokens_out, float* scores_out, int32_t* lengths_out, uint8_t* finished_out,
                                           const parseq_beam_trace* trace, void* workspace, size_t workspace_bytes, void* stream,
                                           const int32_t* trie_next, int trie_nodes, const int32_t* roots, int32_t* words_out) {
    BeamCall call; call.trace = trace;
    call.lexicon = true; call.trie_next = trie_next; call.trie_nodes = trie_nodes; call.roots = roots;
    return forward_beam(p, images, images_dtype, batch, beam_width, num_steps, {tokens_out, scores_out, lengths_out, finished_out, words_out}, call,
                        workspace, workspace_bytes, stream);
}

// beam search over a weighted automaton
extern "C" size_t parseq_beam_automaton_workspace_bytes(const parseq_plan* p, int batch, int beam_width, int num_steps) {
    if (beam_check(p, batch, beam_width, num_steps) != 0) return 0;
    return beam_ws(p, batch, beam_width, true, 0, nullptr, true).total;
}

extern "C" int parseq_forward_beam_automaton(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps,
                                             int32_t* tokens_out, float* scores_out, int32_t* lengths_out, uint8_t* finished_out,
                                             const parseq_beam_trace* trace, void* workspace, size_t workspace_bytes, void* stream,
                                             const int32_t* next, const float* weight, int states, const int32_t* roots, float alpha, float beta,
                                             int32_t* words_out, float* model_scores_out, float* priors_out) {
    BeamCall call; call.trace = trace;
    call.lexicon = true; call.trie_next = next; call.trie_nodes = states; call.roots = roots;
    call.weighted = true; call.wt = BeamWeights{weight, alpha, beta};
    BeamOut out{tokens_out, scores_out, lengths_out, finished_out, words_out};
    out.model_scores = model_scores_out; out.priors = priors_out;
    return forward_beam(p, images, images_dtype, batch, beam_width, num_steps, out, call, workspace, workspace_bytes, stream);
}

// cloze refinement of the N-best
static_assert(PARSEQ_BEAM_REFINE_SCORE == BEAM_REFINE_SCORE && PARSEQ_BEAM_REFINE_EDIT == BEAM_REFINE_EDIT, "refinement modes of the header and the kernels");
extern "C" size_t parseq_beam_refine_workspace_bytes(const parseq_plan* p, int batch, int beam_width, int num_steps, int lexicon) {
    if (beam_check(p, batch, beam_width, num_steps) != 0) return 0;
    return beam_ws(p, batch, beam_width, lexicon != 0, num_steps).total;
}

extern "C" int parseq_forward_beam_refine(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps,
                                          int32_t* tokens_out, float* scores_out, int32_t* lengths_out, uint8_t* finished_out,
                                          const parseq_beam_trace* trace, void* workspace, size_t workspace_bytes, void* stream,
                                          const int32_t* trie_next, int trie_nodes, const int32_t* roots, int32_t* words_out, int refine_mode,
                                          int refine_iters, float* ar_scores_out, const parseq_beam_refine_trace* refine_trace) {
    BeamCall call; call.trace = trace;
    call.lexicon = trie_next != nullptr; call.trie_next = trie_next; call.trie_nodes = trie_nodes; call.roots = roots;      // no table: an unconstrained search
    call.refine = true; call.refine_mode = refine_mode; call.refine_iters = refine_iters; call.refine_trace = refine_trace;
    return forward_beam(p, images, images_dtype, batch, beam_width, num_steps, {tokens_out, scores_out, lengths_out, finished_out, words_out, ar_scores_out},
                        call, workspace, workspace_bytes, stream);
}

// the workspace of parseq_op_beam_refine: the statistics lp_tok, amax, lp_max [batch * W][L]
static size_t refine_op_ws(int batch, int W, int L, void* workspace, BeamState& b) {
    Carver cv{reinterpret_cast<unsigned char*>(workspace)};
    take_refine_stats(cv, (size_t)batch * W * L, b);
    return cv.off;
}
static bool refine_op_shape_ok(int batch, int W, int L) { return batch > 0 && W >= 1 && W <= PARSEQ_BEAM_MAX_WIDTH && L >= 1 && L <= BEAM_REFINE_MAX_L; }

extern "C" size_t parseq_op_beam_refine_workspace_bytes(int batch, int beam_width, int L) {
    BeamState b;
    return refine_op_shape_ok(batch, beam_width, L) ? refine_op_ws(batch, beam_width, L, nullptr, b) : 0;
}

extern "C" int parseq_op_beam_refine(const float* logits, int batch, int beam_width, int C, int L, int refine_mode, int32_t* tokens, int ldt,
                                     float* scores, uint8_t* finished, int32_t* lengths, int32_t* picked, int32_t* nodes, int32_t* words,
                                     float* ar_scores, int eos_id, int pad_id, void* workspace, size_t workspace_bytes, void* stream) {
    if (!logits || !tokens || !scores || !finished || !lengths || !picked || !ar_scores || !workspace) return fail(PARSEQ_E_INVALID, "null argument");
    if (!refine_op_shape_ok(batch, beam_width, L) || C < 1) return fail(PARSEQ_E_INVALID, "bad shape: batch %d, beam_width %d (1..%d), C %d, L %d (1..%d)", batch, beam_width, PARSEQ_BEAM_MAX_WIDTH, C, L, BEAM_REFINE_MAX_L);
    if (ldt < L || ldt > 64) return fail(PARSEQ_E_INVALID, "L %d / ldt %d: need L <= ldt <= 64", L, ldt);
    if (eos_id < 0 || eos_id >= C) return fail(PARSEQ_E_INVALID, "eos_id %d outside [0, %d)", eos_id, C);
    if (refine_mode != PARSEQ_BEAM_REFINE_SCORE && refine_mode != PARSEQ_BEAM_REFINE_EDIT) return fail(PARSEQ_E_INVALID, "refine_mode %d", refine_mode);
    BeamState b = BeamState::of_tensors(tokens, ldt, scores, finished, lengths, picked, nodes, words, ar_scores);
    const size_t need = refine_op_ws(batch, beam_width, L, workspace, b);
    if (workspace_bytes < need) return fail(PARSEQ_E_INVALID, "refinement workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(PARSEQ_E_INVALID, "refinement workspace not 16-byte aligned");
    return launch_beam_refine((hipStream_t)stream, logits, batch, beam_width, C, L, refine_mode, b, eos_id, pad_id);
}

// The three parseq_op_beam_step* entries: their refusals, then the step.  trie_next, nodes and words: the lexicon entry's; wt and
// fused_out: the automaton entry's.
static int beam_step_op(hipStream_t s, const float* logits, int batch, int W, int C, int step, const BeamState& b, int* parent_out, int eos_id, int pad_id,
                        bool lexicon, const int32_t* trie_next = nullptr, int trie_nodes = 0, const BeamWeights* wt = nullptr, float* fused_out = nullptr) {
    if (!logits || !b.tok || !b.score || !b.finished || !b.length || !b.picked || (lexicon && (!trie_next || !b.node || !b.word))) return fail(PARSEQ_E_INVALID, "null argument");
    if (wt && (!wt->weight || !b.wsum)) return fail(PARSEQ_E_INVALID, "null automaton weights / weight sums");
    if (wt && (!std::isfinite(wt->alpha) || !std::isfinite(wt->beta))) return fail(PARSEQ_E_INVALID, "alpha %g / beta %g: both must be finite", (double)wt->alpha, (double)wt->beta);
    if (batch <= 0 || C < 1 || W < 1 || W > PARSEQ_BEAM_MAX_WIDTH) return fail(PARSEQ_E_INVALID, "bad shape: batch %d, beam_width %d (1..%d), C %d", batch, W, PARSEQ_BEAM_MAX_WIDTH, C);
    if (step < 0 || b.ldt < step + 1 || b.ldt > 64) return fail(PARSEQ_E_INVALID, "step %d / ldt %d: need step + 1 <= ldt <= 64", step, b.ldt);
    if (eos_id < 0 || eos_id >= C) return fail(PARSEQ_E_INVALID, "eos_id %d outside [0, %d)", eos_id, C);
    if (lexicon && trie_nodes < 1) return fail(PARSEQ_E_INVALID, "trie_nodes %d: a trie has at least its root", trie_nodes);
    if (beam_step_lds(W, C, b.ldt) > BEAM_LDS_MAX) return fail(PARSEQ_E_INVALID, "beam_width %d x %d classes does not fit the step kernel's LDS", W, C);
    return launch_beam_step(s, logits, batch, W, C, step, b, parent_out, eos_id, pad_id, trie_next, trie_nodes, wt, fused_out);
}

extern "C" int parseq_op_beam_step(const float* logits, int batch, int beam_width, int C, int step, int32_t* tokens, int ldt, float* scores,
                                   uint8_t* finished, int32_t* lengths, int32_t* parent_out, int32_t* picked_out, int eos_id, int pad_id,
                                   void* stream) {
    return beam_step_op((hipStream_t)stream, logits, batch, beam_width, C, step, BeamState::of_tensors(tokens, ldt, scores, finished, lengths, picked_out),
                        parent_out, eos_id, pad_id, false);
}

extern "C" int parseq_op_beam_step_lexicon(const float* logits, int batch, int beam_width, int C, int step, int32_t* tokens, int ldt, float* scores,
                                           uint8_t* finished, int32_t* lengths, int32_t* parent_out, int32_t* picked_out, int eos_id, int pad_id,
                                           void* stream, const int32_t* trie_next, int trie_nodes, int32_t* nodes, int32_t* words) {
    return beam_step_op((hipStream_t)stream, logits, batch, beam_width, C, step,
                        BeamState::of_tensors(tokens, ldt, scores, finished, lengths, picked_out, nodes, words), parent_out, eos_id, pad_id, true, trie_next,
                        trie_nodes);
}

extern "C" int parseq_op_beam_step_automaton(const float* logits, int batch, int beam_width, int C, int step, int32_t* tokens, int ldt, float* scores,
                                             uint8_t* finished, int32_t* lengths, int32_t* parent_out, int32_t* picked_out, int eos_id, int pad_id,
                                             void* stream, const int32_t* next, const float* weight, int states, int32_t* nodes, int32_t* words,
                                             float alpha, float beta, float* wsums, float* fused_out) {
    BeamState b = BeamState::of_tensors(tokens, ldt, scores, finished, lengths, picked_out, nodes, words);
    b.wsum = wsums;
    const BeamWeights wt{weight, alpha, beta};
    return beam_step_op((hipStream_t)stream, logits, batch, beam_width, C, step, b, parent_out, eos_id, pad_id, true, next, states, &wt, fused_out);
}

// -------------------------------------------------------------------------------------------------------------------
// lexicon matching
// -------------------------------------------------------------------------------------------------------------------
static_assert(PARSEQ_LEXICON_MATCH_DEAD == LM_DEAD_DISTANCE && PARSEQ_LEXICON_ROW_BYTES == LM_ROW_BYTES, "lexicon matching constants of the header and the kernels");

// What the matching kernel reads besides the readings: the caller's table and the optional arrays beside it.
struct LexMatch { const uint8_t* table; int n_rows; const int32_t *row_ids, *ranges, *fold; int C, eos_id, n; };

static int lexmatch_shape_check(int batch, int ldt, const LexMatch& m) {
    if (batch <= 0) return fail(PARSEQ_E_INVALID, "batch %d", batch);
    if (ldt < 1 || ldt > LM_MAX_READING) return fail(PARSEQ_E_INVALID, "readings of %d positions: 1 .. %d", ldt, LM_MAX_READING);
    if (!m.table || m.n_rows < 1) return fail(PARSEQ_E_INVALID, "null or empty word table (n_rows %d)", m.n_rows);
    if (m.n_rows > (1 << LM_KEY_SHIFT)) return fail(PARSEQ_E_INVALID, "word table of %d rows: at most 2^%d", m.n_rows, LM_KEY_SHIFT);
    if ((uintptr_t)m.table % 16) return fail(PARSEQ_E_INVALID, "word table not 16-byte aligned");
    if (m.C < 1 || m.C > LM_MAX_CLASSES) return fail(PARSEQ_E_INVALID, "%d classes: a class id of the table is a byte, 1 .. %d", m.C, LM_MAX_CLASSES);
    if (m.eos_id < 0 || m.eos_id >= m.C) return fail(PARSEQ_E_INVALID, "eos_id %d outside [0, %d)", m.eos_id, m.C);
    if (m.n < 1 || m.n > PARSEQ_BEAM_MAX_WIDTH) return fail(PARSEQ_E_INVALID, "n %d outside [1, %d]", m.n, PARSEQ_BEAM_MAX_WIDTH);
    if ((long long)batch * lm_chunks(m.n_rows) * m.n > 0x7fffffffLL) return fail(PARSEQ_E_INVALID, "batch %d x %d rows x n %d: the partial lists pass 2^31 keys", batch, m.n_rows, m.n);
    return 0;
}

static size_t lexmatch_partial_keys(int batch, int n_rows, int n) { return (size_t)batch * lm_chunks(n_rows) * n; }

// The match of `batch` readings [batch][ldt]: the partial lists, then the merge.  crops_per_block 0: enough workgroups to fill the device
// (about 2048) where the list alone does not give them.  The result does not depend on it.
static int launch_lexicon_match(hipStream_t s, const int32_t* readings, int ldt, const int32_t* lengths, int batch, const LexMatch& m, int crops_per_block,
                                unsigned* partial, int32_t* word_ids, int32_t* distances, int32_t* rows_out) {
    const int wblocks = (m.n_rows + LM_THREADS - 1) / LM_THREADS, tiles = (batch + LM_TC - 1) / LM_TC, chunks = lm_chunks(m.n_rows);
    if (crops_per_block <= 0) {
        const int groups = std::max(1, std::min(tiles, (2048 + wblocks - 1) / wblocks));
        crops_per_block = (tiles + groups - 1) / groups * LM_TC;
    }
    const int groups = (batch + crops_per_block - 1) / crops_per_block;
    if (groups > 65535) return fail(PARSEQ_E_INVALID, "crops_per_block %d at batch %d: more than 65535 crop groups", crops_per_block, batch);
    CHK(launch(lexicon_match_kernel, dim3(wblocks, groups), dim3(LM_THREADS), 0, s, readings, ldt, lengths, batch, reinterpret_cast<const unsigned*>(m.table),
               m.n_rows, m.ranges, m.fold, m.C, m.eos_id, m.n, partial, chunks, crops_per_block));
    return launch(lexicon_match_merge_kernel, dim3(batch), dim3(LM_THREADS), 0, s, partial, chunks, m.n_rows, m.ranges, m.row_ids, m.n, word_ids, distances, rows_out);
}

extern "C" size_t parseq_op_lexicon_match_workspace_bytes(int batch, int n_rows, int n) {
    if (batch <= 0 || n_rows < 1 || n_rows > (1 << LM_KEY_SHIFT) || n < 1 || n > PARSEQ_BEAM_MAX_WIDTH || (long long)batch * lm_chunks(n_rows) * n > 0x7fffffffLL) return 0;
    size_t off = 0;
    carve(off, lexmatch_partial_keys(batch, n_rows, n) * sizeof(unsigned));
    return off;
}

extern "C" int parseq_op_lexicon_match(const int32_t* readings, int ldt, const int32_t* lengths, int batch, const uint8_t* table, int n_rows,
                                       const int32_t* row_ids, const int32_t* ranges, const int32_t* fold, int C, int eos_id, int n, int crops_per_block,
                                       int32_t* word_ids_out, int32_t* distances_out, void* workspace, size_t workspace_bytes, void* stream) {
    if (!readings || !word_ids_out || !distances_out || !workspace) return fail(PARSEQ_E_INVALID, "null readings / output / workspace");
    const LexMatch m{table, n_rows, row_ids, ranges, fold, C, eos_id, n};
    CHK(lexmatch_shape_check(batch, ldt, m));
    if (crops_per_block < 0) return fail(PARSEQ_E_INVALID, "crops_per_block %d", crops_per_block);
    const size_t need = parseq_op_lexicon_match_workspace_bytes(batch, n_rows, n);
    if (workspace_bytes < need) return fail(PARSEQ_E_INVALID, "lexicon match workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(PARSEQ_E_INVALID, "lexicon match workspace not 16-byte aligned");
    return launch_lexicon_match((hipStream_t)stream, readings, ldt, lengths, batch, m, crops_per_block, reinterpret_cast<unsigned*>(workspace), word_ids_out,
                                distances_out, nullptr);
}

// The whole call's refusals, in beam_check's style; W = n (+ 1 with keep_reading) hypotheses per crop.
static int lexmatch_check(const parseq_plan* p, int batch, const parseq_lexicon_match_args* a) {
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    if (!a) return fail(PARSEQ_E_INVALID, "null lexicon match arguments");
    const parseq_model* m = p->m;
    if (m->vitstr) return fail(PARSEQ_E_INVALID, "lexicon matching on a ViTSTR model: it has no decoder to rescore with");
    if (m->cfg.dec_depth > 1) return fail(PARSEQ_E_INVALID, "lexicon matching at dec_depth %d: only dec_depth 1", m->cfg.dec_depth);
    const int keep = a->keep_reading ? 1 : 0;
    if (a->n < 1 || a->n + keep > PARSEQ_BEAM_MAX_WIDTH) return fail(PARSEQ_E_INVALID, "n %d outside [1, %d]%s", a->n, PARSEQ_BEAM_MAX_WIDTH - keep, keep ? " (one slot is the reading's)" : "");
    if (batch <= 0 || (long long)batch * (a->n + keep) > p->max_batch) return fail(PARSEQ_E_INVALID, "batch %d x %d hypotheses outside (0, %d]", batch, a->n + keep, p->max_batch);
    const LexMatch lm{a->table, a->n_rows, a->row_ids, a->ranges, a->fold, m->classes, m->cfg.eos_id, a->n};
    CHK(lexmatch_shape_check(batch, m->cfg.max_label_length + 1, lm));
    if (a->table_own && (uintptr_t)a->table_own % 16) return fail(PARSEQ_E_INVALID, "word table not 16-byte aligned");
    return 0;
}

// The caller's workspace: the forward's logits, the match (partial lists, rows, ids, distances), the beam state, and with rescoring the
// memory, its W-fold replication, the refinement logits and the row statistics.
struct LexMatchWs { float *memory, *memory_rep, *logits, *rlogits; unsigned* partial; int *m_rows, *m_ids, *m_dist; BeamState st; size_t total; };
static LexMatchWs lexmatch_ws(const parseq_plan* p, int batch, const parseq_lexicon_match_args* a, void* workspace = nullptr) {
    const parseq_model* m = p->m;
    const int W = a->n + (a->keep_reading ? 1 : 0), L = m->cfg.max_label_length + 1;
    const size_t rows = (size_t)batch * W, img = (size_t)m->tokens * m->cfg.embed_dim;
    Carver cv{reinterpret_cast<unsigned char*>(workspace)};
    LexMatchWs o{}; BeamState& b = o.st;
    b.tok = p->tok; b.ldt = LDT;
    o.logits = cv.take<float>((size_t)batch * L * m->classes);
    o.partial = cv.take<unsigned>(lexmatch_partial_keys(batch, a->n_rows, a->n));
    o.m_rows = cv.take<int>((size_t)batch * a->n); o.m_ids = cv.take<int>((size_t)batch * a->n); o.m_dist = cv.take<int>((size_t)batch * a->n);
    b.score = cv.take<float>(rows); b.length = cv.take<int>(rows); b.picked = cv.take<int>(rows); b.finished = cv.take<unsigned char>(rows);
    b.node = cv.take<int>(rows); b.word = cv.take<int>(rows);      // node: the hypothesis' distance, which moves with its row as a trie node does
    b.ar_score = cv.take<float>(rows);
    if (a->rescore) {
        o.memory = cv.take<float>(batch * img);
        o.memory_rep = cv.take<float>(rows * img);
        o.rlogits = cv.take<float>(rows * L * m->classes);
        take_refine_stats(cv, rows * L, b);
    }
    o.total = cv.off;
    return o;
}

extern "C" size_t parseq_forward_lexicon_match_workspace_bytes(const parseq_plan* p, int batch, const parseq_lexicon_match_args* args) {
    if (lexmatch_check(p, batch, args) != 0) return 0;
    return lexmatch_ws(p, batch, args).total;
}

struct LexMatchOut { int32_t* tokens; float* scores; int32_t* lengths; uint8_t* finished; int32_t *words, *distances, *reading, *reading_len; };

template <typename T, int E>
static int lexmatch_impl(parseq_plan* p, int B, int flags, int refine_iters, const parseq_lexicon_match_args* a, const LexMatchWs& ws, const LexMatchOut& out,
                         hipStream_t s) {
    const parseq_config& c = p->m->cfg;
    const int C = p->m->classes, L = c.max_label_length + 1, N = a->n, W = N + (a->keep_reading ? 1 : 0), rows = B * W;
    const BeamState& b = ws.st;
    // the reading forward would give: its logits, then the arg-max of every position and the index of the first <eos>
    CHK((forward_impl<T, E>(p, B, flags & ~PARSEQ_FLAG_TESTING, refine_iters, L, ws.logits, nullptr, s)));
    CHK(launch(postprocess_kernel, dim3((B + 3) / 4), dim3(256), 0, s, ws.logits, B, L, C, c.eos_id, out.reading, out.reading_len, (float*)nullptr, (float*)nullptr));
    const LexMatch lm{a->table, a->n_rows, a->row_ids, a->ranges, a->fold, C, c.eos_id, N};
    CHK(launch_lexicon_match(s, out.reading, L, out.reading_len, B, lm, 0, ws.partial, ws.m_ids, ws.m_dist, ws.m_rows));
    const size_t cells = (size_t)rows * b.ldt;
    CHK(launch(lexicon_seed_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, s, B, N, a->keep_reading ? 1 : 0, L, a->table_own ? a->table_own : a->table,
               ws.m_rows, ws.m_ids, ws.m_dist, out.reading, out.reading_len, c.bos_id, c.eos_id, c.pad_id, b.tok, b.ldt, b.score, b.finished, b.length, b.picked,
               b.word, b.node, b.ar_score));
    if (a->rescore) {
        // section 20's 'score' selection on the seeded rows: every candidate against its crop's memory, one cloze pass
        const size_t per_img4 = (size_t)p->m->tokens * E / 4, total4 = per_img4 * rows;
        CHK(launch(beam_replicate_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(ws.memory),
                   reinterpret_cast<float4*>(ws.memory_rep), per_img4, W, total4));
        CHK(set_memory_impl<T>(p, ws.memory_rep, rows, s));
        const DecW<T> w = dec_weights<T>(p);
        CHK((refine_iteration<T, E>(p, s, w, rows, L, ws.rlogits, 0)));
        CHK(launch_beam_refine(s, ws.rlogits, B, W, C, L, PARSEQ_BEAM_REFINE_SCORE, b, c.eos_id, c.pad_id));
    }
    HIPCHK(hipMemcpyAsync(out.distances, b.node, (size_t)rows * sizeof(int), hipMemcpyDeviceToDevice, s));
    CHK(launch(beam_finish_lexicon_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, rows, b.score, b.finished, b.word, out.words));
    return launch(beam_finish_kernel, dim3((rows * L + 255) / 256), dim3(256), 0, s, b.tok, b.ldt, rows, L, c.pad_id, b.score, b.finished, b.length, b.picked,
                  out.tokens, out.scores, out.lengths, out.finished);
}

extern "C" int parseq_forward_lexicon_match(parseq_plan* p, const void* images, int images_dtype, int batch, int flags, int refine_iters,
                                            const parseq_lexicon_match_args* args, int32_t* tokens_out, float* scores_out, int32_t* lengths_out,
                                            uint8_t* finished_out, int32_t* words_out, int32_t* distances_out, int32_t* reading_tokens_out,
                                            int32_t* reading_lengths_out, void* workspace, size_t workspace_bytes, void* stream) {
    CHK(lexmatch_check(p, batch, args));
    CHK(check_call(p, batch, images_dtype));
    if (!images || !tokens_out || !scores_out || !lengths_out || !finished_out || !words_out || !distances_out || !reading_tokens_out || !reading_lengths_out || !workspace)
        return fail(PARSEQ_E_INVALID, "null images / output / workspace");
    if (refine_iters < 0) return fail(PARSEQ_E_INVALID, "refine_iters %d", refine_iters);
    const LexMatchWs ws = lexmatch_ws(p, batch, args, workspace);
    if (workspace_bytes < ws.total) return fail(PARSEQ_E_INVALID, "lexicon match workspace of %zu bytes, %zu needed", workspace_bytes, ws.total);
    if ((uintptr_t)workspace % 16) return fail(PARSEQ_E_INVALID, "lexicon match workspace not 16-byte aligned");
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    hipStream_t s = (hipStream_t)stream;
    CHK(encode_dispatch(p, images, images_dtype, batch, ws.memory, s));      // (without rescoring ws.memory is null: nothing reads the memory again)
    const LexMatchOut out{tokens_out, scores_out, lengths_out, finished_out, words_out, distances_out, reading_tokens_out, reading_lengths_out};
    return dispatch_te(p, [&](auto te) { return lexmatch_impl<typename decltype(te)::T, decltype(te)::E>(p, batch, flags, refine_iters, args, ws, out, s); });
}

// -------------------------------------------------------------------------------------------------------------------
// orientation-robust reading (orient.h): the best of K turned views of every crop
// -------------------------------------------------------------------------------------------------------------------
// What postprocess_kernel leaves for the batch * views rows.
struct OrientWs { int *ids, *lens; float *probs, *confs; size_t total; };
static OrientWs orient_ws(int batch, int views, int L, void* workspace = nullptr) {
    const size_t rows = (size_t)batch * views;
    Carver cv{reinterpret_cast<unsigned char*>(workspace)};
    OrientWs o{};
    o.ids = cv.take<int>(rows * L); o.probs = cv.take<float>(rows * L); o.lens = cv.take<int>(rows); o.confs = cv.take<float>(rows);
    o.total = cv.off;
    return o;
}

static int orient_shape_check(int batch, int views, int L) {
    if (views < 1 || views > ORIENT_MAX_VIEWS) return fail(PARSEQ_E_INVALID, "orient: %d views, it must be in 1 .. %d", views, ORIENT_MAX_VIEWS);
    if (batch < 1 || (long long)batch * views > (1 << 26)) return fail(PARSEQ_E_INVALID, "orient: batch %d x %d views outside (0, %d]", batch, views, 1 << 26);
    if (L < 1 || L > 64) return fail(PARSEQ_E_INVALID, "orient: L = %d positions, it must be in 1 .. 64", L);
    return 0;
}

extern "C" size_t parseq_op_orient_select_workspace_bytes(int batch, int views, int L) {
    if (orient_shape_check(batch, views, L) != 0) return 0;
    return orient_ws(batch, views, L).total;
}

extern "C" int parseq_op_orient_select(const float* logits, int batch, int views, int L, int C, int eos_id, const void* images, int images_dtype,
                                       int64_t image_elems, int criterion, const float* prior, int32_t* view_out, double* keys_out, float* logits_out,
                                       int32_t* ids_out, int32_t* lengths_out, float* confidence_out, void* images_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    static_assert(ORIENT_MAX_VIEWS == PARSEQ_ORIENT_MAX_VIEWS && ORIENT_MEAN == PARSEQ_ORIENT_MEAN && ORIENT_SUM == PARSEQ_ORIENT_SUM, "header and kernel must agree");
    CHK(orient_shape_check(batch, views, L));
    if (C < 1 || eos_id < 0 || eos_id >= C) return fail(PARSEQ_E_INVALID, "orient: C = %d classes, eos_id %d", C, eos_id);
    if (criterion != PARSEQ_ORIENT_MEAN && criterion != PARSEQ_ORIENT_SUM) return fail(PARSEQ_E_INVALID, "orient: unknown criterion %d", criterion);
    if (!logits || !view_out || !keys_out || !logits_out || !ids_out || !lengths_out || !confidence_out || !workspace)
        return fail(PARSEQ_E_INVALID, "orient: null logits / output / workspace");
    size_t image_bytes = 0;
    if (images || images_out) {
        if (!images || !images_out) return fail(PARSEQ_E_INVALID, "orient: images and images_out go together");
        if (images_dtype != PARSEQ_F32 && images_dtype != PARSEQ_BF16 && images_dtype != PARSEQ_U8) return fail(PARSEQ_E_INVALID, "orient: images_dtype %d", images_dtype);
        if (image_elems < 1 || image_elems > (int64_t)1 << 32) return fail(PARSEQ_E_INVALID, "orient: %lld elements per crop", (long long)image_elems);
        image_bytes = (size_t)image_elems * (images_dtype == PARSEQ_F32 ? 4 : images_dtype == PARSEQ_BF16 ? 2 : 1);
    }
    const OrientWs ws = orient_ws(batch, views, L, workspace);
    if (workspace_bytes < ws.total) return fail(PARSEQ_E_INVALID, "orient workspace of %zu bytes, %zu needed", workspace_bytes, ws.total);
    if ((uintptr_t)workspace % 16) return fail(PARSEQ_E_INVALID, "orient workspace not 16-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    const int rows = batch * views;
    CHK(launch(postprocess_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, rows, L, C, eos_id, ws.ids, ws.lens, ws.probs, ws.confs));
    return launch(orient_select_kernel, dim3(batch), dim3(ORIENT_THREADS), 0, s, logits, (const int*)ws.ids, (const int*)ws.lens, (const float*)ws.probs,
                  (const float*)ws.confs, images, image_bytes, views, L, C, criterion, prior, view_out, keys_out, logits_out, ids_out, lengths_out,
                  confidence_out, images_out);
}

// The whole call's workspace: the logits of the batch * views rows, then the op's.
static int orient_forward_check(const parseq_plan* p, int batch, int views, int num_steps, int criterion) {
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    if (p->m->vitstr) return fail(PARSEQ_E_INVALID, "parseq_forward_oriented on a ViTSTR model: parseq_vitstr_forward, then parseq_op_orient_select");
    const int npos = p->m->cfg.max_label_length + 1;
    if (num_steps < 1 || num_steps > npos) return fail(PARSEQ_E_INVALID, "num_steps %d outside [1, %d]", num_steps, npos);
    CHK(orient_shape_check(batch, views, num_steps));
    if ((long long)batch * views > p->max_batch) return fail(PARSEQ_E_INVALID, "orient: batch %d x %d views outside (0, %d]", batch, views, p->max_batch);
    if (criterion != PARSEQ_ORIENT_MEAN && criterion != PARSEQ_ORIENT_SUM) return fail(PARSEQ_E_INVALID, "orient: unknown criterion %d", criterion);
    return 0;
}

extern "C" size_t parseq_forward_oriented_workspace_bytes(const parseq_plan* p, int batch, int views, int num_steps) {
    if (orient_forward_check(p, batch, views, num_steps, PARSEQ_ORIENT_MEAN) != 0) return 0;
    size_t off = 0;
    carve(off, (size_t)batch * views * num_steps * p->m->classes * sizeof(float));
    return off + orient_ws(batch, views, num_steps).total;
}

extern "C" int parseq_forward_oriented(parseq_plan* p, const void* images, int images_dtype, int batch, int views, int flags, int refine_iters,
                                       int num_steps, int criterion, const float* prior, int32_t* view_out, double* keys_out, float* logits_out,
                                       int32_t* ids_out, int32_t* lengths_out, float* confidence_out, void* images_out, void* workspace,
                                       size_t workspace_bytes, void* stream) {
    CHK(orient_forward_check(p, batch, views, num_steps, criterion));
    if (!view_out || !keys_out || !logits_out || !ids_out || !lengths_out || !confidence_out || !workspace) return fail(PARSEQ_E_INVALID, "orient: null output / workspace");
    const size_t need = parseq_forward_oriented_workspace_bytes(p, batch, views, num_steps);
    if (workspace_bytes < need) return fail(PARSEQ_E_INVALID, "orient workspace of %zu bytes, %zu needed", workspace_bytes, need);
    if ((uintptr_t)workspace % 16) return fail(PARSEQ_E_INVALID, "orient workspace not 16-byte aligned");
    const parseq_config& c = p->m->cfg;
    const int rows = batch * views;
    size_t off = 0;
    carve(off, (size_t)rows * num_steps * p->m->classes * sizeof(float));
    float* all = reinterpret_cast<float*>(workspace);
    // every position of every view: the early exit only truncates what parseq_forward returns, and a reading is cut at its <eos> anyway
    CHK(parseq_forward(p, images, images_dtype, rows, flags & ~PARSEQ_FLAG_TESTING, refine_iters, num_steps, all, nullptr, stream));
    DevGuard dg(p->m->device);
    return parseq_op_orient_select(all, batch, views, num_steps, p->m->classes, c.eos_id, images_out ? images : nullptr, images_dtype,
                                   (int64_t)3 * c.img_h * c.img_w, criterion, prior, view_out, keys_out, logits_out, ids_out, lengths_out, confidence_out,
                                   images_out, static_cast<unsigned char*>(workspace) + off, workspace_bytes - off, stream);
}

// -------------------------------------------------------------------------------------------------------------------
// long text lines (line_stitch.h): overlapping windows of a line, stitched by position
// -------------------------------------------------------------------------------------------------------------------
static int stitch_check(int rows, int L, int C, int img_h, int img_w, int lines, int max_out) {
    static_assert(LINE_MAX_WINDOWS == PARSEQ_LINE_MAX_WINDOWS && LINE_MAX_OUT == PARSEQ_LINE_MAX_OUT && LINE_MAX_L == DEC_MAXL, "header and kernel must agree");
    if (L < 1 || L > LINE_MAX_L) return fail(PARSEQ_E_INVALID, "lines: L = %d positions, it must be in 1 .. %d", L, LINE_MAX_L);
    if (lines < 1 || rows < lines) return fail(PARSEQ_E_INVALID, "lines: %d lines over %d rows: there must be a line, and a row for each", lines, rows);
    if (max_out < 1 || max_out > LINE_MAX_OUT) return fail(PARSEQ_E_INVALID, "lines: max_out %d, it must be in 1 .. %d", max_out, LINE_MAX_OUT);
    if (C < 1 || img_h < 1 || img_w < 1) return fail(PARSEQ_E_INVALID, "lines: C = %d classes, input of %d x %d", C, img_h, img_w);
    return 0;
}

extern "C" int parseq_op_stitch_lines(const int32_t* tokens, const int32_t* lengths, const float* probs, const float* centres, const float* boxes, int rows,
                                      int L, int C, const int32_t* win, int img_h, int img_w, const int32_t* line_first, int lines, const double* min_sep,
                                      int max_out, int32_t* len_out, int32_t* tokens_out, float* probs_out, float* boxes_out, double* x_out,
                                      int32_t* src_out, float* confidence_out, void* stream) {
    if (!tokens || !lengths || !probs || !centres || !boxes || !win || !line_first || !min_sep || !len_out || !tokens_out || !probs_out || !boxes_out ||
        !x_out || !src_out || !confidence_out)
        return fail(PARSEQ_E_INVALID, "lines: null argument");
    CHK(stitch_check(rows, L, C, img_h, img_w, lines, max_out));
    const LineStitchArgs a{tokens, lengths, probs, centres, boxes, rows, L, C, win, img_h, img_w, line_first, min_sep, max_out,
                           len_out, tokens_out, probs_out, boxes_out, x_out, src_out, confidence_out};
    return launch(line_stitch_kernel, dim3(lines), dim3(LINE_THREADS), 0, (hipStream_t)stream, a);
}

// parseq_read_lines' workspace: parseq_localize's (the logits, at the start), then what the call keeps to itself — the maps, their peaks and
// what postprocess_kernel leaves beside the probabilities.
struct ReadLinesWs { size_t localize; float* attn; int* peak; float* peak_mass; int* ids; int* lens; size_t total; };
static ReadLinesWs read_lines_ws(const parseq_plan* p, int rows, size_t localize, void* workspace = nullptr) {
    const size_t L = p->m->cfg.max_label_length + 1;
    Carver cv{reinterpret_cast<unsigned char*>(workspace)};
    cv.off = localize;
    ReadLinesWs w{};
    w.localize = localize;
    w.attn = cv.take<float>((size_t)rows * L * p->m->tokens);
    w.peak = cv.take<int>((size_t)rows * L); w.peak_mass = cv.take<float>((size_t)rows * L);
    w.ids = cv.take<int>((size_t)rows * L); w.lens = cv.take<int>(rows);
    w.total = cv.off;
    return w;
}

extern "C" size_t parseq_read_lines_workspace_bytes(const parseq_plan* p, int rows) {
    const size_t localize = parseq_localize_workspace_bytes(p, rows);
    if (localize == 0) return 0;
    return read_lines_ws(p, rows, localize).total;
}

extern "C" int parseq_read_lines(parseq_plan* p, const void* images, int images_dtype, int rows, int flags, int refine_iters, const int32_t* win,
                                 const int32_t* line_first, int lines, const double* min_sep, int max_out, int32_t* tokens_out, int32_t* lengths_out,
                                 float* probs_out, float* centres_out, float* boxes_out, int32_t* line_len_out, int32_t* line_tokens_out,
                                 float* line_probs_out, float* line_boxes_out, double* line_x_out, int32_t* line_src_out, float* line_confidence_out,
                                 void* workspace, size_t workspace_bytes, void* stream) {
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    const int L = p->m->cfg.max_label_length + 1;
    CHK(attention_check(p, L));
    if (!win || !line_first || !min_sep || !probs_out || !line_len_out || !line_tokens_out || !line_probs_out || !line_boxes_out || !line_x_out ||
        !line_src_out || !line_confidence_out)
        return fail(PARSEQ_E_INVALID, "lines: null argument");
    const parseq_config& c = p->m->cfg;
    CHK(stitch_check(rows, L, p->m->classes, c.img_h, c.img_w, lines, max_out));
    const size_t localize = parseq_localize_workspace_bytes(p, rows);
    if (localize == 0) return PARSEQ_E_INVALID;
    const ReadLinesWs ws = read_lines_ws(p, rows, localize, workspace);
    if (workspace && workspace_bytes < ws.total) return fail(PARSEQ_E_INVALID, "lines workspace of %zu bytes, %zu needed", workspace_bytes, ws.total);
    // the windows are rows of an ordinary batch: read and localise them (its own refusals come before any device work, too)
    CHK(parseq_localize(p, images, images_dtype, rows, nullptr, flags, refine_iters, tokens_out, lengths_out, ws.attn, centres_out, boxes_out, ws.peak,
                        ws.peak_mass, workspace, localize, stream));
    DevGuard dg(p->m->device);
    hipStream_t s = (hipStream_t)stream;
    const float* logits = reinterpret_cast<const float*>(workspace);
    CHK(launch(postprocess_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, logits, rows, L, p->m->classes, c.eos_id, ws.ids, ws.lens, probs_out, (float*)nullptr));
    return parseq_op_stitch_lines(tokens_out, lengths_out, probs_out, centres_out, boxes_out, rows, L, p->m->classes, win, c.img_h, c.img_w, line_first,
                                  lines, min_sep, max_out, line_len_out, line_tokens_out, line_probs_out, line_boxes_out, line_x_out, line_src_out,
                                  line_confidence_out, stream);
}

// -------------------------------------------------------------------------------------------------------------------
// scoring of given readings (score.h): joint log-probabilities of candidates in any decoding order
// -------------------------------------------------------------------------------------------------------------------
static_assert(SCORE_MAX_N == PARSEQ_SCORE_MAX_CANDIDATES && SCORE_MAX_ORDERS == PARSEQ_SCORE_MAX_ORDERS && SCORE_MEAN == PARSEQ_SCORE_MEAN &&
              SCORE_LENGTH_NORM == PARSEQ_SCORE_LENGTH_NORM && PARSEQ_SCORE_MIX == 0 && LDT <= SCORE_MAX_L, "header and kernel must agree");

static int score_op_check(int batch, int n, int L, int orders, int flags) {
    if (n < 1 || n > SCORE_MAX_N) return fail(PARSEQ_E_INVALID, "score: %d candidates per crop, it must be in 1 .. %d", n, SCORE_MAX_N);
    if (orders < 1 || orders > SCORE_MAX_ORDERS) return fail(PARSEQ_E_INVALID, "score: %d orders, it must be in 1 .. %d", orders, SCORE_MAX_ORDERS);
    if (batch < 1 || (long long)batch * n > (1 << 26)) return fail(PARSEQ_E_INVALID, "score: batch %d x %d candidates outside (0, %d]", batch, n, 1 << 26);
    if (L < 1 || L > SCORE_MAX_L) return fail(PARSEQ_E_INVALID, "score: L = %d positions, it must be in 1 .. %d", L, SCORE_MAX_L);
    if (flags & ~(PARSEQ_SCORE_MEAN | PARSEQ_SCORE_LENGTH_NORM)) return fail(PARSEQ_E_INVALID, "score: unknown flags 0x%x", flags);
    return 0;
}

extern "C" int parseq_op_score_rows(const float* logits, int rows, int L, int C, const int32_t* targets, const int32_t* lengths, const uint8_t* valid,
                                    int orders, int order, float* order_scores, float* char_logprobs, void* stream) {
    if (!logits || !targets || !lengths || !valid || !order_scores) return fail(PARSEQ_E_INVALID, "score: null argument");
    if (rows < 1 || rows > (1 << 26) || C < 1) return fail(PARSEQ_E_INVALID, "score: %d rows of %d classes", rows, C);
    if (L < 1 || L > SCORE_MAX_L) return fail(PARSEQ_E_INVALID, "score: L = %d positions, it must be in 1 .. %d", L, SCORE_MAX_L);
    if (orders < 1 || orders > SCORE_MAX_ORDERS || order < 0 || order >= orders) return fail(PARSEQ_E_INVALID, "score: order %d of %d (1 .. %d)", order, orders, SCORE_MAX_ORDERS);
    return launch(score_rows_kernel, dim3(rows), dim3(256), 0, (hipStream_t)stream, logits, L, C, targets, lengths, valid, orders, order, order_scores, char_logprobs);
}

extern "C" int parseq_op_score_rank(const float* order_scores, const int32_t* lengths, const uint8_t* valid, int batch, int n, int orders, int flags,
                                    float* scores_out, int32_t* rank_out, void* stream) {
    if (!order_scores || !lengths || !valid || !scores_out || !rank_out) return fail(PARSEQ_E_INVALID, "score: null argument");
    CHK(score_op_check(batch, n, 1, orders, flags));
    return launch(score_rank_kernel, dim3(batch), dim3(64), 0, (hipStream_t)stream, order_scores, lengths, valid, n, orders, flags, scores_out, rank_out);
}

// The caller's workspace: the encoder memory of the crops, its N-fold replication (set_memory_impl's operand), one order's logits of every
// position and the targets the seed leaves.  The token rows and the key padding live in the plan, where the decoder reads them.
struct ScoreWs { float *memory, *memory_rep, *logits; int* target; size_t total; };
static ScoreWs score_ws(const parseq_plan* p, int batch, int n, int L, void* workspace = nullptr) {
    const parseq_model* m = p->m;
    const size_t rows = (size_t)batch * n, img = (size_t)m->tokens * m->cfg.embed_dim;
    Carver cv{reinterpret_cast<unsigned char*>(workspace)};
    ScoreWs o{};
    o.memory = cv.take<float>(batch * img);
    o.memory_rep = cv.take<float>(rows * img);
    o.logits = cv.take<float>(rows * L * m->classes);
    o.target = cv.take<int>(rows * L);
    o.total = cv.off;
    return o;
}

static int score_check(const parseq_plan* p, int batch, int n, int num_steps, int orders, int flags) {
    if (!p) return fail(PARSEQ_E_INVALID, "null plan");
    const parseq_model* m = p->m;
    if (m->vitstr) return fail(PARSEQ_E_INVALID, "parseq_score on a ViTSTR model: it has no decoder to condition on a reading");
    if (m->cfg.dec_depth > 1) return fail(PARSEQ_E_INVALID, "parseq_score at dec_depth %d: only dec_depth 1", m->cfg.dec_depth);
    const int npos = m->cfg.max_label_length + 1;
    if (num_steps < 2 || num_steps > npos) return fail(PARSEQ_E_INVALID, "score: num_steps %d outside [2, %d]", num_steps, npos);
    CHK(score_op_check(batch, n, num_steps, orders, flags));
    if ((long long)batch * n > p->max_batch) return fail(PARSEQ_E_INVALID, "score: batch %d x %d candidates outside (0, %d]", batch, n, p->max_batch);
    return 0;
}

extern "C" size_t parseq_score_workspace_bytes(const parseq_plan* p, int batch, int n, int num_steps, int orders) {
    if (score_check(p, batch, n, num_steps, orders, 0) != 0) return 0;
    return score_ws(p, batch, n, num_steps).total;
}

template <typename T, int E>
static int score_impl(parseq_plan* p, int B, int N, int L, const int32_t* candidates, const uint8_t* query_masks, int K, int flags, const ScoreWs& ws,
                      float* scores_out, float* order_scores_out, float* char_logprobs_out, int32_t* rank_out, int32_t* lengths_out, uint8_t* valid_out,
                      hipStream_t s) {
    const parseq_config& c = p->m->cfg;
    const int C = p->m->classes, rows = B * N;
    // every candidate of a crop attends to that crop's memory: N copies through the projection every caller-supplied memory takes
    const size_t per_img4 = (size_t)p->m->tokens * E / 4, total4 = per_img4 * rows;
    CHK(launch(beam_replicate_kernel, dim3((unsigned)((total4 + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float4*>(ws.memory),
               reinterpret_cast<float4*>(ws.memory_rep), per_img4, N, total4));
    CHK(set_memory_impl<T>(p, ws.memory_rep, rows, s));
    CHK(launch(score_seed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, candidates, rows, L, C, c.bos_id, c.eos_id, c.pad_id, p->tok, LDT, p->kpm, LDT,
               ws.target, lengths_out, valid_out));
    const DecW<T> w = dec_weights<T>(p);
    // the teacher-forced pass of training_step (system.py:183-189): every position queried against the whole context under the order's mask
    DecPass a; a.B = rows; a.Lk = a.Lq = L; a.qmask = p->qmask_user; a.kpm = p->kpm; a.logits = ws.logits; a.Ltot = L;
    for (int k = 0; k < K; ++k) {
        HIPCHK(hipMemcpy2DAsync(p->qmask_user, LDT, query_masks + (size_t)k * L * L, L, L, L, hipMemcpyDeviceToDevice, s));
        CHK((decoder_pass<T, E>(p, s, w, a)));
        CHK(launch(score_rows_kernel, dim3(rows), dim3(256), 0, s, (const float*)ws.logits, L, C, (const int*)ws.target, (const int*)lengths_out,
                   (const unsigned char*)valid_out, K, k, order_scores_out, char_logprobs_out));
    }
    return launch(score_rank_kernel, dim3(B), dim3(64), 0, s, (const float*)order_scores_out, (const int*)lengths_out, (const unsigned char*)valid_out, N, K,
                  flags, scores_out, rank_out);
}

extern "C" int parseq_score(parseq_plan* p, const void* images, int images_dtype, int batch, const int32_t* candidates, int n, int num_steps,
                            const uint8_t* query_masks, int orders, int flags, float* scores_out, float* order_scores_out, float* char_logprobs_out,
                            int32_t* rank_out, int32_t* lengths_out, uint8_t* valid_out, void* workspace, size_t workspace_bytes, void* stream) {
    CHK(score_check(p, batch, n, num_steps, orders, flags));
    CHK(check_call(p, batch, images_dtype));
    if (!images || !candidates || !query_masks || !scores_out || !order_scores_out || !rank_out || !lengths_out || !valid_out || !workspace)
        return fail(PARSEQ_E_INVALID, "score: null images / candidates / query_masks / output / workspace");
    const ScoreWs ws = score_ws(p, batch, n, num_steps, workspace);
    if (workspace_bytes < ws.total) return fail(PARSEQ_E_INVALID, "score workspace of %zu bytes, %zu needed", workspace_bytes, ws.total);
    if ((uintptr_t)workspace % 16) return fail(PARSEQ_E_INVALID, "score workspace not 16-byte aligned");
    DevGuard dg(p->m->device);
    SplitScope ss(p->precision == PARSEQ_BF16X3);
    hipStream_t s = (hipStream_t)stream;
    CHK(encode_dispatch(p, images, images_dtype, batch, ws.memory, s));
    return dispatch_te(p, [&](auto te) {
        return score_impl<typename decltype(te)::T, decltype(te)::E>(p, batch, n, num_steps, candidates, query_masks, orders, flags, ws, scores_out,
                                                                     order_scores_out, char_logprobs_out, rank_out, lengths_out, valid_out, s);
    });
}
