/*
 * parseq_hip.h — C ABI of libparseq_hip.so, the MI355X (gfx950) implementation of the PARSeq inference hot path.
 *
 * The reference (baudm/parseq @ /root/reference, strhub 1.2.0) is pure Python and has NO plugin / operator / FFI
 * interface for this path: the boundary it exposes is `PARSeq.forward(tokenizer, images, max_length)`
 * (strhub/models/parseq/model.py:105-169, called through strhub/models/parseq/system.py:87-88).  This header is the
 * interface a native backend sits behind; each entry point names the reference code it replaces.  The Python
 * binding a maintainer would add is shown in INTEGRATION.md; this repo's own binding is parseq_amd/_native.py
 * (ctypes).
 *
 * Conventions
 *   - plain C: opaque handles, raw pointers, sizes.  No torch / ATen types.
 *   - every `const void*` / `float*` below that is documented "device" must be a pointer into HIP device memory
 *     of the device that was current when the model was created.  The caller owns all such buffers.
 *   - every call enqueues on the `hipStream_t` passed as `void* stream` (NULL = the default stream) and returns
 *     without synchronising, EXCEPT where stated (parseq_forward with PARSEQ_FLAG_TESTING and refine_iters == 0,
 *     which has to read one int back — the reference has a device->host sync per AR step at model.py:144).
 *   - return value: 0 on success, a negative PARSEQ_E_* code otherwise; parseq_last_error() gives the message
 *     (thread-local).  No exceptions cross the boundary.
 *   - a model and its plans are not internally locked: use one plan per host thread / stream.
 *   - devices: a model lives on the device that was current at parseq_model_create; every entry point that takes a model or
 *     a plan makes that device current for the duration of the call and restores the caller's (so `stream` must be a stream
 *     of the model's device).  The raw-pointer entry points (parseq_op_*, parseq_postprocess, parseq_resize_bicubic,
 *     parseq_rotate_resize_bicubic, parseq_cross_entropy, parseq_grad_norm) launch on the CURRENT device.  Per-kernel launch attributes are tracked per
 *     device, so one process may drive several GPUs / host threads (one plan each).
 *   - memory: the caller owns every tensor it passes; each plan owns ONE device arena (packed weights, decoder tables and all
 *     intermediates, about 0.9 GB at max_batch 512 in bf16) taken from hipMalloc (parseq_plan_create) or from the caller's
 *     allocator (parseq_plan_create_ex, ABI 7: "all workspace through the host framework's caching allocator", SURVEY.md
 *     section 8b), and the model one hipMalloc'ed buffer of fp32 master weights.  Nothing is allocated on the hot path; the
 *     arena's lifetime is the plan's.
 */
#ifndef PARSEQ_HIP_H_
#define PARSEQ_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PARSEQ_ABI_VERSION 15

/* (ABI 9) deepest decoder a model may have: parseq_config.dec_depth in [1, PARSEQ_DEC_DEPTH_MAX] */
#define PARSEQ_DEC_DEPTH_MAX 4

typedef struct parseq_model parseq_model;   /* weights of one PARSeq instance on one device */
typedef struct parseq_plan parseq_plan;     /* workspace + derived tables for (model, max_batch, precision) */

/* Constructor arguments of the reference model that shape the arithmetic
 * (strhub/models/parseq/model.py:33-49; values from configs/model/parseq.yaml, configs/main.yaml:9-10). */
typedef struct parseq_config {
    int32_t img_h, img_w;          /* 32, 128 */
    int32_t patch_h, patch_w;      /* 4, 8 */
    int32_t embed_dim;             /* 384 (PARSeq-S), 192 (PARSeq-Ti) */
    int32_t enc_depth, enc_heads, enc_mlp_ratio;   /* 12, 6 | 3, 4 */
    int32_t dec_depth, dec_heads, dec_mlp_ratio;   /* 1 (the reference default; 1 .. PARSEQ_DEC_DEPTH_MAX), 12 | 6, 4 */
    int32_t num_tokens;            /* len(tokenizer) = 97 for the 94-char set; the head predicts num_tokens - 2 classes */
    int32_t max_label_length;      /* 25 */
    int32_t bos_id, eos_id, pad_id;/* 95, 0, 96  (strhub/data/utils.py:107-111) */
    float enc_ln_eps, dec_ln_eps;  /* 1e-6 (timm ViT), 1e-5 (nn.LayerNorm default) */
    int32_t arch;                  /* PARSEQ_ARCH_PARSEQ (0) or PARSEQ_ARCH_VITSTR (1): the ViT encoder
                                    * with a class token and a per-token head (strhub/models/vitstr/model.py:20-28), no decoder;
                                    * the dec_* fields are ignored and the parameter keys are timm's (cls_token, pos_embed,
                                    * patch_embed.proj.*, blocks.N.*, norm.*, head.*) */
} parseq_config;

enum { PARSEQ_ARCH_PARSEQ = 0, PARSEQ_ARCH_VITSTR = 1 };

enum {
    PARSEQ_F32 = 0,    /* exact mode: f32 storage, v_mfma_f32_16x16x4_f32; parity target |dlogit| <= 1e-3 vs CPU fp32 */
    PARSEQ_BF16 = 1,   /* throughput mode: bf16 GEMM/attention operands, fp32 accumulate / residual / LayerNorm / softmax */
    PARSEQ_BF16X3 = 3, /* precision only (plans, parseq_op_linear / parseq_op_encoder_attention): exact-tolerance mode at matrix-core
                        * speed.  Storage is f32 exactly as in PARSEQ_F32 (images are passed as PARSEQ_F32 / _BF16 / _U8), but every
                        * GEMM / attention operand is split into a bf16 pair hi = bf16(v), lo = bf16(v - hi) and every product is
                        * evaluated as hi*hi + hi*lo + lo*hi on v_mfma_f32_*_bf16 with fp32 accumulation: ~2^-17 relative error per
                        * product (bf16: 2^-9), 3 bf16 MFMAs per product instead of the f32 MFMA's 16x cost.  Meets the north
                        * star's |dlogit| <= 1e-3 with argmax-identical decodes (tests/test_hip_parity.py) */
    PARSEQ_U8 = 2      /* images_dtype only: raw 0..255 pixels, [batch, 3, H, W]; the patch-embed
                        * operand loader applies the reference transform's ToTensor + Normalize(0.5, 0.5)
                        * (strhub/data/module.py:78-81): ((v / 255) - 0.5) / 0.5 in f32, bit-identical to feeding the
                        * normalised f32 image (then rounded to bf16 in bf16 mode) */
};

enum {
    PARSEQ_FLAG_DECODE_AR = 1,   /* model.decode_ar (model.py:53,119): autoregressive vs one-shot NAR decoding */
    PARSEQ_FLAG_TESTING = 2,     /* max_length was None (model.py:106): batch-level early exit applies (model.py:144-145) */
    PARSEQ_FLAG_LATENCY = 4      /* (ABI 6) a hint, never a change of semantics: this forward has the device to itself (the reference's one call
                                  * at a time), so the AR step may spread its out_proj -> norm1 -> q-projection chain over three workgroups per
                                  * row tile (decoder_step.h DS_QS: a shorter dependent chain for ~2x the compute-unit time of that kernel).
                                  * Leave it clear when several forwards are in flight on different streams — there the compute units
                                  * the wider step takes are another batch's.  Results of the two forms differ by rounding only. */
};

enum {
    PARSEQ_E_INVALID = -1,       /* bad argument / unsupported configuration */
    PARSEQ_E_HIP = -2,           /* a HIP runtime call failed */
    PARSEQ_E_STATE = -3,         /* weights missing / not finalised */
    PARSEQ_E_ARCH = -4           /* device is not gfx950 */
};

int parseq_abi_version(void);
const char* parseq_last_error(void);

/* ---- model: replaces the nn.Module parameter storage of strhub/models/parseq/model.py:56-67 ---------------------- */

/* Validates the configuration (1 <= dec_depth <= PARSEQ_DEC_DEPTH_MAX, head dims 64 / 32, embed_dim in {192, 384, 768}, 128 tokens) and the
 * device architecture.  Allocates device storage for the fp32 master weights. */
int parseq_model_create(const parseq_config* cfg, parseq_model** out);
void parseq_model_destroy(parseq_model* m);

/* Copies one parameter (fp32, contiguous, `numel` elements) from device memory.  `key` is the reference
 * state_dict key (e.g. "encoder.blocks.3.attn.qkv.weight", "decoder.layers.0.cross_attn.in_proj_weight",
 * "pos_queries"; full list: SURVEY.md section 8b), so a released checkpoint can be streamed in key by key.
 * Unknown key or wrong numel -> PARSEQ_E_INVALID. */
int parseq_model_set_param(parseq_model* m, const char* key, const float* device_ptr, int64_t numel, void* stream);

/* Number of parameters / i-th key and element count, for binding-side validation. */
int parseq_model_num_params(const parseq_model* m);
int parseq_model_param_info(const parseq_model* m, int index, const char** key, int64_t* numel);

/* ---- plan: per-(max_batch, precision) workspace, packed weights and batch-independent decoder tables ------------ */

/* All device memory the hot path needs is allocated here, never inside parseq_forward / parseq_encode.
 * Requires every parameter to have been set.  precision: PARSEQ_F32, PARSEQ_BF16 or PARSEQ_BF16X3.  (Re)packs weights for `precision`; call parseq_plan_refresh after
 * parameters change. */
int parseq_plan_create(parseq_model* m, int max_batch, int precision, void* stream, parseq_plan** out);
/* (ABI 7) The same with the plan's ONE device arena taken from the caller's allocator instead of hipMalloc — "all workspace through the
 * host framework's caching allocator" (what the reference gets for free from torch: every intermediate of
 * strhub/models/parseq/model.py:86-169 is a caching-allocator block).  alloc(bytes, user) is called exactly once, inside this call, on the
 * model's device, with bytes == what parseq_plan_workspace_bytes will report; it returns device memory aligned to 256 bytes or NULL
 * (-> PARSEQ_E_HIP).  release(ptr, user) is called exactly once from parseq_plan_destroy (or from this call if a later step of the
 * creation fails); the caller's release must not recycle the block while work of this plan is still in flight on any stream (hipFree
 * synchronises implicitly; a caching allocator does not).  alloc == NULL and release == NULL: hipMalloc / hipFree (parseq_plan_create).
 * A torch binding hands c10::hip::HIPCachingAllocator::raw_alloc / raw_delete; the ctypes binding of this repository allocates a uint8
 * torch tensor per plan (parseq_amd/_native.py torch_plan_allocator). */
typedef void* (*parseq_alloc_fn)(size_t bytes, void* user);
typedef void (*parseq_release_fn)(void* ptr, void* user);
int parseq_plan_create_ex(parseq_model* m, int max_batch, int precision, void* stream, parseq_alloc_fn alloc, parseq_release_fn release,
                          void* user, parseq_plan** out);
int parseq_plan_refresh(parseq_plan* p, void* stream);
void parseq_plan_destroy(parseq_plan* p);
size_t parseq_plan_workspace_bytes(const parseq_plan* p);

/* Optional per-kernel-family timing: while enabled, every launch is bracketed by HIP events on the caller's stream
 * (this perturbs throughput: use a separate pass).  parseq_plan_get_profile(index) returns 0 and fills the family name,
 * accumulated milliseconds and launch count since profiling was (re-)enabled, or returns 1 when index is past the last
 * family; it synchronises on the recorded events. */
int parseq_plan_set_profiling(parseq_plan* p, int enable);
int parseq_plan_get_profile(parseq_plan* p, int index, const char** name, double* total_ms, int64_t* launches);

/* ---- hot path ---------------------------------------------------------------------------------------------------- */

/* model.PARSeq.encode (model.py:83-84 -> modules.py:163-165 -> timm ViT.forward_features).
 * images: device, [batch, 3, img_h, img_w], contiguous; normalised fp32 (images_dtype = PARSEQ_F32) or bf16 (PARSEQ_BF16),
 * or raw uint8 pixels (PARSEQ_U8, normalised on the fly).
 * memory_out: device fp32 [batch, tokens, embed_dim], or NULL to keep the result only inside the plan. */
int parseq_encode(parseq_plan* p, const void* images, int images_dtype, int batch, float* memory_out, void* stream);

/* model.PARSeq.forward (model.py:105-169): encode, AR loop or NAR pass, `refine_iters` cloze refinements.
 * num_steps = min(max_length, max_label_length) + 1 (model.py:107-110), i.e. 26 by default.
 * logits_out: device fp32 [batch, num_steps, num_tokens - 2], contiguous.  Rows [*, 0:L, *] are valid, where L is
 * written to *out_len (host int): L = num_steps, except AR + PARSEQ_FLAG_TESTING + refine_iters == 0, where L is the
 * early-exit length of model.py:144-145 and the call synchronises the stream to read it. */
int parseq_forward(parseq_plan* p, const void* images, int images_dtype, int batch, int flags, int refine_iters,
                   int num_steps, float* logits_out, int* out_len, void* stream);

/* model.PARSeq.decode + head for the contexts the reference's forward() builds (model.py:86-103, 138, 152, 167),
 * exposed for per-stage parity tests: `memory` must have been produced by parseq_encode on this plan (its K/V
 * projection is cached in the plan).  tokens: device int32 [batch, ctx_len] (tgt_in).  Queries are
 * pos_queries[q_start : q_start + q_len].  query_mask: device uint8 [num_steps? no: (max_label_length + 1)] x ctx_len
 * rows indexed by absolute query position, or NULL; key_padding_mask: device uint8 [batch, ctx_len] or NULL
 * (non-zero = masked, torch semantics).  logits_out: device fp32 [batch, q_len, num_tokens - 2]. */
int parseq_decode_logits(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, int q_start, int q_len,
                         const uint8_t* query_mask, const uint8_t* key_padding_mask, float* logits_out, void* stream);

/* model.PARSeq.decode (model.py:86-103): the same pass as parseq_decode_logits, additionally returning what `decode`
 * returns in the reference — the decoder output after decoder.norm (modules.py:124), fp32 [batch, q_len, embed_dim] — so that
 * `model.head(model.decode(...))` keeps working.  logits_out is written too (head of the same pass, library arithmetic). */
int parseq_decode_hidden(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, int q_start, int q_len,
                         const uint8_t* query_mask, const uint8_t* key_padding_mask, float* hidden_out, float* logits_out,
                         void* stream);

/* model.PARSeq.decode with a caller-supplied query stream (model.py:100-102: `tgt_query` need not be a slice of pos_queries):
 * query: device fp32 [batch, q_len, embed_dim].  norm_q + the query projection run at call time, self-attention scores are
 * computed against the content-key table, and the residual stream starts from `query` itself (modules.py:60-66).
 * query_mask: device uint8 [q_len, ctx_len] or NULL.  hidden_out: fp32 [batch, q_len, embed_dim] or NULL; logits_out as above. */
int parseq_decode_query(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, const float* query, int q_len,
                        const uint8_t* query_mask, const uint8_t* key_padding_mask, float* hidden_out, float* logits_out,
                        void* stream);

/* (ABI 9) model.PARSeq.decode with every argument of the reference (model.py:86-103), including the content mask `tgt_mask`, which
 * only a decoder deeper than one layer reads (layers 0 .. dec_depth - 2 update the content stream under it, modules.py:116-124).
 * query: device fp32 [batch, q_len, embed_dim] (caller-supplied tgt_query; q_start must be 0) or NULL (pos_queries[q_start :
 * q_start + q_len]).  query_mask: device uint8 [q_len, ctx_len] or NULL; content_mask: device uint8 [ctx_len, ctx_len] or NULL;
 * key_padding_mask: device uint8 [batch, ctx_len] or NULL (non-zero = masked).  hidden_out: fp32 [batch, q_len, embed_dim] or NULL;
 * logits_out: fp32 [batch, q_len, num_tokens - 2].  The three entry points above are this one with content_mask == NULL, i.e. the
 * reference with tgt_mask=None; at dec_depth == 1 the content mask is ignored, exactly as the reference ignores it. */
int parseq_decode_ex(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, int q_start, int q_len, const float* query,
                     const uint8_t* query_mask, const uint8_t* content_mask, const uint8_t* key_padding_mask, float* hidden_out,
                     float* logits_out, void* stream);

/* model.PARSeq.decode's `memory` argument (model.py:89): projects a caller-supplied encoder output — device fp32
 * [batch, tokens, embed_dim], as parseq_encode returns it (after the encoder's final norm) — to the decoder's cross-attention
 * K / V of every decoder layer, replacing the ones cached by the last parseq_encode / parseq_forward on this plan.  The decode entry points then
 * attend to THIS memory until the next encode / forward / set_memory. */
int parseq_set_memory(parseq_plan* p, const float* memory, int batch, void* stream);

/* ---- beam search (added under ABI 15: pure additions; the reference has none, DESIGN.md section 18 defines it) ------- */

/* Beam-search AR decoding with N-best output for a PARSeq model of dec_depth 1, in every plan precision.  For `batch` crops, beam width
 * W = beam_width (1 .. PARSEQ_BEAM_MAX_WIDTH, <= num_tokens - 2, batch * W <= the plan's max_batch) and num_steps as in parseq_forward:
 *   hypothesis  a sequence of class ids (<eos> and the charset); score = sum over its positions of log_softmax(logits)[chosen], natural
 *               log, fp32, the <eos> term included, no length normalisation
 *   start       beam 0 = [<bos>] at score 0, beams 1 .. W-1 dead (score -inf; a dead beam offers no candidate)
 *   step i      every live unfinished beam w offers its C candidates (w, c) at score[w] + logp[w][c], every finished beam itself at its
 *               score; the W best become the new beams in rank order: higher score, then lower parent, then lower class (a finished
 *               carry counts as class -1).  Picking <eos> finishes a beam; its later token slots hold pad_id
 * All num_steps steps always run; the call makes no host read and does not synchronise.  Outputs (device, best first per image):
 *   tokens_out   int32 [batch, W, num_steps]      lengths_out  int32 [batch, W] characters before <eos> (num_steps if there is none)
 *   scores_out   fp32  [batch, W]                 finished_out uint8 [batch, W] 0 = no <eos> after the last step
 * The encoder memory is replicated W times and projected through parseq_set_memory's path, so afterwards the plan's cached K / V are
 * those of the replicated batch (last batch = batch * W) until the next encode / forward / set_memory.
 * trace: NULL, or four nullable device pointers filled per step i (tests and diagnosis), rows in the order the decoder ran them:
 *   logits    fp32  [num_steps][batch * W][C]             the step's logits
 *   tokens_in int32 [num_steps][batch * W][num_steps]     the histories the step ran on (<bos> first, pad_id past position i)
 *   parent    int32 [num_steps][batch * W]                new beam r's parent row within its image after the step (-1: dead)
 *   score     fp32  [num_steps][batch * W]                new beam r's score after the step
 * workspace: device, parseq_beam_workspace_bytes(...) bytes, the caller's; nothing is allocated inside the call.  Refused with
 * PARSEQ_E_INVALID before any device work: dec_depth > 1 (its per-layer content cache would need re-parenting), a ViTSTR model, a width
 * or batch outside the ranges above, a short workspace. */
#define PARSEQ_BEAM_MAX_WIDTH 16
typedef struct parseq_beam_trace {
    float* logits;
    int32_t* tokens_in;
    int32_t* parent;
    float* score;
} parseq_beam_trace;
size_t parseq_beam_workspace_bytes(const parseq_plan* p, int batch, int beam_width, int num_steps);
int parseq_forward_beam(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps,
                        int32_t* tokens_out, float* scores_out, int32_t* lengths_out, uint8_t* finished_out,
                        const parseq_beam_trace* trace, void* workspace, size_t workspace_bytes, void* stream);
/* One selection step alone on caller tensors (tests/test_beam.py), in place: logits fp32 [batch * W][C] of step `step`; tokens int32
 * [batch * W][ldt] histories (step + 1 <= ldt <= 64; position step + 1 is written when it exists), scores fp32, finished uint8, lengths
 * int32 [batch * W]; parent_out (may be NULL) and picked_out int32 [batch * W]: each new beam's parent (-1: dead) and the class it
 * picked (pad_id for a finished carry or a dead slot). */
int parseq_op_beam_step(const float* logits, int batch, int beam_width, int C, int step, int32_t* tokens, int ldt, float* scores,
                        uint8_t* finished, int32_t* lengths, int32_t* parent_out, int32_t* picked_out, int eos_id, int pad_id,
                        void* stream);

/* ---- lexicon-constrained beam search (pure additions under ABI 15; DESIGN.md section 19 defines it) ------------------ */

/* parseq_forward_beam over a lexicon: the search offers only candidates that are still a prefix of a word, and changes no number — a
 * score stays the model's log-probability of the reading (the log-soft-max runs over all C classes, nothing is renormalised).
 *   trie_next  device int32 [trie_nodes][C], C = num_tokens - 2 head classes: next[n][c] >= 0 is the child of node n along class c;
 *              next[n][eos_id] >= 0 says a word ends at n and is its word id; any negative entry is "not allowed".  Several tries may
 *              share the table (a forest).  The contents are the caller's: a child id >= trie_nodes is treated as not allowed
 *   roots      device int32 [batch], each image's root node, or NULL: node 0 for every image.  A root outside [0, trie_nodes) starts its
 *              image with every beam dead
 *   words_out  device int32 [batch, W]: the word id of each finished hypothesis, -1 otherwise (unfinished or dead)
 * Every other argument, output and refusal is parseq_forward_beam's; also refused: a NULL table or words_out, trie_nodes < 1.  A word of
 * more than num_steps - 1 characters cannot finish and comes back with finished 0.  If the trie under an image's root holds at most W
 * words no candidate is ever dropped: the finished results are that lexicon, ranked by teacher-forced log-probability.
 * workspace: parseq_beam_lexicon_workspace_bytes(...) bytes — parseq_beam_workspace_bytes' parts, then node and word int32 [batch * W].
 * No host synchronisation and no allocation inside the call. */
size_t parseq_beam_lexicon_workspace_bytes(const parseq_plan* p, int batch, int beam_width, int num_steps);
int parseq_forward_beam_lexicon(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps,
                                int32_t* tokens_out, float* scores_out, int32_t* lengths_out, uint8_t* finished_out,
                                const parseq_beam_trace* trace, void* workspace, size_t workspace_bytes, void* stream,
                                const int32_t* trie_next, int trie_nodes, const int32_t* roots, int32_t* words_out);
/* parseq_op_beam_step under a lexicon (tests/test_lexicon_beam.py): its arguments, then the table as above and, in place, nodes and
 * words int32 [batch * W]: each beam's trie node (-1 for a dead beam; a live unfinished beam whose node is outside [0, trie_nodes) offers
 * nothing) and the word id of a finished beam (-1 otherwise). */
int parseq_op_beam_step_lexicon(const float* logits, int batch, int beam_width, int C, int step, int32_t* tokens, int ldt, float* scores,
                                uint8_t* finished, int32_t* lengths, int32_t* parent_out, int32_t* picked_out, int eos_id, int pad_id,
                                void* stream, const int32_t* trie_next, int trie_nodes, int32_t* nodes, int32_t* words);

/* ---- cloze refinement of the N-best (pure additions under ABI 15; DESIGN.md section 20 defines it) ------------------- */

/* parseq_forward_beam / parseq_forward_beam_lexicon followed by refine_iters iterations of the model's cloze refinement on every beam:
 * the pass parseq_forward runs on its greedy reading (tgt_in = [<bos>, t[0 .. num_steps - 2]], keys from the first <eos> on padded, the
 * cloze mask, all num_steps positions at once against the row's image memory) gives logits R[row][i][c]; lp = log_softmax(R[row][i]).
 *   PARSEQ_BEAM_REFINE_SCORE  every hypothesis keeps its tokens and gets the pseudo-log-likelihood sum_{i <= last} lp[i][t[i]] as its score,
 *                             last = its <eos> position, or num_steps - 1 without one.  refine_iters must be 1 (it is idempotent)
 *   PARSEQ_BEAM_REFINE_EDIT   every hypothesis becomes the arg-max reading of R cut at its first <eos> (pad_id after it), scored by the
 *                             sum of its log-max-probabilities; of equal readings of one image the best-scored (then the lower row) stays,
 *                             the others become dead beams.  Every iteration runs on the previous one's readings.  Refused under a lexicon
 * Then the beams of an image are ranked again: higher new score, then the lower previous rank, dead beams last.  Outputs as
 * parseq_forward_beam's, scores_out the new scores, plus
 *   ar_scores_out  fp32 [batch, W]  the score the search itself gave the hypothesis each output row descends from
 * trie_next = NULL: unconstrained (trie_nodes, roots and words_out are ignored); otherwise parseq_forward_beam_lexicon's arguments, the
 * words following their rows.  refine_trace: NULL, or two nullable device pointers filled per iteration.
 * workspace: parseq_beam_refine_workspace_bytes(..., lexicon = 0 / 1) bytes: the parts of parseq_beam_workspace_bytes (and the lexicon's),
 * then, each on a 256-byte boundary, the refinement logits fp32 [batch * W][num_steps][C], three statistics arrays [batch * W][num_steps]
 * (fp32 lp of the row's token, int32 arg-max class, fp32 its lp) and the search's scores fp32 [batch * W].
 * Refused with PARSEQ_E_INVALID before any device work, outputs untouched: whatever parseq_forward_beam(_lexicon) refuses, an unknown
 * mode, EDIT with a trie, SCORE with refine_iters != 1, refine_iters < 1, a short or misaligned workspace, a NULL ar_scores_out.
 * No host synchronisation and no allocation inside the call. */
#define PARSEQ_BEAM_REFINE_SCORE 1
#define PARSEQ_BEAM_REFINE_EDIT 2
typedef struct parseq_beam_refine_trace {
    int32_t* tokens_in;      /* int32 [refine_iters][batch * W][num_steps]     the tgt_in rows the iteration ran on */
    float* logits;           /* fp32  [refine_iters][batch * W][num_steps][C]  the iteration's refinement logits */
} parseq_beam_refine_trace;
size_t parseq_beam_refine_workspace_bytes(const parseq_plan* p, int batch, int beam_width, int num_steps, int lexicon);
int parseq_forward_beam_refine(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps,
                               int32_t* tokens_out, float* scores_out, int32_t* lengths_out, uint8_t* finished_out,
                               const parseq_beam_trace* trace, void* workspace, size_t workspace_bytes, void* stream,
                               const int32_t* trie_next, int trie_nodes, const int32_t* roots, int32_t* words_out, int refine_mode,
                               int refine_iters, float* ar_scores_out, const parseq_beam_refine_trace* refine_trace);
/* The selection of one iteration alone on caller tensors (tests/test_beam_refine.py), in place: logits fp32 [batch * W][L][C]; the beam
 * state as parseq_op_beam_step leaves it — tokens int32 [batch * W][ldt] (<bos>, then token i at position i + 1; L <= ldt <= 64, with
 * L == ldt the last token is picked[row]), scores, finished, lengths, picked; nodes and words (either may be NULL) and ar_scores travel
 * with their rows.  A dead row comes out with score -inf, length 0, finished 0, word -1 and pad_id in picked and after <bos>.
 * workspace: parseq_op_beam_refine_workspace_bytes(batch, beam_width, L) device bytes (0: a shape outside the ranges). */
size_t parseq_op_beam_refine_workspace_bytes(int batch, int beam_width, int L);
int parseq_op_beam_refine(const float* logits, int batch, int beam_width, int C, int L, int refine_mode, int32_t* tokens, int ldt,
                          float* scores, uint8_t* finished, int32_t* lengths, int32_t* picked, int32_t* nodes, int32_t* words,
                          float* ar_scores, int eos_id, int pad_id, void* workspace, size_t workspace_bytes, void* stream);

/* ---- character localisation (pure additions under ABI 15; DESIGN.md section 21 defines it) --------------------------- */

/* The map of a reading: ONE decoder pass over all ctx_len positions, set up as the refinement iteration of parseq_forward sets it up
 * (model.py:154-167: content `tokens`, the cloze query mask, keys from each row's first <eos> on padded), whose last-layer cross-attention
 * probabilities of the query stream are averaged over the heads (the reference's `ca_weights`, modules.py:74-79):
 *   A[b][i][t] = mean_h softmax_t(q[b][h][i] . K[b][h][t] / sqrt(32))        t < S = the encoder's patch tokens
 *   tokens            device int32 [batch, ctx_len]: the content rows [<bos>, reading], as for parseq_decode_logits; 2 <= ctx_len <=
 *                     max_label_length + 1.  It attends to the memory of the most recent parseq_encode / parseq_forward / parseq_set_memory
 *   key_padding_mask  device uint8 [batch, ctx_len], or NULL: derived on the device, (an <eos> at a content position <= j)
 *   attn_out          device fp32 [batch, ctx_len, S].  Row i of image b sums to 1 where key_padding_mask[b][i] is clear — the positions
 *                     0 .. len(b) of the reading, its <eos> included — and is written as zeros elsewhere
 *   logits_out        device fp32 [batch, ctx_len, num_tokens - 2] of the same pass, or NULL
 * Scores, soft-max and head mean are fp32 in every precision, heads summed in ascending order (deterministic).  No allocation, no host
 * synchronisation.  Refused with PARSEQ_E_INVALID before any device work, outputs untouched: a ViTSTR model (no decoder), dec_depth != 1,
 * ctx_len outside [2, max_label_length + 1], a batch that is not the last encode's, NULL plan / tokens / attn_out. */
int parseq_decode_attention(parseq_plan* p, const int32_t* tokens, int batch, int ctx_len, const uint8_t* key_padding_mask, float* attn_out,
                            float* logits_out, void* stream);
/* The geometry of any map on caller tensors (tests/test_attn_map.py).  attn fp32 [batch, L, gh * gw]; token t is cell (t / gw, t % gw) of
 * ph x pw pixels with centre x_c = (c + 1/2) pw, y_r = (r + 1/2) ph; lengths int32 [batch]: row i of image b is valid iff i <= lengths[b].
 *   centres    fp32 [batch, L, 2]  (sum A x_c, sum A y_r)
 *   boxes      fp32 [batch, L, 4]  (cx - hx, cy - hy, cx + hx, cy + hy) clipped to [0, gw pw] x [0, gh ph], hx = sqrt(3 var_x),
 *                                  var_x = sum A (x_c - cx)^2 + pw^2 / 12 (two passes), the same in y: the uniform distribution of that variance
 *   peak       int32 [batch, L]    the arg-max token, lowest index on ties;  peak_mass fp32 [batch, L]  its probability
 * Invalid rows: zeros, peak -1. */
int parseq_op_attention_geometry(const float* attn, const int32_t* lengths, int batch, int L, int gh, int gw, int ph, int pw, float* centres,
                                 float* boxes, int32_t* peak, float* peak_mass, void* stream);
/* Read and localise in one call, no host synchronisation, no allocation: the encoder; then, with tokens_in NULL, the model's own reading —
 * parseq_forward with `flags` (PARSEQ_FLAG_DECODE_AR, PARSEQ_FLAG_LATENCY; the early exit never applies) and `refine_iters`, tokens by arg-max on
 * the device; then the map pass over all L = max_label_length + 1 positions; then the geometry in pixels of the model's input.
 *   tokens_in    NULL, or device int32 [batch, L]: readings to align instead (characters, <eos>, anything after it)
 *   tokens_out   device int32 [batch, L]: the reading that was localised — its characters, <eos> at position lengths_out[b], pad_id after
 *   lengths_out  device int32 [batch]: its number of characters;  attn_out fp32 [batch, L, S];  the rest as parseq_op_attention_geometry
 *   workspace    device, parseq_localize_workspace_bytes(p, batch) bytes (0: refused, parseq_last_error says why), 16-byte aligned
 * Refusals as parseq_decode_attention's, plus whatever parseq_forward refuses, a NULL output and a short workspace. */
size_t parseq_localize_workspace_bytes(const parseq_plan* p, int batch);
int parseq_localize(parseq_plan* p, const void* images, int images_dtype, int batch, const int32_t* tokens_in, int flags, int refine_iters,
                    int32_t* tokens_out, int32_t* lengths_out, float* attn_out, float* centres_out, float* boxes_out, int32_t* peak_out,
                    float* peak_mass_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- lexicon matching (pure additions under ABI 15; DESIGN.md section 23 defines it) --------------------------------- */

/* The n words of a list nearest to every reading in Levenshtein distance (unit costs), on caller tensors (tests/test_lexicon_match.py),
 * ordered by (distance, word id) ascending.  All integer arithmetic; the result is the same for every crops_per_block.
 *   readings   device int32 [batch, ldt], 1 <= ldt <= 32; lengths device int32 [batch] or NULL (= ldt).  Reading b is its first
 *              min(lengths[b], ldt) ids up to the first eos_id, none of them included; an empty reading is legal; an id outside [0, C)
 *              equals no character of any word
 *   table      device, 16-byte aligned, n_rows rows of PARSEQ_LEXICON_ROW_BYTES bytes, one word each: bytes 0 .. 30 its class ids (< C <= 256),
 *              byte 31 its length (1 .. 31).  Row order is the order of the ties: rows ascend in word id
 *   row_ids    device int32 [n_rows] or NULL: the word id of every row (NULL: the row index)
 *   ranges     device int32 [batch, 2] or NULL: crop b is matched against rows [begin, end) only, clipped to the table; begin >= end: an
 *              empty list
 *   fold       device int32 [C] or NULL: every id of a reading inside [0, C) goes through this map before it is compared (the rows of a
 *              case-folded table went through it on the host)
 *   n          1 .. PARSEQ_BEAM_MAX_WIDTH;  crops_per_block: 0 (the library's choice) or how many crops one workgroup walks
 *   word_ids_out, distances_out   device int32 [batch, n]; a slot beyond the list holds -1 and PARSEQ_LEXICON_MATCH_DEAD
 *   workspace  device, parseq_op_lexicon_match_workspace_bytes(batch, n_rows, n) bytes (0: a shape outside the ranges), 16-byte aligned
 * Refused with PARSEQ_E_INVALID before any device work: a NULL or empty table, more than 2^26 rows, shapes outside the ranges above. */
#define PARSEQ_LEXICON_ROW_BYTES 32
#define PARSEQ_LEXICON_MATCH_DEAD 0x7FFFFFFF
size_t parseq_op_lexicon_match_workspace_bytes(int batch, int n_rows, int n);
int parseq_op_lexicon_match(const int32_t* readings, int ldt, const int32_t* lengths, int batch, const uint8_t* table, int n_rows,
                            const int32_t* row_ids, const int32_t* ranges, const int32_t* fold, int C, int eos_id, int n, int crops_per_block,
                            int32_t* word_ids_out, int32_t* distances_out, void* workspace, size_t workspace_bytes, void* stream);
/* Read freely, match, rescore — one call, no host synchronisation, no allocation, for a PARSeq model of dec_depth 1 in every plan precision:
 * the encoder; the reading parseq_forward gives with `flags` (PARSEQ_FLAG_DECODE_AR, PARSEQ_FLAG_LATENCY; the early exit never applies) and
 * `refine_iters` over all L = max_label_length + 1 positions, arg-max on the device; the match above against `table`; then W = n (+ 1 with
 * keep_reading) hypotheses per crop as a beam state — a word's own characters (table_own), <eos>, pad_id — which, with rescore != 0, get
 * parseq_forward_beam_refine's PARSEQ_BEAM_REFINE_SCORE pass: the pseudo-log-likelihood as score, ranked by it, ties by (distance, word id).
 * Without rescore the order is (distance, word id) and a live hypothesis' score is 0.
 *   keep_reading   the reading itself competes: word id -1, distance 0, first in (distance, id) order; unfinished when its L positions hold no
 *                  <eos>.  It is dead when a word has distance 0 (it is that word)
 *   table_own      the rows whose characters are scored, NULL = table (a case-folded table matches on folded ids and scores the words' own)
 * Outputs, device, W per crop: tokens_out int32 [batch, W, L], scores_out fp32, lengths_out int32, finished_out uint8, words_out int32 (the word id,
 * -1: none) as parseq_forward_beam_lexicon's; distances_out int32 [batch, W]; a dead slot (beyond the list; a word of more than
 * max_label_length characters) has score -inf, word -1, distance PARSEQ_LEXICON_MATCH_DEAD, pad_id tokens and sorts last.  reading_tokens_out int32
 * [batch, L]: the arg-max of every position; reading_lengths_out int32 [batch]: the index of its first <eos> (L: none).
 * workspace: parseq_forward_lexicon_match_workspace_bytes(p, batch, args) device bytes (0: refused, parseq_last_error says why), 16-byte
 * aligned.  Afterwards the plan's cached memory K / V are the replicated batch's (rescore) or the batch's.
 * Refused with PARSEQ_E_INVALID before any device work, outputs untouched: a ViTSTR model, dec_depth > 1, n outside [1, PARSEQ_BEAM_MAX_WIDTH -
 * keep_reading], batch * W above the plan's max_batch, a NULL or empty table, more than 256 classes, whatever parseq_forward refuses, a
 * NULL output, a short or misaligned workspace. */
typedef struct parseq_lexicon_match_args {
    const uint8_t* table;        /* the rows that are matched */
    const uint8_t* table_own;    /* the rows that are scored, or NULL */
    const int32_t* row_ids;      /* [n_rows] or NULL */
    const int32_t* ranges;       /* [batch, 2] or NULL */
    const int32_t* fold;         /* [num_tokens - 2] or NULL */
    int32_t n_rows, n, rescore, keep_reading;
} parseq_lexicon_match_args;
size_t parseq_forward_lexicon_match_workspace_bytes(const parseq_plan* p, int batch, const parseq_lexicon_match_args* args);
int parseq_forward_lexicon_match(parseq_plan* p, const void* images, int images_dtype, int batch, int flags, int refine_iters,
                                 const parseq_lexicon_match_args* args, int32_t* tokens_out, float* scores_out, int32_t* lengths_out,
                                 uint8_t* finished_out, int32_t* words_out, int32_t* distances_out, int32_t* reading_tokens_out,
                                 int32_t* reading_lengths_out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- orientation-robust reading (pure additions under ABI 15; DESIGN.md section 27 defines it) ----------------------- */

/* The best of K turned views of every crop, chosen on the device.  Rows b K .. b K + K - 1 of `logits` (fp32 [batch * views, L, C]) are the
 * views of crop b.  parseq_postprocess' kernel runs on all rows; the key of a view is, in fp64 and with n = min(length + 1, L),
 *   s = sum_{i < n} log((double)p_i) added in position order (p_i the fp32 probability parseq_postprocess gives position i),
 *   PARSEQ_ORIENT_SUM: s (the log of the confidence's product)      PARSEQ_ORIENT_MEAN: s / n
 * plus (double)prior[k] when prior (device fp32 [views]) is not NULL; a NaN key counts as -inf and is stored as -inf.  The winner is the
 * first view of the largest key (view 0 when every key is -inf).
 *   images, images_out   NULL together, or device [batch * views, image_elems] and [batch, image_elems] of images_dtype (PARSEQ_F32,
 *                        PARSEQ_BF16 or PARSEQ_U8): the winner's crop is copied beside its logits; no alignment is asked of either
 *   view_out             int32 [batch]              keys_out   fp64 [batch, views]
 *   logits_out           fp32 [batch, L, C]: the winner's rows, bit for bit
 *   ids_out, lengths_out, confidence_out   int32 [batch, L], int32 [batch], fp32 [batch]: exactly what parseq_postprocess writes for the winner
 *   workspace            device, parseq_op_orient_select_workspace_bytes(batch, views, L) bytes (0: a shape outside the ranges), 16-byte aligned
 * Two launches, no host synchronisation.  Refused with PARSEQ_E_INVALID before any device work, outputs untouched: views outside
 * 1 .. PARSEQ_ORIENT_MAX_VIEWS, L outside 1 .. 64, batch * views above 2^26, an eos_id outside [0, C), an unknown criterion, only one of images
 * and images_out, a NULL output, a short or misaligned workspace. */
#define PARSEQ_ORIENT_MAX_VIEWS 8
enum parseq_orient_criterion { PARSEQ_ORIENT_MEAN = 0, PARSEQ_ORIENT_SUM = 1 };
size_t parseq_op_orient_select_workspace_bytes(int batch, int views, int L);
int parseq_op_orient_select(const float* logits, int batch, int views, int L, int C, int eos_id, const void* images, int images_dtype,
                            int64_t image_elems, int criterion, const float* prior, int32_t* view_out, double* keys_out, float* logits_out,
                            int32_t* ids_out, int32_t* lengths_out, float* confidence_out, void* images_out, void* workspace,
                            size_t workspace_bytes, void* stream);
/* parseq_forward's body on the batch * views rows of `images` (crop-major: row b * views + k is view k of crop b), then the op above on its
 * logits — one call, no host synchronisation, no allocation.  flags: PARSEQ_FLAG_DECODE_AR, PARSEQ_FLAG_LATENCY; all num_steps positions
 * are computed and the early exit never applies (a reading is cut at its <eos>, so readings and confidences are the same without it).
 * images_out (NULL: not wanted) [batch, 3, img_h, img_w] of images_dtype.  workspace: parseq_forward_oriented_workspace_bytes(p, batch,
 * views, num_steps) device bytes (0: refused, parseq_last_error says why), 16-byte aligned.  Afterwards the plan's cached memory K / V are
 * those of the batch * views rows.  Refused with PARSEQ_E_INVALID before any device work, outputs untouched: a ViTSTR model (run
 * parseq_vitstr_forward, then the op), batch * views above the plan's max_batch, views outside 1 .. PARSEQ_ORIENT_MAX_VIEWS, an unknown
 * criterion, whatever parseq_forward refuses, a NULL output, a short or misaligned workspace. */
size_t parseq_forward_oriented_workspace_bytes(const parseq_plan* p, int batch, int views, int num_steps);
int parseq_forward_oriented(parseq_plan* p, const void* images, int images_dtype, int batch, int views, int flags, int refine_iters,
                            int num_steps, int criterion, const float* prior, int32_t* view_out, double* keys_out, float* logits_out,
                            int32_t* ids_out, int32_t* lengths_out, float* confidence_out, void* images_out, void* workspace,
                            size_t workspace_bytes, void* stream);

/* ---- long text lines (pure additions under ABI 15; DESIGN.md section 29 defines it) ---------------------------------- */

/* A text line wider than the model's input is read as overlapping windows, every window one row of a batch, and stitched by position.
 * Rows line_first[l] .. line_first[l + 1] - 1 are the windows of line l, left to right; win[row] = (x0, ww, h): the window is the columns
 * x0 .. x0 + ww - 1 of a source line h pixels high.  In fp64, every product and sum rounded on its own:
 *   X = (double)x0 + (double)cx * ((double)ww / (double)img_w)      Y = (double)cy * ((double)h / (double)img_h)
 *   cut c_k = ((double)x0_{k+1} + (double)(x0_k + ww_k)) / 2        delta = min_sep[l] / 2
 *   1  position i of window k is a candidate when i < clamp(lengths[row], 0, L) and 0 <= tokens[row][i] < C
 *   2  it is kept iff lo_k <= X < hi_k: lo_0 = -inf, hi_{K-1} = +inf, else lo_k = c_{k-1} - delta, hi_k = c_k + delta (a NaN X is dropped)
 *   3  per seam (k, k + 1), on the lists of step 2: the kept characters b of window k + 1 in position order are matched to the kept, not yet
 *      matched character a of window k of the same token and the smallest |X_a - X_b| < min_sep (ties: the lowest position); of a matched
 *      pair b is dropped if !(p_b > p_a), else a; a character is dropped if any seam drops it; min_sep = 0 matches nothing
 *   4  the survivors in (window, position) order
 *   5  confidence = (float)((((1.0 q_0) q_1) .. q_{K-1}) p_eos), q_k the product of window k's surviving probabilities in position order
 *      from 1.0, p_eos the last window's probability at position n = clamp(lengths, 0, L) when n < L, else 1.0
 * Inputs, device: tokens int32 [rows, L], lengths int32 [rows], probs fp32 [rows, L], centres fp32 [rows, L, 2] and boxes fp32 [rows, L, 4]
 * in pixels of the model's input (img_h x img_w), win int32 [rows, 3], line_first int32 [lines + 1], min_sep fp64 [lines].
 * Outputs, device, max_out slots per line: len_out int32 [lines] the true number of survivors (stores stop at max_out); tokens_out int32
 * (padding -1), probs_out fp32, boxes_out fp32 [.., 4] and x_out fp64 in source pixels (padding 0), src_out int32 [.., 2] = (window index in
 * the line, position) (padding -1); confidence_out fp32 [lines].
 * One launch, a workgroup per line, no atomics: bit-identical on any stream.  That line_first ascends with 1 .. PARSEQ_LINE_MAX_WINDOWS
 * windows per line inside [0, rows] and that x0 increases within a line is the caller's contract; a table that breaks it is clamped so that
 * every index stays in bounds.  Refused with PARSEQ_E_INVALID before any device work, outputs untouched: a NULL argument, L outside 1 .. 32,
 * lines < 1, rows < lines, max_out outside 1 .. PARSEQ_LINE_MAX_OUT, C < 1, img_h or img_w < 1. */
#define PARSEQ_LINE_MAX_WINDOWS 64
#define PARSEQ_LINE_MAX_OUT 2048
int parseq_op_stitch_lines(const int32_t* tokens, const int32_t* lengths, const float* probs, const float* centres, const float* boxes, int rows,
                           int L, int C, const int32_t* win, int img_h, int img_w, const int32_t* line_first, int lines, const double* min_sep,
                           int max_out, int32_t* len_out, int32_t* tokens_out, float* probs_out, float* boxes_out, double* x_out,
                           int32_t* src_out, float* confidence_out, void* stream);
/* Read, localise and stitch in one call, no host synchronisation, no allocation: parseq_localize's body with tokens_in NULL on the `rows`
 * windows of `images`, parseq_postprocess' kernel on the logits that leaves in the workspace (probs_out), then the op above.  The per-window
 * outputs tokens_out int32 [rows, L], lengths_out int32 [rows], centres_out, boxes_out are parseq_localize's, probs_out fp32 [rows, L] is
 * parseq_postprocess'; the line_* outputs are the op's.  workspace: parseq_read_lines_workspace_bytes(p, rows) device bytes (0: refused,
 * parseq_last_error says why), 16-byte aligned.  Refusals: parseq_localize's (a ViTSTR model, dec_depth > 1, more than 256 memory tokens, rows
 * above the plan's max_batch, a NULL output, a short or misaligned workspace) and the op's, all before any device work. */
size_t parseq_read_lines_workspace_bytes(const parseq_plan* p, int rows);
int parseq_read_lines(parseq_plan* p, const void* images, int images_dtype, int rows, int flags, int refine_iters, const int32_t* win,
                      const int32_t* line_first, int lines, const double* min_sep, int max_out, int32_t* tokens_out, int32_t* lengths_out,
                      float* probs_out, float* centres_out, float* boxes_out, int32_t* line_len_out, int32_t* line_tokens_out,
                      float* line_probs_out, float* line_boxes_out, double* line_x_out, int32_t* line_src_out, float* line_confidence_out,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- scoring given readings (pure additions under ABI 15; DESIGN.md section 30 defines it) -------------------------- */

/* How likely is THIS string for this crop?  Rows b n .. b n + n - 1 are the candidates of crop b.  A candidate of len characters is the
 * int32 row c_0 .. c_{len-1}, <eos>, then <pad> to L = num_steps entries; a first entry of <pad> is an absent candidate.  A row is invalid
 * when a token before its <eos> lies outside [0, C), when anything but <pad> follows the <eos>, or when it holds no <eos>; the staging
 * kernel turns absent and invalid rows into <bos>, <pad> .. before the decoder sees them, so no table is indexed out of range.
 * The decoder input of a row is <bos>, c_0 .. c_{len-1}, <pad> .., its key padding the <pad> slots, its targets the row itself.  For each of
 * `orders` decoding orders, query_masks (device uint8 [orders, L, L], 1 = masked: generate_attn_masks(perm)[1] of the reference) is the
 * attention mask of the query stream of one teacher-forced decoder pass over all batch * n rows, and with lp = log_softmax(logits):
 *   char_logprobs_out  fp32 [batch, n, orders, L] (NULL: not wanted): lp[i][c_i] for i <= len (i = len: the <eos>), 0 past it and in rows
 *                      that are not valid
 *   order_scores_out   fp32 [batch, n, orders]: the fp32 sum of those terms from 0 in ascending i, the <eos> term always included; a sum
 *                      that is not a number is -inf
 *   scores_out         fp32 [batch, n]: in fp64 with k ascending, PARSEQ_SCORE_MIX: m + log(sum_k exp(s_k - m)) - log(orders), m = max_k s_k
 *                      (the mixture of the orders, a probability); PARSEQ_SCORE_MEAN: (sum_k s_k) / orders.  orders = 1: the order's bits.
 *                      -inf for rows that are not valid
 *   rank_out           int32 [batch, n]: the candidates of a crop best first — the higher key, then the lower index; the key is the score,
 *                      under PARSEQ_SCORE_LENGTH_NORM (double)score / (len + 1).  Rows of score -inf come last.  A permutation of 0 .. n-1
 *   lengths_out, valid_out   int32, uint8 [batch, n]: len and 1, or 0 and 0 for an absent or invalid row
 * The log-soft-max is the expression of parseq_op_beam_refine's statistics, (x - max) - logf(sum expf(x - max)) with the same lane-strided
 * partial sums: given the same logits the terms have the same bits.  No atomics: bit-identical on any stream.
 * parseq_score: encode once, replicate the memory n-fold, then `orders` x (decoder pass, row kernel), then the rank — no allocation, no host
 * synchronisation.  workspace: parseq_score_workspace_bytes(p, batch, n, num_steps, orders) device bytes (0: refused, parseq_last_error says
 * why), 16-byte aligned.  Afterwards the plan's cached memory K / V are the replicated batch's.  Refused with PARSEQ_E_INVALID before any
 * device work, outputs untouched: a NULL argument (char_logprobs_out may be NULL), a ViTSTR model, dec_depth > 1, n outside
 * 1 .. PARSEQ_SCORE_MAX_CANDIDATES, orders outside 1 .. PARSEQ_SCORE_MAX_ORDERS, batch * n above the plan's max_batch, num_steps outside
 * [2, max_label_length + 1], a short or misaligned workspace, unknown flags. */
#define PARSEQ_SCORE_MAX_CANDIDATES 16
#define PARSEQ_SCORE_MAX_ORDERS 16
enum parseq_score_flags { PARSEQ_SCORE_MIX = 0, PARSEQ_SCORE_MEAN = 1, PARSEQ_SCORE_LENGTH_NORM = 2 };
size_t parseq_score_workspace_bytes(const parseq_plan* p, int batch, int n, int num_steps, int orders);
int parseq_score(parseq_plan* p, const void* images, int images_dtype, int batch, const int32_t* candidates, int n, int num_steps,
                 const uint8_t* query_masks, int orders, int flags, float* scores_out, float* order_scores_out, float* char_logprobs_out,
                 int32_t* rank_out, int32_t* lengths_out, uint8_t* valid_out, void* workspace, size_t workspace_bytes, void* stream);
/* The two kernels after the decoder pass, on the caller's tensors.  parseq_op_score_rows: order `order` of `orders` from logits fp32
 * [rows, L, C] (any C), targets int32 [rows, L] (a summed target outside [0, C) gives a term of -inf), lengths int32 [rows] (positions
 * 0 .. lengths are summed), valid uint8 [rows]; it writes order_scores [rows, orders] and char_logprobs [rows, orders, L] (may be NULL) at
 * that order.  parseq_op_score_rank: scores_out and rank_out from order_scores [batch, n, orders], lengths and valid [batch, n]; a NaN in
 * order_scores counts as -inf.  One launch each.  Refused: a NULL argument, L outside 1 .. 64, rows, n or orders outside their ranges, an
 * order outside [0, orders), unknown flags. */
int parseq_op_score_rows(const float* logits, int rows, int L, int C, const int32_t* targets, const int32_t* lengths, const uint8_t* valid,
                         int orders, int order, float* order_scores, float* char_logprobs, void* stream);
int parseq_op_score_rank(const float* order_scores, const int32_t* lengths, const uint8_t* valid, int batch, int n, int orders, int flags,
                         float* scores_out, int32_t* rank_out, void* stream);

/* ---- beam search over a weighted automaton (pure additions under ABI 15; DESIGN.md section 24 defines it) ------------ */

/* parseq_forward_beam_lexicon with a weight on every arc of the table, which then need not be a tree (cycles and shared states are
 * allowed): a word list with frequencies, a character n-gram model or a regular pattern (parseq_amd/automaton.py builds all three).
 *   next       device int32 [states][C], exactly trie_next above; the <eos> column holds a non-negative tag where the state accepts
 *   weight     device fp32 [states][C], the natural-log weight of taking class c from state s (the <eos> column: the final weight).  A
 *              non-finite weight makes its arc not allowed
 *   roots      as above (each image's start state)
 *   alpha, beta   finite: the prior weight and the per-character bonus
 * A beam also carries wsum, the sum of the weights along its path.  A candidate (w, c) of model score m = score[w] + logp[w][c] is
 * ranked by f = m + (alpha (wsum[w] + weight[n][c]) + beta k), k the characters the hypothesis would have (<eos> not counted), every
 * operation rounded to fp32 on its own (a candidate whose f overflows is not allowed); a finished beam carries at score + (alpha wsum + beta length).  Ties as in parseq_forward_beam.
 *   scores_out        the fused value f the ranking used        model_scores_out  fp32 [batch, W] the model's own sum of log-probabilities
 *   priors_out        fp32 [batch, W] wsum (0 for a dead beam)  words_out         the tag of a finished hypothesis, -1 otherwise
 * trace->score holds the fused values.  With alpha = beta = 0 every output equals parseq_forward_beam_lexicon's on the same table; with a
 * one-state table that allows every class at weight 0 and beta = 0, parseq_forward_beam's.
 * Refused before any device work, outputs untouched: whatever parseq_forward_beam_lexicon refuses, a NULL weight, model_scores_out or
 * priors_out, a non-finite alpha or beta.
 * workspace: parseq_beam_automaton_workspace_bytes(...) bytes — parseq_beam_lexicon_workspace_bytes' parts, then wsum fp32 [batch * W]. */
size_t parseq_beam_automaton_workspace_bytes(const parseq_plan* p, int batch, int beam_width, int num_steps);
int parseq_forward_beam_automaton(parseq_plan* p, const void* images, int images_dtype, int batch, int beam_width, int num_steps,
                                  int32_t* tokens_out, float* scores_out, int32_t* lengths_out, uint8_t* finished_out,
                                  const parseq_beam_trace* trace, void* workspace, size_t workspace_bytes, void* stream,
                                  const int32_t* next, const float* weight, int states, const int32_t* roots, float alpha, float beta,
                                  int32_t* words_out, float* model_scores_out, float* priors_out);
/* parseq_op_beam_step under a weighted automaton (tests/test_automaton.py): parseq_op_beam_step_lexicon's arguments with the weights
 * beside the table, then alpha, beta and, in place, wsums fp32 [batch * W]; scores stay the model's sums, fused_out fp32 [batch * W]
 * (may be NULL) receives each new beam's fused value (-inf for a dead slot). */
int parseq_op_beam_step_automaton(const float* logits, int batch, int beam_width, int C, int step, int32_t* tokens, int ldt, float* scores,
                                  uint8_t* finished, int32_t* lengths, int32_t* parent_out, int32_t* picked_out, int eos_id, int pad_id,
                                  void* stream, const int32_t* next, const float* weight, int states, int32_t* nodes, int32_t* words,
                                  float alpha, float beta, float* wsums, float* fused_out);

/* ViTSTR.forward (strhub/models/vitstr/system.py:76-82 -> vitstr/model.py:20-28) for a model created with
 * arch = PARSEQ_ARCH_VITSTR: encoder with class token, head on tokens [1, num_steps], i.e. logits_out fp32
 * [batch, num_steps, num_tokens - 2] with num_steps = min(max_length, max_label_length) + 1.  images as parseq_forward. */
int parseq_vitstr_forward(parseq_plan* p, const void* images, int images_dtype, int batch, int num_steps, float* logits_out,
                          void* stream);

/* ---- input resize ------------------------------------------------------------------- */

/* One RGB image, HWC uint8: `data` is a DEVICE pointer, row_stride in bytes (>= 3 * width). */
typedef struct {
    const uint8_t* data;
    int32_t height, width;
    int64_t row_stride;
} parseq_image_desc;

/* The resize step of the reference's input transform, T.Resize(img_size, BICUBIC) on a PIL image
 * (strhub/data/module.py:77, read.py:41-43): Pillow's 8-bit ImagingResample, bit-exact (double-precision weights, 22-bit
 * fixed point, horizontal pass stored as uint8 before the vertical pass).  images: HOST array of `batch` descriptors
 * (image sizes may differ); out: device uint8 [batch, 3, out_h, out_w] — exactly the PARSEQ_U8 input of parseq_forward /
 * parseq_encode, which applies ToTensor + Normalize(0.5, 0.5) in its patch-embed loader; workspace: device scratch of
 * parseq_resize_workspace_bytes(batch) bytes (the descriptors are copied there on `stream`). */
size_t parseq_resize_workspace_bytes(int batch);
int parseq_resize_bicubic(const parseq_image_desc* images, int batch, int out_h, int out_w, uint8_t* out, void* workspace, void* stream);

/* (ABI 13) The rotation ahead of the resize: `img.rotate(rotation, expand=True)` of the same transform (strhub/data/module.py:72-73, the
 * reference's test.py --rotation), i.e. Pillow's Image.rotate with nearest resampling and black fill, bit-exact.  A descriptor holds the
 * MAP, not an angle — the library does no trigonometry: the caller evaluates Pillow's float64 expressions on the host
 * (parseq_amd/preprocess.py rotation_map; INTEGRATION.md spells them out) and the kernels do 32-bit integer arithmetic only.
 *   mode                    PARSEQ_ROTATE_NONE (a copy), _90 / _180 / _270 (Pillow's exact transposes for those angles; a[] unused), or
 *                           PARSEQ_ROTATE_AFFINE
 *   rot_height, rot_width   size of the rotated image: the source's for NONE / 180, swapped for 90 / 270 (anything else is refused),
 *                           Pillow's expanded canvas for AFFINE
 *   a[6]                    AFFINE: Pillow's 16.16 fixed-point inverse map; pixel (x, y) of the rotated image is source pixel
 *                           ((a[2] + a[0] x + a[1] y) >> 16, (a[5] + a[3] x + a[4] y) >> 16), arithmetic shift, black outside the source
 * No side, source or rotated, may exceed PARSEQ_ROTATE_MAX_SIDE (the sums then fit 32 bits; PARSEQ_E_INVALID otherwise). */
enum { PARSEQ_ROTATE_NONE = 0, PARSEQ_ROTATE_90 = 1, PARSEQ_ROTATE_180 = 2, PARSEQ_ROTATE_270 = 3, PARSEQ_ROTATE_AFFINE = 4 };
#define PARSEQ_ROTATE_MAX_SIDE 16384
typedef struct {
    const uint8_t* data;            /* DEVICE pointer, RGB HWC uint8 */
    int32_t height, width;          /* of the source */
    int64_t row_stride;             /* in bytes, >= 3 * width */
    int32_t mode;
    int32_t rot_height, rot_width;
    int32_t a[6];
} parseq_rotated_image_desc;

/* parseq_resize_bicubic of the ROTATED images, in one launch whatever the batch: the horizontal pass gathers each tap through the image's
 * map straight from the source, so no rotated copy is ever written.  Arguments as parseq_resize_bicubic; workspace of
 * parseq_rotate_resize_workspace_bytes(batch) bytes.  An image in mode PARSEQ_ROTATE_NONE gives parseq_resize_bicubic's bytes. */
size_t parseq_rotate_resize_workspace_bytes(int batch);
int parseq_rotate_resize_bicubic(const parseq_rotated_image_desc* images, int batch, int out_h, int out_w, uint8_t* out, void* workspace,
                                 void* stream);

/* ---- (ABI 14) training augmentation: the reference's RandAugment operators ----------------------------------------- */

/* The operators of rand_augment_transform() (strhub/data/augment.py, aa_overrides.py: timm's auto_augment calls into Pillow) on a ragged
 * batch of RGB uint8 HWC images in device memory, bit-exact with Pillow.  An image carries a chain of up to PARSEQ_AUGMENT_MAX_OPS
 * operators; the chains run stage by stage, one launch per stage for the whole batch, between two per-image regions of the workspace.
 *   PARSEQ_AUG_TABLE         arg.table: a 256-entry table applied to every channel (Invert, Posterize, Solarize, SolarizeAdd, Brightness;
 *                            parseq_amd/augment.py lut_for builds it from Pillow's own steps)
 *   PARSEQ_AUG_AUTOCONTRAST  ImageOps.autocontrast(img)                      (per-channel histogram, table built on the device)
 *   PARSEQ_AUG_EQUALIZE      ImageOps.equalize(img)                          (the same)
 *   PARSEQ_AUG_CONTRAST      ImageEnhance.Contrast(img).enhance(arg.factor)  (rounded mean of convert('L'), table built on the device)
 *   PARSEQ_AUG_COLOR         ImageEnhance.Color(img).enhance(arg.factor)
 *   PARSEQ_AUG_AFFINE        img.transform((out_width, out_height), AFFINE, arg.coef, resample=mode, fillcolor=(128, 128, 128)); mode is
 *                            PARSEQ_AUG_BILINEAR or PARSEQ_AUG_BICUBIC.  ShearX / ShearY / TranslateXRel / TranslateYRel keep the size,
 *                            Rotate (expand=True) carries its expanded size (augment.py rotate_expand_map)
 *   PARSEQ_AUG_TURN          Pillow's exact rotation by 90 / 180 / 270 degrees: mode is PARSEQ_ROTATE_90 / _180 / _270
 *   PARSEQ_AUG_GAUSSIAN_BLUR img.filter(ImageFilter.GaussianBlur(radius)), 0 < radius <= 4, bit-exact with Pillow: three box passes along x,
 *                            then three along y, each out = (ww * (the 2 r + 1 samples around x) + fw * (the two at distance r + 1) + 2^23)
 *                            >> 24 in 32-bit unsigned arithmetic, indices clamped to the line in every pass, rounded to uint8 after every
 *                            pass.  arg.blur = (r, ww, fw) of parseq_amd/augment.py gaussian_box(radius), Pillow's single-precision steps;
 *                            0 <= r <= 3 and (2 r + 1) ww + 2 fw <= 2^24 (more would overflow the sum)
 *   PARSEQ_AUG_POISSON_NOISE imgaug's AdditivePoissonNoise(lam) = AddElementwise(RandomSign(Poisson(lam)), per_channel=False), RESTATED from
 *                            its published definition, not pinned against imgaug: per pixel ONE draw n = +-k, k ~ Poisson(arg.noise.lam),
 *                            both signs equally likely, added to R, G and B, clipped to 0 .. 255.  The generator is Philox4x32-10 with key
 *                            (low, high word of arg.noise.seed) and counter (pixel index y * width + x, 0, 0, 0): word 0 is the uniform u,
 *                            bit 31 of word 1 set means minus; k = the number of thresholds T_j <= u, j = 0 .. 126, T_j = min(floor(C_j
 *                            2^32), 2^32 - 1), C_j = C_(j-1) + p_j, p_(j+1) = (p_j lam) / (j + 1) in float64 without contraction, p_0 =
 *                            arg.noise.p0 = exp(-lam) computed by the caller.  1 <= lam <= 41, p0 finite and in (0, 1).  A pixel's noise
 *                            depends on (seed, index) alone: the same bytes every run
 * out_height / out_width: the image after the operator; every operator but AFFINE and TURN must repeat its input's size.  Factors are
 * finite and >= 0.1, coefficients finite, no side (source or any stage) outside 1 .. PARSEQ_ROTATE_MAX_SIDE.  Every descriptor is checked
 * on the host before anything is launched (PARSEQ_E_INVALID, parseq_last_error names the image and the field).
 * The two last operators came after ABI 14 without a new version: the descriptor's layout is unchanged (both fit the 256 bytes of arg) and
 * an older library refuses them as unknown operators.  The value 9 is no operator and stays refused. */
enum { PARSEQ_AUG_NONE = 0, PARSEQ_AUG_TABLE = 1, PARSEQ_AUG_AUTOCONTRAST = 2, PARSEQ_AUG_EQUALIZE = 3, PARSEQ_AUG_CONTRAST = 4,
       PARSEQ_AUG_COLOR = 5, PARSEQ_AUG_AFFINE = 6, PARSEQ_AUG_TURN = 7, PARSEQ_AUG_GAUSSIAN_BLUR = 8, PARSEQ_AUG_POISSON_NOISE = 10 };
enum { PARSEQ_AUG_BILINEAR = 2, PARSEQ_AUG_BICUBIC = 3 };      /* Pillow's Image.Resampling values */
#define PARSEQ_AUGMENT_MAX_OPS 3

typedef struct {
    int32_t op;                       /* PARSEQ_AUG_* (never NONE inside a chain) */
    int32_t mode;                     /* AFFINE: the resampling filter; TURN: the quarter turn; otherwise 0 */
    int32_t out_height, out_width;
    union {
        uint8_t table[256]; float factor; double coef[6];
        struct { int32_t r; uint32_t ww, fw; } blur;                    /* GAUSSIAN_BLUR: one box pass's radius and 8.24 weights */
        struct { double p0; uint64_t seed; int32_t lam; } noise;        /* POISSON_NOISE: exp(-lam), the Philox key, lam */
    } arg;
} parseq_augment_op;

typedef struct {
    const uint8_t* data;              /* DEVICE pointer, RGB, HWC */
    int32_t height, width;
    int64_t row_stride;               /* bytes between rows (>= 3 * width) */
    int32_t num_ops;                  /* 0 .. PARSEQ_AUGMENT_MAX_OPS; 0 = the image passes unchanged */
    int32_t reserved;
    parseq_augment_op ops[PARSEQ_AUGMENT_MAX_OPS];
} parseq_augment_desc;

/* Bytes of workspace the two calls below need for these descriptors (HOST array): the descriptors' device copy, the plan, and two regions per
 * image of its largest stage.  0 if a descriptor is invalid (parseq_last_error says why). */
size_t parseq_augment_workspace_bytes(const parseq_augment_desc* descs, int batch);

/* Runs every chain, then parseq_resize_bicubic's arithmetic (the same kernel) on the augmented images: out = device uint8
 * [batch, 3, out_h, out_w], no host round trip, no synchronisation inside.  descs: HOST array, copied on `stream` — keep it alive until the
 * stream has passed.  workspace: device memory of at least parseq_augment_workspace_bytes(descs, batch) bytes; workspace_bytes says how
 * much there is (less is refused). */
int parseq_augment_resize_bicubic(const parseq_augment_desc* descs, int batch, int out_h, int out_w, uint8_t* out, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* ---- rectification of quadrilateral text regions ------------------------------------------- */

/* What a caller with a text detector does first: cut every detected quadrilateral out of the scene and straighten it.  A region names one
 * of the call's source images and carries the size of its rectified crop and Pillow's PERSPECTIVE data; any number of regions may name
 * the same image.  The result is, byte for byte, Image.fromarray(src).transform((width, height), Image.PERSPECTIVE, coef, Image.BICUBIC)
 * with fill 0: for output pixel (x, y), X = x + 0.5, Y = y + 0.5, in double precision without contraction and with correctly rounded
 * divisions,
 *     sx = (coef[0] X + coef[1] Y + coef[2]) / (coef[6] X + coef[7] Y + 1),   sy = (coef[3] X + coef[4] Y + coef[5]) / (the same);
 * the pixel stays 0 unless 0 <= sx < width and 0 <= sy < height of the source; otherwise Pillow's bicubic filter (sixteen clamped taps)
 * around (sx - 0.5, sy - 0.5), clipped to 0 .. 255 and truncated.  The library does no geometry: the caller derives the coefficients from
 * its quadrilateral (parseq_amd/preprocess.py quad_coeffs).  Came after ABI 15 without a new version: pure additions.
 * Refused with PARSEQ_E_INVALID before any device work, outputs untouched: an image index outside 0 .. n_images - 1, a side outside
 * 1 .. PARSEQ_ROTATE_MAX_SIDE, a coefficient that is not finite, a denominator coef[6] X + coef[7] Y + 1 that is not > 0 at one of the
 * four corners of the output rectangle (0, 0), (width, 0), (width, height), (0, height) — it is linear, so it is then positive at every
 * pixel —, a source image whose row_stride * height does not fit 31 bits, a workspace that is too small. */
typedef struct {
    int32_t image;                    /* index into the call's images */
    int32_t height, width;            /* of the rectified region */
    double coef[8];
} parseq_region_desc;

/* Bytes of workspace the two calls below need for these regions (HOST array) and n_images source images: the device copies of both
 * arrays, the tile table, the region images of the resize and one slot of 3 * width * height bytes per region (rounded up to 256).
 * 0 if a region's size is out of range (parseq_last_error says why). */
size_t parseq_rectify_workspace_bytes(const parseq_region_desc* regions, int n_regions, int n_images);

/* The rectified regions themselves, one launch for all of them: outs = HOST array of n_regions device pointers, region i written to
 * outs[i] as uint8 [height_i, width_i, 3], dense.  images, regions and outs are copied on `stream`: keep them alive until the stream has
 * passed.  No allocation, no synchronisation inside. */
int parseq_rectify(const parseq_image_desc* images, int n_images, const parseq_region_desc* regions, int n_regions, uint8_t* const* outs,
                   void* workspace, size_t workspace_bytes, void* stream);

/* parseq_rectify into the workspace's slots, then parseq_resize_bicubic's arithmetic (the same kernel) on the rectified regions: out =
 * device uint8 [n_regions, 3, out_h, out_w], the PARSEQ_U8 input of the model, with no host round trip. */
int parseq_rectify_resize_bicubic(const parseq_image_desc* images, int n_images, const parseq_region_desc* regions, int n_regions,
                                  int out_h, int out_w, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* ---- rectification of polygon text regions -------------------------------------------------- */

/* The same step for a detector of curved text: a region is a row of strips side by side, each a box (x0, 0, x1, height) of the output
 * painted through a bilinear map of one source quadrilateral.  The result is, byte for byte,
 * Image.fromarray(src).transform((width, height), Image.MESH, [((x0, 0, x1, height), quad), ...], Image.BICUBIC) with fill 0: for output
 * pixel (x, y) of the strip with x0 <= x < x1, X = (x - x0) + 0.5, Y = y + 0.5, in double precision without contraction, left to right,
 *     sx = coef[0] + coef[1] X + coef[2] Y + coef[3] X Y,   sy = coef[4] + coef[5] X + coef[6] Y + coef[7] X Y;
 * the inside test and the bicubic filter are those of parseq_rectify above.  The library does no geometry: coef is what Pillow derives
 * for QUAD from the strip's box and quadrilateral (parseq_amd/preprocess.py polygon_mesh).  Came after ABI 15 without a new version: pure
 * additions.  Refused with PARSEQ_E_INVALID before any device work, outputs untouched: everything parseq_rectify refuses about images,
 * sizes and the workspace; a coefficient that is not finite; a region with fewer than 1 or more than PARSEQ_MESH_MAX_STRIPS strips; a
 * strip range [first_strip, first_strip + n_strips) outside the strips array; strips that do not tile [0, width) in order without gap
 * or overlap (the first x0 is 0, every x1 > x0, every next x0 the previous x1, the last x1 the width). */
#define PARSEQ_MESH_MAX_STRIPS 64

typedef struct {
    int32_t x0, x1;                   /* the strip's output columns x0 .. x1 - 1 */
    double coef[8];
} parseq_mesh_strip;

typedef struct {
    int32_t image;                    /* index into the call's images */
    int32_t height, width;            /* of the rectified region */
    int32_t first_strip, n_strips;    /* its strips in the call's strips array, left to right */
} parseq_mesh_region_desc;

/* Bytes of workspace the two calls below need: what parseq_rectify_workspace_bytes counts, and the device copy of the n_strips strips.
 * 0 if a region's size is out of range (parseq_last_error says why). */
size_t parseq_mesh_rectify_workspace_bytes(const parseq_mesh_region_desc* regions, int n_regions, const parseq_mesh_strip* strips, int n_strips,
                                           int n_images);

/* parseq_rectify for strips: region i written to outs[i] as uint8 [height_i, width_i, 3], dense, one launch for all regions.  images,
 * regions, strips and outs are HOST arrays copied on `stream`: keep them alive until the stream has passed.  No allocation, no
 * synchronisation inside. */
int parseq_mesh_rectify(const parseq_image_desc* images, int n_images, const parseq_mesh_region_desc* regions, int n_regions,
                        const parseq_mesh_strip* strips, int n_strips, uint8_t* const* outs, void* workspace, size_t workspace_bytes, void* stream);

/* parseq_mesh_rectify into the workspace's slots, then parseq_resize_bicubic's arithmetic (the same kernel): out = device uint8
 * [n_regions, 3, out_h, out_w]. */
int parseq_mesh_rectify_resize_bicubic(const parseq_image_desc* images, int n_images, const parseq_mesh_region_desc* regions, int n_regions,
                                       const parseq_mesh_strip* strips, int n_strips, int out_h, int out_w, uint8_t* out, void* workspace,
                                       size_t workspace_bytes, void* stream);

/* ---- post-processing --------------------------------------------------------------- */

/* Numeric half of `preds, probs = tokenizer.decode(logits.softmax(-1))` (strhub/models/base.py:132-137,
 * strhub/data/utils.py:79-99 greedy max per position, :120-129 truncation at the first EOS) on the device, so a caller
 * moves B*L ids + B lengths (+ probabilities) to the host instead of B*L*C probabilities and one .tolist() per row.
 * logits: device fp32 [batch, L, C] contiguous (L <= 64).  Outputs (device):
 *   ids_out      int32 [batch, L]  arg-max class per position (first maximum), for every position.  A position whose logits hold a NaN
 *                                  or a +inf, or nothing but -inf, has no finite soft-max: its id is 0 and its probability NaN, which is
 *                                  what the reference's `max` over NaN probabilities returns (so the label is cut there if eos_id is 0)
 *   lengths_out  int32 [batch]     index of the first position whose id is eos_id, or L: the label is ids_out[b, :len]
 *   probs_out    fp32  [batch, L]  max soft-max probability per position (NULL to skip); the reference's per-label
 *                                  probability tensor is probs_out[b, :min(len + 1, L)] (it keeps the EOS probability)
 *   confidence_out fp32 [batch]    product of that tensor (base.py:137), NULL to skip */
int parseq_postprocess(const float* logits, int batch, int L, int C, int eos_id, int32_t* ids_out, int32_t* lengths_out,
                       float* probs_out, float* confidence_out, void* stream);

/* Validation loss of strhub/models/base.py:194-201 (CrossEntropySystem.forward_logits_loss):
 * F.cross_entropy(logits.flatten(end_dim=1), targets.flatten(), ignore_index) with mean reduction, and the number of
 * non-ignored targets.  logits: device fp32 [rows, C]; targets: device int32 [rows] (class index or ignore_index);
 * loss_out / numel_out: device scalars; workspace: device, `rows` floats.  Deterministic (fixed summation order). */
int parseq_cross_entropy(const float* logits, const int32_t* targets, int rows, int C, int ignore_index, float* loss_out,
                         int32_t* numel_out, float* workspace, void* stream);

/* (ABI 11) The per-sample loop of BaseSystem._eval_step (strhub/models/base.py:132-143) on the device: greedy decode, test-charset
 * adapter, edit distance, exact match and the running totals the reference's test.py:115-126 sums on the host — nothing is copied back,
 * nothing is allocated, the call does not synchronise.
 *   logits         device fp32 [batch, L, C] contiguous, L <= 32 (max_label_length + 1)
 *   adapter_table  device int32 [C]: the Unicode code point CharsetAdapter (strhub/data/utils.py:26-43) turns train token id into, or
 *                  -1 for a token it drops (the entry of eos_id is never read)
 *   gt, gt_len     device int32 [batch, gt_width] code points of the labels (any padding) and int32 [batch] their lengths;
 *                  1 <= gt_width <= PARSEQ_EVAL_MAX_GT, a wider array is refused with PARSEQ_E_INVALID; lengths are clamped to gt_width
 *   ids_out, lengths_out, confidence_out   int32 [batch, L], int32 [batch], fp32 [batch]: exactly what parseq_postprocess writes
 *                  for these logits (the same kernel runs first)
 *   rows_out       int32 [batch, 4]: length of the adapted prediction, length of the label, Levenshtein distance between them (unit
 *                  costs, no transpositions: nltk.edit_distance's defaults, base.py:138), 1 if they are equal else 0
 *   workspace      device, `batch` doubles (each row's distance / max(len(pred), len(gt), 1))
 *   accum          device, PARSEQ_EVAL_ACCUM_BYTES: int64 num_samples, correct, label_length; double ned, confidence — ACCUMULATED
 *                  into (zero it to start an evaluation).  The batch is summed in a fixed order by one workgroup, so equal inputs give
 *                  bit-identical totals; calls that share an accumulator must be ordered (one stream). */
#define PARSEQ_EVAL_MAX_GT 256
#define PARSEQ_EVAL_ACCUM_BYTES 40
int parseq_eval_metrics(const float* logits, int batch, int L, int C, int eos_id, const int32_t* adapter_table, const int32_t* gt,
                        const int32_t* gt_len, int gt_width, int32_t* ids_out, int32_t* lengths_out, float* confidence_out,
                        int32_t* rows_out, double* workspace, void* accum, void* stream);

/* The same for an N-best: the metrics of the first live hypothesis of every image, and where in the list the label stands.  Nothing is
 * copied back or allocated, the call does not synchronise and uses no atomics (fixed summation order: equal inputs, bit-identical totals).
 *   tokens, scores, lengths   device int32 [B, W, T], fp32 [B, W], int32 [B, W]: a beam result.  A slot is LIVE iff its score is not -inf;
 *                  its live rank is the number of live slots before it in its image.  A hypothesis is its first lengths[b, w] tokens
 *                  (clamped to [0, min(T, 32)]) mapped through adapter_table; ids outside [0, C) and entries -1 are dropped.
 *   conf_scores    device fp32 [B, W]: the log-probability the confidence exp((double)conf_scores[b, w]) of the top-1 is taken from
 *                  (`scores` itself, or the model's own scores under a weighted automaton)
 *   gt, gt_len, G, adapter_table   as parseq_eval_metrics takes them; the W hypotheses of image b share label b
 *   hyp_rows_out   int32 [B * W, 4]: {length of the adapted hypothesis, length of the label, Levenshtein distance, 1 if equal}; a dead
 *                  slot's row is {-1, -1, -1, 0}
 *   image_rows_out int32 [B, 8]: {m, n, distance, exact} of the top-1 (the first live slot; an image without one reads as the empty
 *                  string: m 0, distance n, not exact), live rank of the first exact live hypothesis or -1, smallest distance over the live
 *                  slots, number of live slots, slot of the top-1 or -1
 *   workspace      device, B * (W + 3) doubles: distance / max(m, n, 1) of every hypothesis (-1 for a dead slot), then per image the
 *                  top-1's, the smallest over the live slots, and the confidence
 *   accum          device, PARSEQ_EVAL_BEAMS_ACCUM_BYTES, ACCUMULATED into: int64 num_samples, correct, label_length, top1_distance,
 *                  oracle_correct, oracle_distance, live, miss, first_hit[PARSEQ_EVAL_MAX_BEAMS]; double ned, confidence, oracle_ned.
 *                  Calls that share an accumulator must be ordered (one stream).
 * The per-image step and the sums run in ONE workgroup: its time grows linearly with B on one compute unit (12 us at B = 512); split a
 * far larger batch into several calls, the accumulator adds up.
 * PARSEQ_E_INVALID, before any device work and with every output untouched: W outside 1 .. PARSEQ_EVAL_MAX_BEAMS, T outside 1 .. 32,
 * G outside 1 .. PARSEQ_EVAL_MAX_GT, B < 1 (or above 2^26), C < 1, a null pointer. */
#define PARSEQ_EVAL_MAX_BEAMS 17
#define PARSEQ_EVAL_BEAMS_ACCUM_BYTES 224
int parseq_eval_beams(const int32_t* tokens, const float* scores, const int32_t* lengths, const float* conf_scores, int B, int W, int T, int C,
                      const int32_t* adapter_table, const int32_t* gt, const int32_t* gt_len, int G, int32_t* hyp_rows_out,
                      int32_t* image_rows_out, double* workspace, void* accum, void* stream);

/* Error analysis: HOW the greedy readings are wrong.  For every sample the canonical edit script between the adapted
 * prediction p[0..m) (ids cut at `lengths`, mapped through adapter_table, dropped characters removed: what parseq_eval_metrics compares) and
 * the label g[0..n), and integer tables summed over the batch.  One launch on the caller's stream, no allocation, no synchronisation.
 *   ids, lengths   device int32 [batch, L], int32 [batch]: what parseq_eval_metrics or parseq_postprocess wrote; 1 <= L <= 32.  Lengths
 *                  are clamped to [0, L], ids outside [0, C) are dropped
 *   adapter_table  device int32 [C], as parseq_eval_metrics takes it
 *   symbols        device int32 [num_symbols], STRICTLY ASCENDING (the caller's contract: the table lies in device memory and is not
 *                  checked): the distinct non-negative code points of adapter_table, T = num_symbols of them.  Index T stands for a label
 *                  code point outside the set ("other"), T + 1 for the missing side of an insertion or a deletion ("none")
 *   gt, gt_len, gt_width   as parseq_eval_metrics takes them
 *   script_out     int8 [batch, PARSEQ_EVAL_SCRIPT_WIDTH]: the script in forward order, padded with -1.  Codes: 0 match, 1 substitution,
 *                  2 insertion (a predicted character that answers to no label character), 3 deletion (a label character nothing was
 *                  predicted for).  With D the unit-cost Levenshtein table (D[i][0] = i, D[0][j] = j) the script is read from (m, n) back
 *                  to (0, 0), at (i, j) by the first rule that holds: (1) i, j > 0 and D[i-1][j-1] + (p[i-1] != g[j-1]) == D[i][j]: match
 *                  or substitution, to (i-1, j-1); (2) i > 0 and D[i-1][j] + 1 == D[i][j]: insertion, to (i-1, j); (3) deletion, to (i, j-1)
 *   script_len_out int32 [batch]: codes of each script (at most m + n)
 *   rows_out       int32 [batch, 4]: {m, n, distance, exact}, equal to parseq_eval_metrics' rows for the same input
 *   accum          device, parseq_eval_errors_accum_bytes(num_symbols) bytes of int64, ACCUMULATED into (zero it to start):
 *                  head[8] = {samples, matches, substitutions, insertions, deletions, exact, 0, 0};
 *                  by_length[33][4], row min(n, 32) = {samples, exact, distance, label characters};
 *                  by_position[33][4], row min(j, 32) with j the label characters before the operation = {label characters at that
 *                  position, substitutions, deletions, insertions};
 *                  confusion[T + 2][T + 2], row = label symbol (or none), column = predicted symbol (or none); matches lie on the diagonal.
 *                  Integer atomic adds only: equal inputs give bit-identical totals in any order, on any stream.
 * PARSEQ_E_INVALID, before any device work and with outputs and accumulator untouched: a null pointer, batch < 1, L outside 1 .. 32, C < 1,
 * gt_width outside 1 .. PARSEQ_EVAL_MAX_GT, num_symbols outside 1 .. PARSEQ_EVAL_MAX_SYMBOLS. */
#define PARSEQ_EVAL_MAX_SYMBOLS 512
#define PARSEQ_EVAL_SCRIPT_WIDTH 288 /* PARSEQ_EVAL_MAX_GT + 32 */
size_t parseq_eval_errors_accum_bytes(int num_symbols); /* 0 outside 1 .. PARSEQ_EVAL_MAX_SYMBOLS */
int parseq_eval_errors(const int32_t* ids, const int32_t* lengths, int batch, int L, int C, const int32_t* adapter_table,
                       const int32_t* symbols, int num_symbols, const int32_t* gt, const int32_t* gt_len, int gt_width,
                       int8_t* script_out, int32_t* script_len_out, int32_t* rows_out, void* accum, void* stream);

/* ---- "next" row N3: training step, decoder side (strhub/models/parseq/system.py:168-199 + loss.backward()) ---------- */

/* Offset (in floats) of parameter `index` inside a gradient buffer, and the buffer's length: gradients are laid out like
 * the model's fp32 master weights, every tensor starting at a multiple of 8 floats.  -1 for a bad index. */
int64_t parseq_model_param_offset(const parseq_model* m, int index);
int64_t parseq_model_grad_elems(const parseq_model* m);
/* Arithmetic of the training step's matrix products (reference: `precision: bf16-mixed`, /root/reference/train.py:62-64):
 * PARSEQ_F32 (default) = exact fp32 products on v_mfma_f32_16x16x4_f32; PARSEQ_BF16 = both operands of every aligned Linear
 * product (forward, dX, dW) rounded to bfloat16 on their way into LDS, fp32 accumulate, fp32 master weights / activations /
 * gradients in memory.  Attention products, LayerNorm, soft-max, loss and the optimiser stay fp32 in both modes.
 * (ABI 15) PARSEQ_BF16X3 = the same Linear products with both operands SPLIT into bf16 pairs hi = bf16(v), lo = bf16(v - hi) on their
 * way into LDS and evaluated as lo*hi + hi*lo + hi*hi (three bf16 MFMAs, fp32 accumulate): within 3 * 2^-16 sum |a||b| of the exact
 * product.  Everything else — attention, workspace layout and sizes, kernel routes — is the PARSEQ_F32 mode's. */
int parseq_model_set_train_precision(parseq_model* m, int precision);

/* Loss of the K-permutation training objective (system.py:168-199, dropout off) for a batch whose encoder output is
 * `memory`, and its gradients — what `loss.backward()` leaves in `.grad` of every decoder-side parameter (decoder.*,
 * head.*, text_embed.*, pos_queries; system.py:183-196 through model.py:86-103, modules.py:55-125) and the gradient
 * w.r.t. `memory` that the encoder backward starts from.  fp32 throughout, computed from the model's master weights;
 * deterministic.
 *   memory            device fp32 [batch, tokens, embed_dim]             (parseq_encode output)
 *   tokens            device int32 [batch, ctx_len]   tgt[:, :-1] of tokenizer.encode(labels)            (system.py:176)
 *   targets           device int32 [2][batch * ctx_len]: tgt[:, 1:] flattened, and the same with <eos> replaced by <pad>
 *                     (used from the third permutation on, system.py:191-195)
 *   key_padding_mask  device uint8 [batch, ctx_len]   (tgt_in == pad) | (tgt_in == eos)                   (system.py:179)
 *   query_masks       device uint8 [num_perms][ctx_len][ctx_len]   generate_attn_masks(perm)[1]           (system.py:152-166)
 *   total_targets     sum over the permutations of their count of non-<pad> targets (the loss denominator, :189,196)
 *   dropout_p, seed   dropout probability of the decoder (configs/model/parseq.yaml:21; 0 = off, the evaluation-mode step the
 *                     parity tests use) and the 64-bit seed of this step's masks.  Eight sites per permutation pass, as in
 *                     the reference (model.py:99-102 embeddings and queries, dropped afresh in every pass; modules.py:33-43,
 *                     70-79 both attentions' probabilities, both projections, the MLP's hidden layer and output).  Masks
 *                     come from a counter-based generator (train_rows.h:drop_factor), not torch's Philox stream: with the
 *                     same masks the gradients are exact (tests), against the reference's run they agree in distribution.
 *   loss_out          device fp32 [1 + num_perms]: the loss, then each permutation's mean cross-entropy
 *   grads             device fp32 [parseq_model_grad_elems]: ACCUMULATED into (zero it for a fresh step); encoder slots untouched
 *   dmemory           device fp32 [batch, tokens, embed_dim]: written
 *   workspace         device, parseq_train_decoder_workspace_bytes(...) bytes; after the call it holds the intermediates of
 *                     the last permutation (parseq_train_decoder_workspace_offset names them; used by the parity tests).
 * The num_perms passes share every weight and differ in masks, dropout sites and (after two passes) targets only, so they run as
 * ONE batch of num_perms * batch images (round 3): same masks bit for bit, same per-pass losses, gradients equal to the
 * one-pass-after-the-other form up to fp32 summation order; the workspace holds num_perms copies of the per-pass buffers (4.5 GB
 * at batch 384, 6 passes).  The environment variable PARSEQ_TRAIN_PERM_GROUP=g (read by both functions below) runs them g at a time. */
size_t parseq_train_decoder_workspace_bytes(const parseq_model* m, int batch, int ctx_len, int num_perms);
int64_t parseq_train_decoder_workspace_offset(const parseq_model* m, int batch, int ctx_len, int num_perms, const char* name);
int parseq_train_decoder(parseq_model* m, const float* memory, const int32_t* tokens, const int32_t* targets,
                         const uint8_t* key_padding_mask, const uint8_t* query_masks, int batch, int ctx_len, int num_perms,
                         int total_targets, float dropout_p, uint64_t seed, float* loss_out, float* grads, float* dmemory,
                         void* workspace, size_t workspace_bytes, void* stream);

/* Encoder half of the training step (timm VisionTransformer blocks, strhub/models/parseq/modules.py:128-165): a forward in
 * fp32 from the master weights that keeps in `workspace` what the backward needs (per block: the residual stream before
 * it, qkv, the attention output, the stream after the attention residual, the fc1 pre-activation), and the backward from
 * `dmemory` (parseq_train_decoder) to the gradient of every encoder.* parameter, ACCUMULATED into `grads`.
 * images: device fp32 [batch, 3, H, W], normalised as the reference's transform leaves them.
 * Streams: in the bf16-operand mode parseq_train_encoder_backward runs the blocks' weight-gradient products on a second, library-owned
 * non-blocking stream beside the chain on `stream` (PARSEQ_TRAIN_ONE_STREAM=1 turns that off) — one such stream per distinct caller stream
 * (up to eight per model), so independent training chains may share a model on different streams (tests/test_training.py
 * test_micro_batched_step_equals_the_one_piece_step).  Every block ends with `stream` waiting
 * for it, so on return everything is ordered behind `stream` as usual — on an error return as well: a failure inside a block
 * synchronises the second stream before it is reported, so `grads` and `workspace` are not in use behind the caller's back. */
size_t parseq_train_encoder_workspace_bytes(const parseq_model* m, int batch);
int parseq_train_encoder_forward(parseq_model* m, const float* images, int batch, float* memory_out, void* workspace,
                                 size_t workspace_bytes, void* stream);
int parseq_train_encoder_backward(parseq_model* m, const float* dmemory, int batch, float* grads, void* workspace,
                                  size_t workspace_bytes, void* stream);

/* (added under ABI 15: a pure addition, no existing entry or structure changes, so the version number stays)
 * parseq_train_encoder_forward with the images' type as an argument: PARSEQ_F32 is the entry above, PARSEQ_U8 takes the raw pixels
 * [batch, 3, H, W] that parseq_resize_bicubic / parseq_augment_resize_bicubic write and normalises them inside the im2col
 * (ToTensor + Normalize(0.5, 0.5), strhub/data/module.py:78-81) — the three element-wise passes over a float image that a caller would
 * otherwise make disappear.  u8_table: NULL, or device fp32 [256] = the normalised value of every byte as the CALLER computes it; the
 * patch rows are then bit for bit the rows of the fp32 entry on table[image].  NULL = ((v / 255) - 0.5) / 0.5 in IEEE fp32, what the
 * inference loaders apply.  The image pointer should be patch_w-aligned (8- / 16-byte loads; otherwise the bytes are read one by one). */
int parseq_train_encoder_forward_ex(parseq_model* m, const void* images, int images_dtype, const float* u8_table, int batch,
                                    float* memory_out, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 10) ViTSTR's training step (strhub/models/vitstr/system.py:75-79 -> base.py:194-204 forward_logits_loss): the encoder entries
 * above take a ViTSTR model too (class token + pos_embed over tokens + 1 rows; the gradient of cls_token, pos_embed and patch_embed
 * ACCUMULATED into `grads`); in between, this entry computes the head on token rows 1 .. T of every image of `memory`
 * ([batch, tokens, E], after the encoder's final norm), the mean cross-entropy against `targets` (int32 [batch, T], ignore_index =
 * pad_id; total_targets = the number of non-pad targets) into loss_out[0], ACCUMULATES the head.weight / head.bias gradients into
 * `grads` and writes d loss / d memory into `dmemory` (zero on row 0 and past row T).  T <= max_label_length + 1.  Refuses a
 * PARSeq model. */
size_t parseq_train_vitstr_head_workspace_bytes(const parseq_model* m, int batch, int T);
int parseq_train_vitstr_head(parseq_model* m, const float* memory, const int32_t* targets, int batch, int T, int total_targets,
                             float* loss_out, float* grads, float* dmemory, void* workspace, size_t workspace_bytes, void* stream);

/* Gradient segments (ABI 5): the hook for overlapping the data-parallel all-reduce with the encoder's backward — what DDP's bucketed
 * reducer does under the reference's Trainer(strategy=DDPStrategy(...), reference train.py:65-71, 88-96).  The flat gradient buffer
 * becomes final piecewise: the decoder's part before parseq_train_encoder_backward starts, then the encoder's blocks from the last to
 * the first.  parseq_train_grad_segments = number of segments (enc_depth + 1; 0 for ViTSTR); segment `index` (in completion order) is
 * the element range [*begin, *end) of the buffer — the ranges tile [0, parseq_model_grad_elems) — and *event (may be NULL) is a
 * hipEvent_t the most recent parseq_train_encoder_backward recorded on its stream right after the last kernel that writes the range.
 * parseq_stream_wait_event makes `stream` wait for it (hipStreamWaitEvent), so that a collective enqueued on that stream starts as
 * soon as its bucket is final while the backward keeps running.  The events belong to ONE step (ABI 7): parseq_train_decoder — the
 * step's first gradient writer — invalidates them, a parseq_train_encoder_backward that returns 0 validates them; asking for an
 * event in between (the backward failed, or was never called for this step) returns PARSEQ_E_STATE instead of the previous step's
 * already-signalled event.  The ranges (event == NULL) are always available. */
int parseq_train_grad_segments(const parseq_model* m);
int parseq_train_grad_segment(parseq_model* m, int index, int64_t* begin, int64_t* end, void** event);
int parseq_stream_wait_event(void* stream, void* event);

/* Data-parallel sharding (ABI 8; SURVEY.md §8(e): the path shards over independent crops, reference bench.py / test.py loop over batches
 * per device under Lightning).  The contiguous split the Python mirror uses (parseq_amd/parallel.py shard_bounds): `world` shards of n
 * items whose sizes differ by at most one, shard `rank` = [*begin, *end).  A caller without torch shards its batch with this, runs
 * parseq_forward on its own shard with its own plan, and exchanges the [b_local, L, C] logits itself — ONE all-gather on its own RCCL
 * communicator when n is a multiple of world (INTEGRATION.md shows the calls); there is no collective inside the library.
 * Returns PARSEQ_E_INVALID for n < 0, world < 1 or rank outside [0, world). */
int parseq_shard_bounds(int64_t n, int world, int rank, int64_t* begin, int64_t* end);

/* Optimiser half of the training step (strhub/models/base.py:98-107: timm create_optimizer_v2('adamw') = torch.optim.AdamW;
 * configs/main.yaml:39 gradient_clip_val = torch.nn.utils.clip_grad_norm_), over the flat buffers:
 *   parseq_grad_norm   norm_out[0] = L2 norm of grads[0..n)  (workspace: 1024 floats); deterministic
 *   parseq_adamw_step  one AdamW update of the model's fp32 master weights IN PLACE from `grads`; exp_avg / exp_avg_sq are the
 *                      caller-owned moment buffers [parseq_model_grad_elems] (zero before step 1); `step` counts from 1;
 *                      decay_flags: host int32 [num_params], non-zero = weight decay applies to that tensor (NULL = none);
 *                      grad_norm: device scalar from parseq_grad_norm or NULL — when given the gradient is scaled by
 *                      min(1, max_norm / (norm + 1e-6)) on the fly (no host round trip).  Plans built on the model must be
 *                      refreshed (parseq_plan_refresh) before the next inference call.
 *   parseq_model_get_param  copies one parameter of the master weights out (device fp32), the inverse of parseq_model_set_param
 *   parseq_model_get_params copies EVERY parameter out in one launch: device_ptrs is a HOST array of `count` = parseq_model_num_params
 *                      device pointers in parseq_model_param_info order, each to that parameter's numel floats (what the reference's
 *                      optimizer.step() leaves in the module's tensors, strhub/models/base.py:98-107) */
int parseq_grad_norm(const float* grads, int64_t n, float* norm_out, float* workspace, void* stream);
int parseq_adamw_step(parseq_model* m, const float* grads, float* exp_avg, float* exp_avg_sq, const int32_t* decay_flags, float lr,
                      float beta1, float beta2, float eps, float weight_decay, int step, const float* grad_norm, float max_norm,
                      void* stream);
int parseq_model_get_param(const parseq_model* m, const char* key, float* device_ptr, int64_t numel, void* stream);
int parseq_model_get_params(parseq_model* m, float* const* device_ptrs, int count, void* stream);

/* Stochastic weight averaging (added under ABI 15, pure additions; the reference's train.py:93-95 switches Lightning's callback on, whose
 * average is torch.optim.swa_utils.AveragedModel's default rule), over flat buffers laid out like the master weights / the gradients:
 *   parseq_weights_average     avg <- weights when n_averaged == 0, else avg <- avg + (weights - avg) / (n_averaged + 1), over the
 *                              model's parseq_model_grad_elems master weights; avg: caller-owned device fp32 of that length.  One
 *                              launch, deterministic, IEEE subtraction / division / addition per element.
 *   parseq_op_weights_average  the same over any two device buffers of n floats (the single operator, for tests)
 *   parseq_model_set_params    the master weights <- flat (device fp32 [parseq_model_grad_elems]): how the average becomes the model at the
 *                              end of training; the flat mirror of parseq_model_get_params.  As after parseq_adamw_step, plans built on
 *                              the model must be refreshed (parseq_plan_refresh) before the next inference call. */
int parseq_weights_average(parseq_model* m, float* avg, int64_t n_averaged, void* stream);
int parseq_op_weights_average(const float* weights, float* avg, int64_t n, int64_t n_averaged, void* stream);
int parseq_model_set_params(parseq_model* m, const float* flat, void* stream);

/* ---- single operators, exported so each kernel is parity-tested through the C ABI ------------------------------- */

/* y = LayerNorm(x) over the last dim `E` (192 | 384 | 768); x fp32 [rows, E]; y in out_dtype. */
int parseq_op_layernorm(const float* x, const float* w, const float* b, void* y, int out_dtype, int rows, int E,
                        float eps, void* stream);
/* C = A W^T + bias.  A [M, K] and W [N, K] in `dtype`, bias fp32 [N] or NULL, C fp32 [M, N] (act = 0) or
 * C in `dtype` with exact-erf GELU applied (act = 1).  K must be a multiple of 8. */
int parseq_op_linear(const void* A, const void* W, const float* bias, void* C, int dtype, int act, int M, int N, int K,
                     void* stream);
/* C[M, N] (fp32) = LayerNorm(x[M, 384]; gamma, beta, eps) W^T + bias with the LayerNorm fused into the A-operand loader of the tile
 * GEMM (the decoder's q-projection / linear1 / head form).  dtype PARSEQ_F32 (W fp32 [N, 384]) or PARSEQ_BF16X3 (W from
 * parseq_op_split_pack). */
int parseq_op_ln_linear(const float* x, const float* gamma, const float* beta, const void* W, const float* bias, float* C, int dtype,
                        int M, int N, float eps, void* stream);
/* bf16x3, both operands pre-split (the encoder's big-M form): ws[M * 384 * 4 bytes] receives LayerNorm(x[M, 384]; gamma, beta, eps) as
 * block-planar hi | lo bf16 pairs (layernorm_split_kernel), then C[M, N] (fp32) = ws W^T + bias with W from parseq_op_split_pack,
 * through the direct-to-LDS GEMM that reads both operands as pairs.  act != 0: C is instead written as gelu(...) in the same
 * block-planar pair layout (N a multiple of 32; C is N * 4 bytes per row) — the fc1 epilogue of that path. */
int parseq_op_ln_linear_pairs(const float* x, const float* gamma, const float* beta, const void* W, const float* bias, void* C, void* ws,
                              int act, int M, int N, float eps, void* stream);
/* dtype = PARSEQ_BF16X3: A is f32 [M, K], K a multiple of 32; W must be the block-planar hi / lo copy of the f32 weight that
 * parseq_op_split_pack(src f32 [numel], dst [numel * 4 bytes]) produces (numel a multiple of 32); C as for PARSEQ_F32. */
int parseq_op_split_pack(const float* src, void* dst, int64_t numel, void* stream);
/* Same as parseq_op_linear with an explicit tile configuration (tools/gemm_bench.py sweeps these; ids in lib_ops.hip). */
int parseq_op_linear_cfg(const void* A, const void* W, const float* bias, void* C, int dtype, int act, int M, int N, int K,
                         int cfg, void* stream);
/* out[M, N] (bf16) = gelu(LayerNorm(x[M, 384]; gamma, beta, eps 1e-6) W^T + bias) through the register-resident-A panel
 * kernel; W bf16 [N, 384], N a multiple of 128.  variant must be 0 (the ablation variants of rounds 1-2 were removed; the parameter stays for ABI 4). */
int parseq_op_ln_linear_gelu(const float* x, const float* gamma, const float* beta, const void* W, const float* bias,
                             void* out, int M, int N, int variant, void* stream);
/* In place x[M, 384] (fp32) += fc2(gelu(fc1(LayerNorm(x; gamma, beta, eps 1e-6)))) through the fused MLP kernel:
 * W1 bf16 [1536, 384], b1 fp32 [1536], W2 bf16 [384, 1536], b2 fp32 [384]  (timm Block: x + mlp(norm2(x))). */
int parseq_op_mlp(float* x, const float* gamma, const float* beta, const void* W1, const float* b1, const void* W2,
                  const float* b2, int M, void* stream);
/* In place x[M, 384] (fp32) += proj(attention(qkv(LayerNorm(x; gamma, beta, eps 1e-6)))) through the fused attention-branch kernel
 * (timm Block: x + attn(norm1(x)), 6 heads of 64, one image = 128 consecutive rows per workgroup; M a multiple of 128):
 * Wqkv bf16 [1152, 384] (q | k | v rows, head-major), bqkv fp32 [1152], Wproj bf16 [384, 384], bproj fp32 [384].
 * variant 0 = encoder_attn_fused.h; 1 = the phase function the one-launch encoder is built from (encoder_blocks.h attn_branch_kernel). */
int parseq_op_attn_fused(float* x, const float* gamma, const float* beta, const void* Wqkv, const float* bqkv, const void* Wproj,
                         const float* bproj, int M, int variant, void* stream);
/* `depth` encoder blocks in one launch (encoder_blocks.h): in place on x[M, 384] (fp32), M a multiple of 128 (one image = 128
 * consecutive rows per workgroup).  block_ptrs: HOST array of depth * 12 DEVICE pointers, per block in this order: norm1 weight,
 * norm1 bias (fp32 [384]), Wqkv bf16 [1152, 384], bqkv fp32 [1152], Wproj bf16 [384, 384], bproj fp32 [384], norm2 weight, norm2
 * bias, W1 bf16 [1536, 384], b1 fp32 [1536], W2 bf16 [384, 1536], b2 fp32 [384].  table_ws: device scratch of depth * 48 bytes.
 * Test hook (the product path builds the table once per plan); uploads the table synchronously. */
int parseq_op_enc_blocks(float* x, const void* const* block_ptrs, int depth, int M, void* table_ws, void* stream);
/* The head and the tail of the one-launch encoder with no blocks in between (encoder_blocks.h patch_head / kv_phase; M a multiple of
 * 128 = whole 32 x 128 crops of 8 x 16 patches).  images != NULL ([M / 128, 3, 32, 128], images_dtype PARSEQ_F32 / PARSEQ_BF16 /
 * PARSEQ_U8): x = patches(images) Wpe^T + posb in the accumulators — timm PatchEmbed (4, 8) + bias + pos_embed, Wpe bf16 [384, 96] =
 * the Conv2d weight flattened (k = 32 c + 8 ky + kx), posb fp32 [128, 384] = pos_embed + bias; otherwise x[M, 384] (fp32) is loaded.
 * kmem != NULL: the launch ends with K | V = LayerNorm(x; norm_w, norm_b, eps 1e-6) Wkv^T + bkv (Wkv bf16 [768, 384], bkv fp32 [768];
 * strhub/models/parseq/modules.py:33-34 on timm's final norm) written as bf16 [M / 128][12][128][32] into kmem / vmem; otherwise x is
 * stored.  Test hook for the two phases the product path only runs inside parseq_forward. */
int parseq_op_enc_head_tail(float* x, const void* images, int images_dtype, const void* wpe, const float* posb, const float* norm_w,
                            const float* norm_b, const void* wkv, const float* bkv, void* kmem, void* vmem, int M, void* stream);
/* `depth` encoder blocks in one launch in the bf16x3 arithmetic (encoder_blocks_x3.h), in place on x[M, 384] (fp32), M a multiple of 128.
 * master: ONE fp32 device buffer holding every parameter of the blocks, each tensor on a 32-element boundary; pack: its block-planar
 * hi | lo copy (parseq_op_split_pack over the whole buffer, master_elems * 4 bytes); offsets: HOST array of depth * 12 element offsets
 * into master, per block: norm1 weight, norm1 bias, Wqkv [1152, 384], bqkv, Wproj [384, 384], bproj, norm2 weight, norm2 bias,
 * W1 [1536, 384], b1, W2 [384, 1536], b2.  table_ws: device scratch of depth * 48 bytes; scratch: device, M / 128 * 393216 bytes.
 * kmem / vmem != NULL (fp32 [M / 128][12][128][32]) with tail_offsets (HOST: final norm weight, bias, Wkv [768, 384], bkv [768]):
 * x is not stored; the launch ends with the decoder's K | V = LayerNorm(x) Wkv^T + bkv (timm forward_features' norm, modules.py:33-34).
 * Test hook (the product path builds the tables once per plan); uploads the table synchronously. */
int parseq_op_enc_blocks_x3(float* x, const float* master, const void* pack, int64_t master_elems, const uint32_t* offsets, int depth,
                            int M, void* table_ws, float* scratch, const uint32_t* tail_offsets, float* kmem, float* vmem, void* stream);
/* The same launch through the kernel parseq_forward runs since ABI 7 (encoder_blocks_x3w.h: eight waves of 16 rows per workgroup, two per
 * SIMD, instead of four of 32); same arguments, bit-identical results.  parseq_op_enc_blocks_x3 stays on the four-wave kernel as the
 * reference of that identity (PARSEQ_X3_FOUR_WAVES=1 puts it back under parseq_forward). */
int parseq_op_enc_blocks_x3w(float* x, const float* master, const void* pack, int64_t master_elems, const uint32_t* offsets, int depth,
                             int M, void* table_ws, float* scratch, const uint32_t* tail_offsets, float* kmem, float* vmem, void* stream);
/* The forms of parseq_op_mlp: variant 0 = x re-read by the epilogue; 10 = x resident in the fc2 accumulators (the form the per-layer
 * encoder path uses); 11 = the phase function the one-launch encoder is built from (encoder_blocks.h mlp_branch_kernel). */
int parseq_op_mlp_variant(float* x, const float* gamma, const float* beta, const void* W1, const float* b1, const void* W2,
                          const float* b2, int M, int variant, void* stream);
/* Encoder attention for `bh` (image, head) pairs: q, k [bh, 128, 64], vt [bh, 64, 128] in `dtype`;
 * out [bh / heads * 128, heads * 64] in `dtype`.  dtype = PARSEQ_BF16X3: f32 tensors, split-bf16 products. */
int parseq_op_encoder_attention(const void* q, const void* k, const void* vt, void* out, int dtype, int bh, int heads,
                                void* stream);
/* The AR cross-attention on 24-bit K / V rows alone, embed_dim 384 (12 heads of 32), 128 memory tokens, one query per image: qc fp32
 * [batch, 384] (unscaled); kmem, vmem: the u16 plane [batch, 12, 128, 32] (bits 31..16 of each f32) with the u8 plane (bits 15..8) of the
 * same shape plane_elems * 2 bytes behind its start; out fp32 [batch, 384].  tile = 0: one workgroup per image (what a forward alone on the
 * device runs); tile = 1: one workgroup per 16 images (the in-flight AR decode's form).  Bit-identical outputs. */
int parseq_op_cross_attention_ar24(const float* qc, const void* kmem, const void* vmem, int64_t plane_elems, int batch, int tile, float* out,
                                   void* stream);
/* (ABI 10) The training step's encoder self-attention alone, fp32 (exact products): `tokens` tokens of `heads` heads of width 64;
 * qkv [batch * tokens, 3 E] (q | k | v per row, E = 64 heads), o [batch * tokens, E]; backward: d_o like o, dqkv like qkv (written).
 * Past 128 tokens (up to 256) the key-streaming kernels run: the forward writes lse [batch, heads, tokens] (each query row's
 * log-sum-exp of the scaled scores), the backward reads it and writes dsum [batch, heads, tokens] (rowsum(d_o * o)); at 128 tokens or
 * fewer the step's resident kernels run and neither is touched.  *route (may be NULL): 1 for the key-streaming kernels, 0 otherwise. */
int parseq_op_train_attention(const float* qkv, float* o, float* lse, const float* d_o, float* dqkv, float* dsum, int batch, int tokens,
                              int heads, int backward, int* route, void* stream);
/* One call of the training step's train_attn(), whichever kernel it takes (tests/test_train_attn.py; additive, no ABI bump).  The
 * descriptor carries every field of the step's own argument block (parseq_amd/csrc/train_attn.h TrainAttnArgs, which documents the
 * layouts and the pass rules) and what the step takes from its context: the head width, the operand mode as a precision constant
 * (PARSEQ_F32, PARSEQ_BF16 or PARSEQ_BF16X3, anything else is refused) and the dropout as (dropout_p in [0, 1), seed), from which the
 * hook derives threshold and scale as parseq_train_decoder does.  All pointers are device pointers; strides in elements. */
enum parseq_train_attn_route {     /* which kernel family a call took (or would have taken, when it is refused) */
    PARSEQ_TRAIN_ATTN_DEC_BF16 = 0,    /* train_attn_dec_bf16_kernel: bf16 operands, head width 32, <= 32 queries, <= 128 keys (two instantiations: <= 32 keys, more) */
    PARSEQ_TRAIN_ATTN_ENC_BF16 = 1,    /* train_attn_bf16_kernel: bf16 operands, 128 x 128 tokens, head width 64 */
    PARSEQ_TRAIN_ATTN_MFMA = 2,        /* train_attn_mfma_kernel: exact fp32 products on the matrix cores, head width 64 */
    PARSEQ_TRAIN_ATTN_WIDE = 3,        /* train_attn_wide_*_kernel: key-streaming, 129..256 tokens, head width 64 */
    PARSEQ_TRAIN_ATTN_HD32 = 4,        /* train_attn_kernel<*, 32> */
    PARSEQ_TRAIN_ATTN_HD64 = 5,        /* train_attn_kernel<*, 64> */
    PARSEQ_TRAIN_ATTN_NONE = 6         /* no kernel */
};
typedef struct parseq_train_attn_desc {
    const float* q; int64_t q_bstride; int32_t ldq;                /* q_bstride = 0: one set of queries for the whole batch */
    const float* k; const float* v; int32_t ldkv;
    const uint8_t* qmask; const uint8_t* kmask; int32_t ldkm;      /* [Lq, Lk] per pass and [images of a pass, ldkm]; non-zero = masked; NULL: none */
    float* o; int32_t ldo;
    void* o16; void* dq16; void* dk16; void* dv16;                 /* bf16 outputs INSTEAD of o / dq / dk + dv (the 128 x 128 bf16 kernel alone) */
    const float* d_o;
    float* dq; int32_t lddq;
    float* dk; float* dv; int32_t lddkv;
    int32_t kv_accumulate;
    int32_t Lq, Lk, H;
    float scale;
    uint32_t drop_site;
    int32_t pass_B; int64_t qmask_pstride; uint32_t site_pstride; int32_t kv_shared;
    int32_t pass_loop;
    float* lse; float* dsum;                                       /* [batch, H, Lq], the key-streaming route alone */
    int32_t head_dim;
    int32_t bf16_ops;
    float dropout_p; uint64_t seed;
} parseq_train_attn_desc;
/* batch: images over all passes.  backward == 0: o (or o16) is written; otherwise dq / dk / dv (or their bf16 twins).  *route (may be
 * NULL) receives an enum parseq_train_attn_route, also when the call is refused (non-zero return, nothing written). */
int parseq_op_train_attention_desc(const parseq_train_attn_desc* desc, int batch, int backward, int32_t* route, void* stream);

/* (ABI 13) The rotation alone, for one image (tests/test_rotate.py compares it with Pillow): out = device uint8
 * [rot_height, rot_width, 3], dense.  image: HOST descriptor, read before the call returns. */
int parseq_op_rotate(const parseq_rotated_image_desc* image, uint8_t* out, void* stream);

/* (ABI 14) One image's augmentation chain alone (tests/test_augment.py compares it with Pillow): out = device uint8 [h, w, 3], dense, of the
 * last operator's size.  desc: HOST descriptor, alive until the stream has passed; workspace as for parseq_augment_resize_bicubic with batch 1. */
int parseq_op_augment(const parseq_augment_desc* desc, uint8_t* out, void* workspace, size_t workspace_bytes, void* stream);

/* (ABI 12) The training step's products and row kernels one operator at a time (tests/test_train_gemm.py).  The three hooks build
 * the step's context from their arguments and call the internal functions the step calls, unchanged.  bf16_ops: the operand
 * mode as a precision constant (parseq_model_set_train_precision): PARSEQ_F32 (0), PARSEQ_BF16 (1) or, from ABI 15, PARSEQ_BF16X3 (3);
 * any other value is refused with PARSEQ_E_INVALID.  scratch / scratch_floats: the caller's, what the step carves out of its
 * workspace (16 Mi floats there): split-K partials, partial column sums, the LayerNorm backward's chunk partials at its end; NULL / a small
 * one are allowed and change the route. */
enum parseq_gemm_kernel {          /* which kernel a product ran on; bf16-operand kernels: orientation of A, B (k = contiguous along the contraction, n = along the outer axis) */
    PARSEQ_GEMM_NONE = -1,         /* refused */
    PARSEQ_GEMM_VALU = 0,          /* sgemm_kernel */
    PARSEQ_GEMM_MFMA_F32 = 1,      /* mfma_sgemm_kernel: exact fp32 products */
    PARSEQ_GEMM_BF16_KK = 2, PARSEQ_GEMM_BF16_KN = 3, PARSEQ_GEMM_BF16_NK = 4, PARSEQ_GEMM_BF16_NN = 5,   /* mfma_bgemm_kernel, both operands fp32 in memory */
    PARSEQ_GEMM_B16_KK = 6, PARSEQ_GEMM_B16_KN = 7, PARSEQ_GEMM_B16_NK = 8, PARSEQ_GEMM_B16_NN = 9,       /* ... B a bf16 shadow */
    PARSEQ_GEMM_A16_NN = 10,       /* ... both shadows, both outer-contiguous, 32-deep stages */
    PARSEQ_GEMM_BOTH16_K = 11,     /* mfma_bgemm16_kernel: both shadows k-contiguous */
    PARSEQ_GEMM_BOTH16_T = 12,     /* mfma_bgemm16t_kernel: both shadows outer-contiguous, 64-deep stages */
    PARSEQ_GEMM_X3_KK = 13, PARSEQ_GEMM_X3_KN = 14, PARSEQ_GEMM_X3_NK = 15, PARSEQ_GEMM_X3_NN = 16         /* (ABI 15) mfma_x3gemm_kernel: split-bf16 operands, both fp32 in memory */
};
typedef struct parseq_gemm_operand {
    const void* data;              /* device */
    int32_t dtype;                 /* PARSEQ_F32, or PARSEQ_BF16: a shadow */
    int64_t outer_stride, k_stride;/* in elements: along m (A) / n (B), and along the contraction */
} parseq_gemm_operand;
/* C[M, N] (+)= alpha * A B + bias[n] + R[m % rper][n], times gelu'(gelu_pre) if given; dense rows of N elements everywhere */
typedef struct parseq_train_gemm_desc {
    parseq_gemm_operand A, B;
    int32_t M, N, K;
    float* C;                      /* fp32 [M, N], may be NULL when c16 is given */
    void* c16;                     /* bf16 [M, N] or NULL */
    const float* bias;             /* [N] or NULL */
    const float* R; int64_t ldr; int32_t rper;      /* residual rows or NULL */
    float alpha;
    int32_t accumulate;
    float* asum;                   /* [M] += row sums of A, or NULL */
    const float* gelu_pre; const void* gelu_pre16;  /* [M, N] fp32 / bf16 or NULL */
    float* gelu_out; void* gelu_out16;              /* [M, N] fp32 / bf16 or NULL: gelu(C) as a second output */
    int32_t bf16_ops;
    float* scratch; size_t scratch_floats;
} parseq_train_gemm_desc;
typedef struct parseq_gemm_route {
    int32_t kernel;                /* enum parseq_gemm_kernel */
    int32_t whole;                 /* the four-workgroups-per-CU form of the all-bf16 kernels */
    int32_t splits, k_chunk;       /* split-K: workgroups per tile along the contraction, and the contraction range of each */
    int32_t folded_asum, folded_gelu_pre, folded_gelu_out;   /* riders the kernel's epilogue took (the others were not run: sgemm leaves them to its caller) */
} parseq_gemm_route;
/* One call of the training step's sgemm().  route may be NULL.  Riders the chosen kernel does not fold are NOT run (route->folded_*). */
int parseq_op_train_gemm(const parseq_train_gemm_desc* desc, parseq_gemm_route* route, void* stream);
/* lin_fwd (backward == 0): y[M, N] = x[M, K] W[N, K]^T + bias + R[m % rper] (R NULL: none), gelu_out (may be NULL) = gelu(y).
 * lin_bwd (backward != 0): dW[N, K] += dy[M, N]^T x;  db[N] += column sums of dy;  dx[M, K] = dy W (dx may be NULL), times
 * gelu'(dx_gelu_pre[M, K]) if given.  All fp32. */
int parseq_op_train_linear(const float* x, const float* W, const float* bias, const float* R, int rper, float* y, float* gelu_out,
                           const float* dy, float* dW, float* db, float* dx, const float* dx_gelu_pre, int M, int N, int K, int backward,
                           int bf16_ops, float* scratch, size_t scratch_floats, void* stream);
/* train_ln_fwd (backward == 0): y[rows, E] = LayerNorm(x; gamma, beta, eps) in y_dtype (PARSEQ_F32 / PARSEQ_BF16).
 * ln_bwd (backward != 0): dx = add (may be NULL) + the LayerNorm backward of dy; dgamma, dbeta += their gradients; dx16 (may be NULL): dx
 * again as bf16.  Refused when the chunk partials (rows / 4 rounded up, times 2 E floats, + 64 E) do not fit the scratch. */
int parseq_op_train_layernorm(const float* x, const float* gamma, const float* beta, void* y, int y_dtype, const float* dy, const float* add,
                              float* dx, void* dx16, float* dgamma, float* dbeta, int rows, int E, float eps, int backward, float* scratch,
                              size_t scratch_floats, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PARSEQ_HIP_H_ */
