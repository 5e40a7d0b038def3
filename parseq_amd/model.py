"""Inner PARSeq model: parameter container with the reference's state_dict layout, forward on libparseq_hip.

Mirrors `strhub/models/parseq/model.py:31-169` (class `PARSeq`): same constructor arguments, same attributes
(`decode_ar`, `refine_iters`, `max_label_length`, `encoder`, `decoder`, `head`, `text_embed`, `pos_queries`), same
`forward(tokenizer, images, max_length=None)`, `encode(img)` and `decode(...)` entry points, and exactly the reference's
`state_dict()` keys/shapes so released checkpoints load with `load_state_dict`.

The sub-modules here only HOLD parameters (their own `forward` is never called).  All arithmetic runs in the HIP
library through `parseq_amd._native`; on a CPU tensor or without the library the call raises.
"""
from __future__ import annotations

import ctypes as C
import math
import os
from dataclasses import dataclass
from typing import Optional, Sequence

import torch
import torch.nn as nn
from torch import Tensor

from . import _native
from .tokenizer import Tokenizer

_PRECISIONS = {'bf16': _native.PARSEQ_BF16, 'fp32': _native.PARSEQ_F32, 'f32': _native.PARSEQ_F32, 'bf16x3': _native.PARSEQ_BF16X3}


BEAM_MAX_WIDTH = 16      # PARSEQ_BEAM_MAX_WIDTH
BEAM_REFINE_MODES = {'score': 1, 'edit': 2}      # PARSEQ_BEAM_REFINE_SCORE / PARSEQ_BEAM_REFINE_EDIT


def check_beam_refine(refine, refine_iters, lexicon=None):
    """The refusals of `beam_search(..., refine=, refine_iters=)` that need no device."""
    if refine is None:
        if refine_iters != 1:
            raise ValueError(f'beam_search: refine_iters = {refine_iters} without refine')
        return
    if refine not in BEAM_REFINE_MODES:
        raise ValueError(f"beam_search: refine must be None, 'edit' or 'score', got {refine!r}")
    if not isinstance(refine_iters, int) or isinstance(refine_iters, bool) or refine_iters < 1:
        raise ValueError(f'beam_search: refine_iters must be an integer >= 1, got {refine_iters!r}')
    if refine == 'score' and refine_iters != 1:
        raise ValueError(f"beam_search: refine='score' is idempotent and runs once, got refine_iters = {refine_iters}")
    if refine == 'edit' and lexicon is not None:
        raise ValueError("beam_search: refine='edit' under a lexicon (an edited reading can leave the word list); use refine='score'")


@dataclass
class BeamResult:
    """What `PARSeq.beam_search` returns, on the device, best hypothesis first per image."""
    tokens: Tensor                       # int32 [B, W, num_steps] class ids; pad_id after a hypothesis' <eos> (and in every slot of a dead beam)
    scores: Tensor                       # fp32 [B, W] sum of log-probabilities (natural log, <eos> included, no length normalisation)
    lengths: Tensor                      # int32 [B, W] characters before <eos>
    finished: Tensor                     # uint8 [B, W] 0 = no <eos> after the last step
    # trace=True only, per step in the row order the decoder ran (row b * W + w):
    trace_logits: Optional[Tensor] = None       # fp32 [num_steps, B * W, C]
    trace_tokens_in: Optional[Tensor] = None    # int32 [num_steps, B * W, num_steps] the histories each step ran on
    trace_parent: Optional[Tensor] = None       # int32 [num_steps, B * W] each new beam's parent within its image (-1: dead)
    trace_score: Optional[Tensor] = None        # fp32 [num_steps, B * W] each new beam's score after the step
    # refine='edit' / 'score' only: `scores` are then the refined scores.  Plain class attributes, set on the instance by
    # a refined search: a result without refinement has the fields it had (`vars(result)` holds tensors only).
    ar_scores = None                   # Optional[Tensor] fp32 [B, W] the score the search itself gave the hypothesis a row descends from
    # ... and trace=True, per refinement iteration:
    trace_refine_tokens_in = None      # Optional[Tensor] int32 [refine_iters, B * W, num_steps] the tgt_in rows of the iteration
    trace_refine_logits = None         # Optional[Tensor] fp32 [refine_iters, B * W, num_steps, C] its logits
    # automaton= only, set on the instance likewise: `scores` (and `trace_score`) are then the fused values the ranking used.
    model_scores = None                # Optional[Tensor] fp32 [B, W] the model's own sum of log-probabilities
    priors = None                      # Optional[Tensor] fp32 [B, W] the sum of the automaton's weights along the hypothesis (0 for a dead beam)


@dataclass
class LexiconBeamResult(BeamResult):
    """`beam_search(..., lexicon=...)`: a `BeamResult` and each hypothesis' word."""
    words: Optional[Tensor] = None       # int32 [B, W] index into `lexicon.words` of a finished hypothesis, -1 otherwise


def check_beam_automaton(automaton, alpha, beta, lexicon, refine, classes):
    """The refusals of `beam_search(..., automaton=, alpha=, beta=)` that need no device."""
    if automaton is None:
        if alpha != 1.0 or beta != 0.0:
            raise ValueError('beam_search: alpha / beta without an automaton')
        return
    if lexicon is not None:
        raise ValueError('beam_search: automaton= and lexicon= exclude each other (Automaton.from_lexicon gives a word list its weights)')
    if refine is not None:
        raise ValueError('beam_search: refine= under a weighted automaton is refused: ranking pseudo-log-likelihoods with a prior is not defined yet')
    if not all(isinstance(v, (int, float)) and not isinstance(v, bool) and math.isfinite(v) for v in (alpha, beta)):
        raise ValueError(f'beam_search: alpha and beta must be finite numbers, got {alpha!r} and {beta!r}')
    nxt, weight = automaton.next, automaton.weight
    if (nxt.dim() != 2 or nxt.shape[1] != classes or nxt.dtype != torch.int32 or nxt.shape[0] < 1 or weight.shape != nxt.shape
            or weight.dtype != torch.float32):
        raise ValueError(f'beam_search: the automaton tables must be int32 and fp32 [states, {classes}] (one column per head class), got '
                         f'{nxt.dtype} {tuple(nxt.shape)} and {weight.dtype} {tuple(weight.shape)}')


@dataclass
class LexiconMatchResult(LexiconBeamResult):
    """What `PARSeq.lexicon_match` returns: the fields of a `LexiconBeamResult` over W = n (+ 1 with `keep_reading`)
    hypotheses per crop — `words` -1 for the reading itself and for a dead slot, `scores` 0 for a live hypothesis without rescoring — plus:"""
    distances: Optional[Tensor] = None          # int32 [B, W] Levenshtein distance of the hypothesis to the reading; MATCH_DEAD for a dead slot
    reading_tokens: Optional[Tensor] = None     # int32 [B, L] the free reading: the arg-max of every position of `forward`'s logits
    reading_lengths: Optional[Tensor] = None    # int32 [B] its characters: the index of the first <eos> (L: none)


def check_lexicon_match(n, keep_reading, lexicon, max_label_length, classes):
    """The refusals of `lexicon_match` that need no device."""
    width = BEAM_MAX_WIDTH - (1 if keep_reading else 0)
    if not isinstance(n, int) or isinstance(n, bool) or not 1 <= n <= width:
        raise ValueError(f'lexicon_match: n must be an integer in [1, {width}]' + (' (one of the 16 slots is the reading\'s)' if keep_reading else '') + f', got {n!r}')
    if lexicon.num_classes != classes:
        raise ValueError(f'lexicon_match: the lexicon was built for {lexicon.num_classes} classes, the model has {classes}')
    if lexicon.max_label_length > max_label_length:
        raise ValueError(f'lexicon_match: the lexicon holds words of up to {lexicon.max_label_length} characters, the model reads {max_label_length}')
    if lexicon.num_rows == 0:
        raise ValueError('lexicon_match: no word of the lexicon was entered (the word table is empty)')


@dataclass
class Localization:
    """What `PARSeq.localize` returns, on the device.  L = max_label_length + 1 positions, S = the encoder's patch
    tokens; coordinates are pixels of the model's input (`img_size`), x to the right and y down."""
    tokens: Tensor                       # int32 [B, L] the reading that was localised: its characters, <eos> at position `lengths[b]`, pad_id after
    lengths: Tensor                      # int32 [B] characters before <eos>
    maps: Tensor                         # fp32 [B, L, S] head-averaged cross-attention of position i over the patch tokens; rows 0 .. lengths[b] sum to 1, the rest are zero
    centres: Tensor                      # fp32 [B, L, 2] (x, y) centre of mass of the map
    boxes: Tensor                        # fp32 [B, L, 4] (x0, y0, x1, y1): centre -+ sqrt(3) sigma per axis, clipped to the image
    peak: Tensor                         # int32 [B, L] the patch token of the largest probability (lowest index on ties); -1 past the reading
    peak_mass: Tensor                    # fp32 [B, L] that probability


def check_labels(labels, max_label_length: int):
    """The refusal of `localize(images, labels)` that needs no device: a label the model has no positions for."""
    for y in labels:
        if len(y) > max_label_length:
            raise ValueError(f'localize: label {y!r} has {len(y)} characters, the model reads at most max_label_length = {max_label_length}')


@dataclass
class OrientedResult:
    """What `orient` returns, on the device: of the K turned views of every crop, the one the model reads best."""
    view: Tensor                         # int32 [B] the winner: the first view of the largest key
    keys: Tensor                         # fp64 [B, K] every view's key (a NaN key is stored as -inf)
    logits: Tensor                       # fp32 [B, L, C] the winner's logits, bit for bit (`tokenizer.decode_logits` reads them)
    ids: Tensor                          # int32 [B, L], int32 [B], fp32 [B]: what parseq_postprocess writes for the winner
    lengths: Tensor
    confidence: Tensor
    images: Tensor                       # [B, 3, H, W] the winner's crop, in the dtype of the views


def check_orient(shape, criterion, prior):
    """The refusals of `orient` that need no device; returns (B, K, the prior as K floats or None)."""
    if len(shape) != 5:
        raise ValueError(f'orient: views must be [B, K, 3, H, W], got {list(shape)}')
    B, K = int(shape[0]), int(shape[1])
    if B < 1:
        raise ValueError('orient: empty batch')
    if not 1 <= K <= _native.ORIENT_MAX_VIEWS:
        raise ValueError(f'orient: {K} views per crop, there must be 1 .. {_native.ORIENT_MAX_VIEWS}')
    if criterion not in _native.ORIENT_CRITERIA:
        raise ValueError(f"orient: criterion must be 'mean' or 'sum', got {criterion!r}")
    if prior is not None:
        prior = [float(v) for v in (prior.tolist() if isinstance(prior, Tensor) else prior)]
        if len(prior) != K:
            raise ValueError(f'orient: a prior of {len(prior)} values for {K} views')
        if any(math.isnan(v) or v == math.inf for v in prior):
            raise ValueError(f'orient: the prior {prior} must hold numbers below +inf (-inf rules a view out)')
    return B, K, prior


def orient_select(logits: Tensor, views: int, eos_id: int, images: Optional[Tensor] = None, criterion: str = 'mean', prior=None) -> OrientedResult:
    """The choice alone (parseq_op_orient_select) on logits [B * K, L, C] whose rows b K .. b K + K - 1 are the K = `views` views of crop b,
    and optionally their crops `images` [B * K, ...]: two launches, no host synchronisation."""
    if logits.dim() != 3 or logits.dtype != torch.float32 or not logits.is_cuda or logits.shape[0] % views:
        raise ValueError(f'orient_select: logits must be CUDA fp32 [B * {views}, L, C], got {logits.dtype} {list(logits.shape)}')
    logits = logits.contiguous()
    rows, L, C = logits.shape
    B, dev = rows // views, logits.device
    _, _, prior = check_orient((B, views, 0, 0, 0), criterion, prior)
    images_out, elems, code = None, 0, 0
    if images is not None:
        if images.shape[0] != rows or images.device != dev:
            raise ValueError(f'orient_select: images must hold {rows} crops on {dev}, got {list(images.shape)} on {images.device}')
        images = images.contiguous()
        code = _native.dtype_code(images.dtype)
        elems = images[0].numel()
        images_out = torch.empty((B,) + tuple(images.shape[1:]), dtype=images.dtype, device=dev)
    pr = torch.tensor(prior, dtype=torch.float32).to(dev) if prior is not None else None
    res = OrientedResult(torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, views, dtype=torch.float64, device=dev),
                         torch.empty(B, L, C, dtype=torch.float32, device=dev), torch.empty(B, L, dtype=torch.int32, device=dev),
                         torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev), images_out)
    lib = _native.lib()
    need = lib.parseq_op_orient_select_workspace_bytes(B, views, L)
    if need == 0:
        raise ValueError(f'orient_select: {B} crops of {views} views and {L} positions: the library takes 1 .. 64 positions and at most 2^26 rows')
    ws = torch.empty(need, dtype=torch.uint8, device=dev)
    with _native.guard(dev):
        _native.check(lib.parseq_op_orient_select(_native.ptr(logits), B, views, L, C, int(eos_id), _native.ptr(images), code, elems,
                                                  _native.ORIENT_CRITERIA[criterion], _native.ptr(pr), _native.ptr(res.view), _native.ptr(res.keys),
                                                  _native.ptr(res.logits), _native.ptr(res.ids), _native.ptr(res.lengths), _native.ptr(res.confidence),
                                                  _native.ptr(images_out), _native.ptr(ws), need, _native.stream_ptr(dev)))
    return res


@dataclass
class LineWindows:
    """The windows a `LineResult` was stitched from, on the device: R = all windows of all lines, rows of one batch."""
    tokens: Tensor                       # int32 [R, L], int32 [R], fp32 [R, L, 2], fp32 [R, L, 4]: what `localize` gives for the window batch
    lengths: Tensor
    centres: Tensor
    boxes: Tensor
    probs: Tensor                        # fp32 [R, L]: what parseq_postprocess gives for `forward`'s logits of the window batch
    win: Tensor                          # int32 [R, 3]: (x0, ww, h) of every window
    line_first: Tensor                   # int32 [N + 1]: line l is rows line_first[l] .. line_first[l + 1] - 1
    images: Tensor                       # uint8 [R, 3, H, W]: the window batch itself


@dataclass
class LineResult:
    """What `read_lines` returns, on the device: N lines of at most M = max_chars characters, in (window, position)
    order; coordinates are pixels of the line's own image."""
    lengths: Tensor                      # int32 [N] the characters that survived the stitch (may exceed M: only M are stored)
    tokens: Tensor                       # int32 [N, M], -1 past the reading
    probs: Tensor                        # fp32 [N, M]
    boxes: Tensor                        # fp32 [N, M, 4] (x0, y0, x1, y1)
    x: Tensor                            # fp64 [N, M] the centres the stitch compared
    src: Tensor                          # int32 [N, M, 2] (window index in its line, position in the window), -1 past the reading
    confidence: Tensor                   # fp32 [N]
    windows: LineWindows


def check_lines(overlap, aspect, min_sep, max_chars, max_batch):
    """The refusals of `read_lines` that need neither an image nor a device (`preprocess.line_windows` has the plan's own)."""
    if not 0.0 <= overlap <= 0.75:
        raise ValueError(f'read_lines: overlap must be in [0, 0.75], got {overlap!r}')
    if not 0.25 <= aspect <= 4.0:
        raise ValueError(f'read_lines: aspect must be in [0.25, 4], got {aspect!r}')
    if not (isinstance(min_sep, (int, float)) and 0.0 <= min_sep < math.inf):
        raise ValueError(f'read_lines: min_sep must be a finite fraction of the line height, at least 0, got {min_sep!r}')
    if max_chars is not None and not (isinstance(max_chars, int) and 1 <= max_chars <= _native.LINE_MAX_OUT):
        raise ValueError(f'read_lines: max_chars must be an integer in [1, {_native.LINE_MAX_OUT}], got {max_chars!r}')
    if not (isinstance(max_batch, int) and max_batch >= 1):
        raise ValueError(f'read_lines: max_batch must be a positive integer, got {max_batch!r}')


def chunk_lines(line_first, max_batch: int):
    """[(first line, end line)] of the calls `read_lines` makes: lines in order, as many whole lines per call as fit in `max_batch` rows.
    ValueError for a line that does not fit on its own."""
    chunks, start = [], 0
    for l in range(len(line_first) - 1):
        k = line_first[l + 1] - line_first[l]
        if k > max_batch:
            raise ValueError(f'read_lines: line {l} has {k} windows, more than max_batch = {max_batch} rows of one call')
        if line_first[l + 1] - line_first[start] > max_batch:
            chunks.append((start, l))
            start = l
    return chunks + [(start, len(line_first) - 1)]


def stitch_lines(tokens: Tensor, lengths: Tensor, probs: Tensor, centres: Tensor, boxes: Tensor, win: Tensor, line_first: Tensor, min_sep: Tensor,
                 C_: int, img_size, max_out: int):
    """The stitch alone (parseq_op_stitch_lines) on caller tensors — as `LineWindows` holds them; `min_sep` fp64 [N] in source pixels.
    Returns (lengths, tokens, probs, boxes, x, src, confidence).  One launch, no host synchronisation."""
    dev = tokens.device
    rows, L = tokens.shape
    n = line_first.numel() - 1
    out = (torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, max_out, dtype=torch.int32, device=dev),
           torch.empty(n, max_out, dtype=torch.float32, device=dev), torch.empty(n, max_out, 4, dtype=torch.float32, device=dev),
           torch.empty(n, max_out, dtype=torch.float64, device=dev), torch.empty(n, max_out, 2, dtype=torch.int32, device=dev),
           torch.empty(n, dtype=torch.float32, device=dev))
    with _native.guard(dev):
        _native.check(_native.lib().parseq_op_stitch_lines(
            _native.ptr(tokens.contiguous()), _native.ptr(lengths.contiguous()), _native.ptr(probs.contiguous()), _native.ptr(centres.contiguous()),
            _native.ptr(boxes.contiguous()), rows, L, int(C_), _native.ptr(win.contiguous()), int(img_size[0]), int(img_size[1]),
            _native.ptr(line_first.contiguous()), n, _native.ptr(min_sep.contiguous()), int(max_out), *[_native.ptr(t) for t in out], _native.stream_ptr(dev)))
    return out


def init_weights(module: nn.Module, name: str = '', exclude: Sequence[str] = ()):
    """Initialisation scheme of the reference (`strhub/models/utils.py:107-125`): trunc-normal(0.02) Linear / Embedding
    weights, zero biases, unit LayerNorm, Kaiming-normal(fan_out) convolutions.  This is a deliberate statement-for-statement
    behavioural mirror of that 19-line function (same branches, same torch initialisers in the same order), not an independent
    design: seeded random-init weights must come out identical to the reference's for bench.py's `manual_seed(0)` model."""
    if any(name.startswith(e) for e in exclude):
        return
    if isinstance(module, nn.Linear):
        nn.init.trunc_normal_(module.weight, std=0.02)
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    elif isinstance(module, nn.Embedding):
        nn.init.trunc_normal_(module.weight, std=0.02)
        if module.padding_idx is not None:
            module.weight.data[module.padding_idx].zero_()
    elif isinstance(module, nn.Conv2d):
        nn.init.kaiming_normal_(module.weight, mode='fan_out', nonlinearity='relu')
        if module.bias is not None:
            nn.init.zeros_(module.bias)
    elif isinstance(module, (nn.LayerNorm, nn.BatchNorm2d, nn.GroupNorm)):
        nn.init.ones_(module.weight)
        nn.init.zeros_(module.bias)


class _Holder(nn.Module):
    """A module that exists to own parameters under the reference's names."""

    def forward(self, *a, **k):  # pragma: no cover
        raise RuntimeError('parameter holder: compute runs in libparseq_hip, call the PARSeq model instead')


class _PatchEmbed(_Holder):
    def __init__(self, patch_size, embed_dim):
        super().__init__()
        self.proj = nn.Conv2d(3, embed_dim, kernel_size=tuple(patch_size), stride=tuple(patch_size))


class _Attention(_Holder):
    def __init__(self, dim):
        super().__init__()
        self.qkv = nn.Linear(dim, 3 * dim)
        self.proj = nn.Linear(dim, dim)


class _Mlp(_Holder):
    def __init__(self, dim, hidden):
        super().__init__()
        self.fc1 = nn.Linear(dim, hidden)
        self.fc2 = nn.Linear(hidden, dim)


class _Block(_Holder):
    def __init__(self, dim, mlp_ratio):
        super().__init__()
        self.norm1 = nn.LayerNorm(dim, eps=1e-6)
        self.attn = _Attention(dim)
        self.norm2 = nn.LayerNorm(dim, eps=1e-6)
        self.mlp = _Mlp(dim, int(dim * mlp_ratio))


class Encoder(_Holder):
    """Parameter layout of timm's VisionTransformer as the reference configures it (modules.py:128-161):
    no class token, no head; LayerNorm eps 1e-6."""

    def __init__(self, img_size, patch_size, embed_dim, depth, num_heads, mlp_ratio):
        super().__init__()
        self.img_size, self.patch_size = tuple(img_size), tuple(patch_size)
        self.num_heads = num_heads
        n_tok = (img_size[0] // patch_size[0]) * (img_size[1] // patch_size[1])
        self.patch_embed = _PatchEmbed(patch_size, embed_dim)
        self.pos_embed = nn.Parameter(torch.empty(1, n_tok, embed_dim))
        self.blocks = nn.ModuleList([_Block(embed_dim, mlp_ratio) for _ in range(depth)])
        self.norm = nn.LayerNorm(embed_dim, eps=1e-6)
        nn.init.trunc_normal_(self.pos_embed, std=0.02)
        for m in self.modules():      # timm ViT init: trunc-normal(0.02) Linear weights, zero biases; conv keeps torch default
            if isinstance(m, nn.Linear):
                nn.init.trunc_normal_(m.weight, std=0.02)
                nn.init.zeros_(m.bias)

    def no_weight_decay(self):
        return {'pos_embed', 'cls_token', 'dist_token'}


class DecoderLayer(_Holder):
    """Parameter layout of the reference's two-stream pre-LN decoder layer (modules.py:27-52)."""

    def __init__(self, d_model, nhead, dim_feedforward, dropout=0.1, layer_norm_eps=1e-5):
        super().__init__()
        self.self_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True)
        self.cross_attn = nn.MultiheadAttention(d_model, nhead, dropout=dropout, batch_first=True)
        self.linear1 = nn.Linear(d_model, dim_feedforward)
        self.linear2 = nn.Linear(dim_feedforward, d_model)
        self.norm1 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.norm2 = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.norm_q = nn.LayerNorm(d_model, eps=layer_norm_eps)
        self.norm_c = nn.LayerNorm(d_model, eps=layer_norm_eps)


class Decoder(_Holder):
    def __init__(self, d_model, nhead, dim_feedforward, dropout, num_layers):
        super().__init__()
        self.layers = nn.ModuleList([DecoderLayer(d_model, nhead, dim_feedforward, dropout) for _ in range(num_layers)])
        self.num_layers = num_layers
        self.norm = nn.LayerNorm(d_model)


class TokenEmbedding(_Holder):
    def __init__(self, charset_size: int, embed_dim: int):
        super().__init__()
        self.embedding = nn.Embedding(charset_size, embed_dim)
        self.embed_dim = embed_dim


def _named_apply(fn, module: nn.Module, name: str = ''):
    for child_name, child in module.named_children():
        full = f'{name}.{child_name}' if name else child_name
        _named_apply(fn, child, full)
        fn(module=child, name=full)


class _Head(nn.Linear):
    """`model.head` (model.py:63): a Linear whose forward runs on the HIP library (fp32 GEMM), so that the reference idiom
    `model.head(model.decode(...))` works; parameters under the reference keys `head.weight` / `head.bias`."""

    def forward(self, x: Tensor) -> Tensor:
        if not x.is_cuda:
            raise RuntimeError('parseq_amd runs on MI355X through libparseq_hip only (no CPU fallback)')
        a = x.detach().to(torch.float32).contiguous().view(-1, self.in_features)
        out = torch.empty(a.shape[0], self.out_features, dtype=torch.float32, device=x.device)
        w = self.weight.detach().to(torch.float32).contiguous()
        b = self.bias.detach().to(torch.float32).contiguous()
        with _native.guard(a):
            _native.check(_native.lib().parseq_op_linear(_native.ptr(a), _native.ptr(w), _native.ptr(b), _native.ptr(out), _native.PARSEQ_F32, 0,
                                                         a.shape[0], self.out_features, self.in_features, _native.stream_ptr(a)))
        return out.view(*x.shape[:-1], self.out_features)


class _NativeState:
    """Device-side twin of the parameters: one parseq_model + cached plans.  Rebuilt when parameters move or change."""

    def __init__(self):
        self.model = C.c_void_p(0)
        self.plans = {}            # (precision code, slot) -> (plan handle, max_batch)
        self.signature = None
        self.param_order = None    # (native model handle, [(state_dict key, numel)] in the library's parameter order)
        self.epoch = 0             # bumped whenever a plan's device-side contents may have changed under an unchanged signature:
                                   # plans created / destroyed / re-packed (re-upload, mark_dirty, an optimiser step on the device)

    def release(self):
        try:
            lib = _native.lib()
        except Exception:
            return
        for plan, _ in self.plans.values():
            lib.parseq_plan_destroy(plan)
        self.plans = {}
        if self.model:
            lib.parseq_model_destroy(self.model)
        self.model = C.c_void_p(0)
        self.signature = None
        self.epoch += 1

    def __del__(self):
        self.release()


class _NativeBacked(nn.Module):
    """A parameter container whose arithmetic lives in libparseq_hip: keeps a device-side twin of the parameters
    (`parseq_model`) and cached workspaces (`parseq_plan`) in step with the module's tensors.  Subclasses provide
    `_cfg` (dict with at least 'img_size'), `precision`, and `_make_native_config()`."""

    @property
    def _device(self) -> torch.device:
        return next(self.parameters()).device

    def _make_native_config(self):  # pragma: no cover
        raise NotImplementedError

    def set_profiling(self, enable: bool, batch: int) -> None:
        """Bracket every kernel launch with HIP events (per-family timing for the roofline report; perturbs throughput)."""
        with _native.guard(self._device):
            _native.check(_native.lib().parseq_plan_set_profiling(self._plan(batch), 1 if enable else 0))

    def get_profile(self, batch: int) -> dict:
        """{family: (total_ms, launches)} accumulated since set_profiling(True)."""
        lib, plan, out, i = _native.lib(), self._plan(batch), {}, 0
        while True:
            name, ms, n = C.c_char_p(), C.c_double(), C.c_int64()
            status = lib.parseq_plan_get_profile(plan, i, C.byref(name), C.byref(ms), C.byref(n))
            if status == 1:
                break
            _native.check(status)
            out[name.value.decode()] = (ms.value, n.value)
            i += 1
        return out

    def _check_images(self, images: Tensor) -> Tensor:
        if not isinstance(images, Tensor) or images.dim() != 4:
            raise RuntimeError('images must be a [N, 3, H, W] tensor')
        if images.device.type != 'cuda':
            raise RuntimeError(
                'parseq_amd runs on MI355X through libparseq_hip only; got a tensor on '
                f"'{images.device}'. There is no CPU fallback (the CPU oracle under oracle/ is test infrastructure).")
        if images.device != self._device:
            raise RuntimeError(f'images on {images.device} but the model is on {self._device}')
        h, w = self._cfg['img_size']
        if tuple(images.shape[1:]) != (3, h, w):
            raise RuntimeError(f'expected images of shape [N, 3, {h}, {w}], got {list(images.shape)}')
        # uint8 = raw pixels: the reference transform's ToTensor + Normalize(0.5, 0.5) (strhub/data/module.py:78-81) is
        # applied inside the patch-embed kernel (row N2); float tensors are taken as already normalised
        if images.dtype not in (torch.float32, torch.bfloat16, torch.uint8):
            images = images.float()
        return images.contiguous()

    @staticmethod
    def _version_of(t: Tensor):
        """In-place-modification counter, or None for tensors that do not keep one (created under torch.inference_mode): an
        in-place edit of such a tensor cannot be noticed, so it is never taken as "unchanged"."""
        return None if t.is_inference() else t._version

    def _signature(self):
        # device, storage addresses and autograd versions of every parameter: load_state_dict, .to(), optimiser steps and
        # in-place ops (also under no_grad) change it; writes through `param.data` do not bump the version and are NOT seen
        params = list(self.parameters())
        return (str(self._device), tuple(p.data_ptr() for p in params), tuple(self._version_of(p) for p in params))

    @staticmethod
    def _trackable(sig) -> bool:
        """False when a parameter keeps no version counter (a tensor created under torch.inference_mode): an in-place edit of it
        could not be noticed, so such a signature never counts as "unchanged" and every call re-uploads (slow, never stale)."""
        return sig is not None and all(v is not None for v in sig[2])

    def mark_dirty(self):
        """Force the next forward / encode / decode to re-upload every parameter.  Needed only after writes the signature cannot
        see: in-place edits through `param.data` (checkpoint averaging, EMA) do not bump a tensor's version counter."""
        self._native_state.signature = None

    def _sync_native(self):
        st: _NativeState = self._native_state
        sig = self._signature()
        if st.signature == sig and self._trackable(sig):
            return st
        if not self._trackable(sig) and not getattr(self, '_warned_untracked', False):
            import warnings
            warnings.warn('parseq_amd: a parameter was created under torch.inference_mode and keeps no version counter; in-place edits of it '
                          'cannot be detected, so every call re-uploads the weights. Create / load the model outside inference_mode.')
            self._warned_untracked = True
        lib = _native.lib()
        if self._device.type != 'cuda':
            raise RuntimeError('move the model to a ROCm device first: model.to("cuda")')
        with torch.cuda.device(self._device):
            fresh = (not st.model) or (st.signature is None) or st.signature[0] != sig[0]
            if fresh:
                st.release()
                cfg = self._make_native_config()
                handle = C.c_void_p(0)
                _native.check(lib.parseq_model_create(C.byref(cfg), C.byref(handle)))
                st.model = handle
            stream = _native.stream_ptr(self._device)
            sd = self.state_dict()
            n_native = lib.parseq_model_num_params(st.model)
            if n_native != len(sd):
                raise RuntimeError(f'state_dict has {len(sd)} tensors, native model expects {n_native}')
            keep = []
            for key, t in sd.items():
                t32 = t.detach().to(dtype=torch.float32).contiguous()
                keep.append(t32)
                _native.check(lib.parseq_model_set_param(st.model, key.encode(), _native.ptr(t32), t32.numel(), stream))
            for plan, _ in st.plans.values():
                _native.check(lib.parseq_plan_refresh(plan, stream))
            torch.cuda.current_stream(self._device).synchronize()    # staging copies in `keep` must outlive the async D2D copies
        st.signature = sig
        st.epoch += 1                     # every plan was re-packed (or released): cached K / V projections are stale
        return st

    def _adopt_native_weights(self):
        """After an optimiser step on the device (`parseq_adamw_step` updates the library's fp32 master weights in place): copy
        them back into this module's parameter tensors — through raw pointers, so their autograd versions, and with them the
        signature, do not change and nothing is uploaded again — and re-pack the plans' bf16 copies / decoder tables."""
        st: _NativeState = self._native_state
        lib, stream = _native.lib(), _native.stream_ptr(self._device)
        sd = self.state_dict()
        n = lib.parseq_model_num_params(st.model)
        if st.param_order is None or st.param_order[0] != st.model.value:      # the library's own parameter order, asked for once per native model
            order = []
            for i in range(n):
                key, numel = C.c_char_p(), C.c_int64()
                _native.check(lib.parseq_model_param_info(st.model, i, C.byref(key), C.byref(numel)))
                order.append((key.value.decode(), numel.value))
            st.param_order = (st.model.value, order)
        ptrs = (C.c_void_p * n)()
        for i, (key, numel) in enumerate(st.param_order[1]):
            t = sd[key]
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != numel:
                raise RuntimeError(f'parameter {key}: training needs contiguous fp32 parameters of the model\'s shape')
            ptrs[i] = t.data_ptr()
        _native.check(lib.parseq_model_get_params(st.model, ptrs, n, stream))      # one launch for all of them
        for plan, _ in st.plans.values():
            _native.check(lib.parseq_plan_refresh(plan, stream))
        st.epoch += 1                     # same signature, new weights: a cached memory K / V projection is stale

    def _plan(self, batch: int, slot: int = 0):
        if self.precision not in _PRECISIONS:
            raise RuntimeError(f"precision must be one of {sorted(_PRECISIONS)}, got '{self.precision}'")
        st = self._sync_native()
        code = _PRECISIONS[self.precision]
        plan, cap = st.plans.get((code, slot), (None, 0))
        if plan is None or batch > cap:
            lib = _native.lib()
            if plan is not None:
                torch.cuda.current_stream(self._device).synchronize()
                lib.parseq_plan_destroy(plan)
                del st.plans[(code, slot)]
            st.epoch += 1                 # a fresh plan holds nobody's K / V (and a freed handle's address may be reused)
            cap = max(8, 1 << (batch - 1).bit_length())
            handle = C.c_void_p(0)
            with torch.cuda.device(self._device):
                if os.environ.get('PARSEQ_PLAN_ALLOCATOR', 'torch') == 'torch':
                    # the plan's arena is a block of the CALLER's allocator — torch's caching allocator (parseq_plan_create_ex; SURVEY.md section 8(b)'s
                    # ownership clause) — the default since round 6; PARSEQ_PLAN_ALLOCATOR=hip opts out to a hipMalloc outside it
                    if getattr(st, 'allocator', None) is None:
                        st.allocator = _native.TorchPlanAllocator(self._device)
                    _native.check(lib.parseq_plan_create_ex(st.model, cap, code, _native.stream_ptr(self._device), st.allocator.alloc_ptr, st.allocator.release_ptr,
                                                            None, C.byref(handle)))
                else:
                    _native.check(lib.parseq_plan_create(st.model, cap, code, _native.stream_ptr(self._device), C.byref(handle)))
            st.plans[(code, slot)] = (handle, cap)
            plan = handle
        return plan

    def _apply(self, fn, *args, **kwargs):
        out = super()._apply(fn, *args, **kwargs)
        st = getattr(self, '_native_state', None)
        if st is not None:
            st.signature = None if st.signature is None else (st.signature[0], (), ())   # force a re-sync
        return out


class PARSeq(_NativeBacked):

    def __init__(self, num_tokens: int, max_label_length: int, img_size: Sequence[int], patch_size: Sequence[int],
                 embed_dim: int, enc_num_heads: int, enc_mlp_ratio: int, enc_depth: int, dec_num_heads: int,
                 dec_mlp_ratio: int, dec_depth: int, decode_ar: bool, refine_iters: int, dropout: float,
                 precision: Optional[str] = None) -> None:
        super().__init__()
        self.max_label_length = max_label_length
        self.decode_ar = decode_ar
        self.refine_iters = refine_iters
        self.precision = precision or os.environ.get('PARSEQ_AMD_PRECISION', 'bf16x3')      # the mode that meets the reference within 1e-3; 'bf16' = throughput mode
        self._cfg = dict(num_tokens=num_tokens, img_size=tuple(img_size), patch_size=tuple(patch_size), embed_dim=embed_dim,
                         enc_num_heads=enc_num_heads, enc_mlp_ratio=enc_mlp_ratio, enc_depth=enc_depth,
                         dec_num_heads=dec_num_heads, dec_mlp_ratio=dec_mlp_ratio, dec_depth=dec_depth)

        self.encoder = Encoder(img_size, patch_size, embed_dim, enc_depth, enc_num_heads, enc_mlp_ratio)
        self.decoder = Decoder(embed_dim, dec_num_heads, embed_dim * dec_mlp_ratio, dropout, dec_depth)
        self.head = _Head(embed_dim, num_tokens - 2)           # <bos> and <pad> are never predicted (model.py:62-63)
        self.text_embed = TokenEmbedding(num_tokens, embed_dim)
        self.pos_queries = nn.Parameter(torch.empty(1, max_label_length + 1, embed_dim))
        _named_apply(lambda module, name: init_weights(module, name, exclude=['encoder']), self)
        nn.init.trunc_normal_(self.pos_queries, std=0.02)
        object.__setattr__(self, '_native_state', _NativeState())

    # ---- reference surface -------------------------------------------------------------------------------------
    @property
    def _device(self) -> torch.device:
        return self.head.weight.device

    def no_weight_decay(self):
        return {'text_embed.embedding.weight', 'pos_queries'} | {'encoder.' + n for n in self.encoder.no_weight_decay()}

    def encode(self, img: Tensor) -> Tensor:
        """images [B, 3, H, W] -> memory [B, tokens, E] (fp32).  model.py:83-84."""
        img = self._check_images(img)
        plan = self._plan(img.shape[0])
        memory = torch.empty(img.shape[0], self.encoder.pos_embed.shape[1], self._cfg['embed_dim'],
                             dtype=torch.float32, device=img.device)
        _native.check(_native.lib().parseq_encode(plan, _native.ptr(img), _native.dtype_code(img.dtype), img.shape[0],
                                                  _native.ptr(memory), _native.stream_ptr(self._device)))
        self._remember_memory(memory, plan)      # the K / V projection of THIS tensor object is what THIS plan now caches
        return memory

    def _bind_memory(self, memory: Optional[Tensor], B: int, plan) -> None:
        """Make the plan's cross-attention K / V those of `memory` (model.py:89).  `None`, or the very tensor the last
        `encode` on this model returned (same storage, unmodified since), means the cached projection is already right;
        anything else — another batch's memory, an edited tensor, a memory produced elsewhere — is re-projected
        (`parseq_set_memory`), never silently ignored."""
        if memory is None:
            return
        E = self._cfg['embed_dim']
        n_tok = self.encoder.pos_embed.shape[1]
        if memory.dim() != 3 or tuple(memory.shape) != (B, n_tok, E):
            raise RuntimeError(f'memory must be [{B}, {n_tok}, {E}], got {list(memory.shape)}')
        if memory.device != self._device:
            raise RuntimeError(f'memory on {memory.device} but the model is on {self._device}')
        key = getattr(self, '_memory_key', None)
        if key is not None and key[0]() is memory and key[1] is not None and key[1:] == (self._version_of(memory), plan.value, self._native_state.epoch):
            return
        mem = memory.detach().to(torch.float32).contiguous()
        _native.check(_native.lib().parseq_set_memory(plan, _native.ptr(mem), B, _native.stream_ptr(self._device)))
        self._memory_keep = mem                 # stays alive until the asynchronous projection has read it
        self._remember_memory(memory, plan)

    def _remember_memory(self, memory: Tensor, plan) -> None:
        # identity of the tensor OBJECT (a weak reference: a freed tensor whose storage address is reused by another one can
        # never match), its in-place-modification counter, the PLAN that holds the projection (another precision or slot is another
        # plan with its own K / V) and the state epoch (bumped by every re-upload, re-pack, optimiser step and plan creation)
        import weakref
        self._memory_key = (weakref.ref(memory), self._version_of(memory), plan.value, self._native_state.epoch)


    def decode(self, tgt: Tensor, memory: Optional[Tensor] = None, tgt_mask: Optional[Tensor] = None,
               tgt_padding_mask: Optional[Tensor] = None, tgt_query: Optional[Tensor] = None,
               tgt_query_mask: Optional[Tensor] = None) -> Tensor:
        """model.py:86-103: decoder output (after decoder.norm) [N, Lq, E] for the context tokens `tgt`.

        `memory`: the encoder output to attend to.  The tensor returned by the most recent `encode` is recognised (its K / V
        projection is still cached on the device); any other tensor is projected afresh; `None` means "the most recent
        `encode` / `forward`".  `tgt_query`: None (all positions `pos_queries[:, :L]`), a view `pos_queries[:, i:j]` (what
        `forward` and the training step pass — served from the position-query tables), or any other [N, Lq, E] / [1, Lq, E]
        tensor (projected at call time).  `tgt_mask` ([L, L], True = masked) is the content mask: a decoder deeper than one layer
        updates the content stream under it in layers 0 .. dec_depth - 2 (modules.py:116-124).  A depth-1 decoder never runs that
        update, so there it has no effect, exactly as in the reference."""
        B, L = tgt.shape
        E = self._cfg['embed_dim']
        user_query = None
        if tgt_query is None:
            q_start, q_len = 0, L
        else:
            pq = self.pos_queries
            if not isinstance(tgt_query, Tensor) or tgt_query.dim() != 3 or tgt_query.shape[-1] != E:
                raise RuntimeError(f'tgt_query must be [{B} or 1, Lq, {E}], got {list(getattr(tgt_query, "shape", []))}')
            off = (tgt_query.data_ptr() - pq.data_ptr()) // pq.element_size()
            q_len = tgt_query.shape[1]
            is_slice = (tgt_query.device == pq.device and tgt_query.dtype == pq.dtype and 0 <= off and off % E == 0 and
                        tgt_query.dim() == 3 and tgt_query.shape[-1] == E and off // E + q_len <= pq.shape[1] and
                        tgt_query.stride(-1) == 1 and tgt_query.stride(-2) == E and
                        (tgt_query.shape[0] == 1 or tgt_query.stride(0) == 0))
            if is_slice:
                q_start = off // E
            else:
                if tgt_query.dim() != 3 or tgt_query.shape[-1] != E or tgt_query.shape[0] not in (1, B):
                    raise RuntimeError(f'tgt_query must be [{B} or 1, Lq, {E}], got {list(tgt_query.shape)}')
                q_start = 0
                user_query = tgt_query.detach().to(device=self._device, dtype=torch.float32).expand(B, q_len, E).contiguous()
        plan = self._plan(B)
        self._bind_memory(memory, B, plan)
        tok = tgt.to(device=self._device, dtype=torch.int32).contiguous()
        kpm = tgt_padding_mask.to(device=self._device, dtype=torch.uint8).contiguous() if tgt_padding_mask is not None else None
        qm = tgt_query_mask.to(device=self._device, dtype=torch.uint8).contiguous() if tgt_query_mask is not None else None
        if qm is not None and tuple(qm.shape) != (q_len, L):
            raise RuntimeError(f'tgt_query_mask shape {tuple(qm.shape)} != ({q_len}, {L})')
        cm = self._content_mask(tgt_mask, L)
        hidden = torch.empty(B, q_len, E, dtype=torch.float32, device=self._device)
        logits = torch.empty(B, q_len, self._cfg['num_tokens'] - 2, dtype=torch.float32, device=self._device)
        lib, stream = _native.lib(), _native.stream_ptr(self._device)
        if cm is not None:
            _native.check(lib.parseq_decode_ex(plan, _native.ptr(tok), B, L, q_start, q_len, _native.ptr(user_query), _native.ptr(qm), _native.ptr(cm),
                                               _native.ptr(kpm), _native.ptr(hidden), _native.ptr(logits), stream))
        elif user_query is None:
            _native.check(lib.parseq_decode_hidden(plan, _native.ptr(tok), B, L, q_start, q_len, _native.ptr(qm), _native.ptr(kpm),
                                                   _native.ptr(hidden), _native.ptr(logits), stream))
        else:
            _native.check(lib.parseq_decode_query(plan, _native.ptr(tok), B, L, _native.ptr(user_query), q_len, _native.ptr(qm),
                                                  _native.ptr(kpm), _native.ptr(hidden), _native.ptr(logits), stream))
        return hidden

    def _content_mask(self, tgt_mask: Optional[Tensor], L: int) -> Optional[Tensor]:
        """The content mask as the library takes it (uint8 [L, L] on the device), or None where it has no effect: no mask, or a
        depth-1 decoder (which never updates the content stream)."""
        if tgt_mask is None or self._cfg['dec_depth'] == 1:
            return None
        cm = tgt_mask.to(device=self._device, dtype=torch.uint8).contiguous()
        if tuple(cm.shape) != (L, L):
            raise RuntimeError(f'tgt_mask shape {tuple(cm.shape)} != ({L}, {L})')
        return cm

    def decode_logits(self, tgt: Tensor, q_start: int, q_len: int, tgt_padding_mask: Optional[Tensor] = None,
                      tgt_query_mask: Optional[Tensor] = None, tgt_mask: Optional[Tensor] = None) -> Tensor:
        """head(decode(...)) for queries pos_queries[q_start:q_start+q_len] against the content tokens `tgt`
        (model.py:86-103 + :138), using the memory of the most recent `encode` / `forward` on this model.
        Per-stage parity hook; masks use torch's convention (True = masked).  `tgt_mask`: the content mask [L, L] (read by
        decoders deeper than one layer only, see `decode`)."""
        B, L = tgt.shape
        plan = self._plan(B)
        tok = tgt.to(device=self._device, dtype=torch.int32).contiguous()
        kpm = tgt_padding_mask.to(device=self._device, dtype=torch.uint8).contiguous() if tgt_padding_mask is not None else None
        qm = tgt_query_mask.to(device=self._device, dtype=torch.uint8).contiguous() if tgt_query_mask is not None else None
        if qm is not None and tuple(qm.shape) != (q_len, L):
            raise RuntimeError(f'tgt_query_mask shape {tuple(qm.shape)} != ({q_len}, {L})')
        cm = self._content_mask(tgt_mask, L)
        out = torch.empty(B, q_len, self._cfg['num_tokens'] - 2, dtype=torch.float32, device=self._device)
        if cm is not None:
            _native.check(_native.lib().parseq_decode_ex(plan, _native.ptr(tok), B, L, q_start, q_len, None, _native.ptr(qm), _native.ptr(cm),
                                                         _native.ptr(kpm), None, _native.ptr(out), _native.stream_ptr(self._device)))
            return out
        _native.check(_native.lib().parseq_decode_logits(plan, _native.ptr(tok), B, L, q_start, q_len, _native.ptr(qm),
                                                         _native.ptr(kpm), _native.ptr(out), _native.stream_ptr(self._device)))
        return out

    def forward(self, tokenizer: Tokenizer, images: Tensor, max_length: Optional[int] = None, slot: Optional[int] = None,
                return_length: bool = False):
        """model.py:105-169.  Returns logits [B, L, num_tokens - 2] (fp32).

        `return_length=True` returns `(logits_all, L)` instead: the logits of ALL `num_steps` positions (every step is always
        run on the device) and the length `L` the reference would have returned for THIS batch — what the data-parallel wrapper
        needs to reproduce the single-device early-exit length across shards (parallel.data_parallel_forward).

        `slot` selects one of several independent workspaces (plans): calls that use different slots on different
        streams may be in flight at the same time (bench.py --streams 2 overlaps the latency-bound AR decode of one batch
        with the encoder of the next).  The default (`slot=None`) is the reference's behaviour: one call at a time,
        stream-ordered, on workspace 0 — and it tells the library so (PARSEQ_FLAG_LATENCY): with the device to itself the AR step
        spreads over more compute units, a shorter dependent chain.  An explicit slot (0 included) says other batches are in flight
        and keeps the narrower step, whose compute units they need; the two forms differ by rounding only.  In `bf16x3` at 512 crops or
        more per call (PARSEQ_TILE_LOOP_MIN) an explicit slot goes further: the whole AR loop is one launch in which a workgroup owns 16
        crops (csrc/decoder_tile_loop.h) — a third of the compute-unit time, but a decode chain of about 4.5 ms instead of 1.7 ms, so it
        pays only with other batches in flight; a caller that passes a slot but keeps one batch in flight should not (or sets
        PARSEQ_NO_TILE_LOOP=1)."""
        testing = max_length is None
        num_steps = self._num_steps(max_length)
        images = self._check_images(images)
        B = images.shape[0]
        plan = self._plan(B, 0 if slot is None else slot)
        self._memory_replaced(plan)
        self._check_tokenizer(tokenizer)
        logits = torch.empty(B, num_steps, self._cfg['num_tokens'] - 2, dtype=torch.float32, device=images.device)
        flags = ((_native.FLAG_DECODE_AR if self.decode_ar else 0) | (_native.FLAG_TESTING if testing else 0)
                 | (_native.FLAG_LATENCY if slot is None else 0))
        out_len = C.c_int(0)
        _native.check(_native.lib().parseq_forward(plan, _native.ptr(images), _native.dtype_code(images.dtype), B, flags,
                                                   int(self.refine_iters), num_steps, _native.ptr(logits),
                                                   C.byref(out_len), _native.stream_ptr(self._device)))
        if return_length:
            return logits, out_len.value
        return logits if out_len.value == num_steps else logits[:, :out_len.value]

    def beam_search(self, tokenizer: Tokenizer, images: Tensor, beam_width: int, max_length: Optional[int] = None,
                    trace: bool = False, lexicon=None, roots: Optional[Tensor] = None, refine: Optional[str] = None,
                    refine_iters: int = 1, automaton=None, alpha: float = 1.0, beta: float = 0.0) -> BeamResult:
        """Beam-search AR decoding with N-best output (the reference has none): the `beam_width` best hypotheses
        of every crop with their log-probabilities, best first, no refinement.  One library call on a plan of B * beam_width rows, no
        host synchronisation; the result stays on the device (`tokenizer.decode_beams` reads it).  `max_length` as in `forward`, except
        that all min(max_length, max_label_length) + 1 steps always run.  Afterwards the plan's cached memory K / V are the replicated
        batch's, as after any `forward`.

        `lexicon` (a `parseq_amd.lexicon.Lexicon`) constrains the search to prefixes of its words, the scores staying
        the model's log-probabilities; `roots` (int32 [B], from `Lexicon.forest`) gives every crop its own trie, none means node 0.  The
        result is then a `LexiconBeamResult` whose `words` index `lexicon.words`.

        `refine` runs the model's cloze refinement on every hypothesis after the search, in the same library call:
        'score' keeps the readings and replaces their scores by the pseudo-log-likelihood (every character given all the others), 'edit'
        replaces every reading by its refined one, `refine_iters` times, and merges equal readings.  Either way the hypotheses are ranked
        again by the new `scores`, and `ar_scores` holds the search's own.  Under a lexicon only 'score' is allowed.

        `automaton` (a `parseq_amd.automaton.Automaton`) is a soft prior instead: a weighted word list, a character
        n-gram model or a pattern.  The search walks its table as it walks a lexicon's (`roots` gives every crop its start state) and ranks
        by the model's score plus `alpha` times the weights along the path plus `beta` per character.  The result is a `LexiconBeamResult`
        whose `scores` are those fused values, with `model_scores`, `priors` and `words` (the accept tags) beside them.  It excludes
        `lexicon` and `refine`."""
        check_beam_refine(refine, refine_iters, lexicon)
        W = int(beam_width)
        classes = self._cfg['num_tokens'] - 2
        check_beam_automaton(automaton, alpha, beta, lexicon, refine, classes)
        if self._cfg['dec_depth'] != 1:
            raise ValueError(f"beam_search needs dec_depth == 1, this model has dec_depth = {self._cfg['dec_depth']} (a deeper decoder's "
                             'per-layer content cache would have to be re-parented)')
        if not 1 <= W <= min(BEAM_MAX_WIDTH, classes):
            raise ValueError(f'beam_width must be in [1, {min(BEAM_MAX_WIDTH, classes)}] ({BEAM_MAX_WIDTH} at most, and no more than the {classes} classes), got {beam_width}')
        if lexicon is None and automaton is None and roots is not None:
            raise ValueError('beam_search: roots without a lexicon')
        if lexicon is not None and (lexicon.next.dim() != 2 or lexicon.next.shape[1] != classes or lexicon.next.dtype != torch.int32
                                    or lexicon.next.shape[0] < 1):
            raise ValueError(f'beam_search: the lexicon table must be int32 [nodes, {classes}] (one column per head class), got '
                             f'{lexicon.next.dtype} {tuple(lexicon.next.shape)}')
        if roots is not None and (roots.dim() != 1 or roots.shape[0] != images.shape[0]):
            raise ValueError(f'beam_search: roots must be [batch] = [{images.shape[0]}], got {tuple(roots.shape)}')
        num_steps = self._num_steps(max_length)
        images = self._check_images(images)
        B = images.shape[0]
        plan = self._plan(B * W)
        self._memory_replaced()                  # by the replicated batch's
        self._check_tokenizer(tokenizer)
        lib, dev = _native.lib(), images.device
        res = (BeamResult if lexicon is None and automaton is None else LexiconBeamResult)(
            torch.empty(B, W, num_steps, dtype=torch.int32, device=dev), torch.empty(B, W, dtype=torch.float32, device=dev),
            torch.empty(B, W, dtype=torch.int32, device=dev), torch.empty(B, W, dtype=torch.uint8, device=dev))
        tr = rtr = table = None
        if trace:
            res.trace_logits = torch.empty(num_steps, B * W, classes, dtype=torch.float32, device=dev)
            res.trace_tokens_in = torch.empty(num_steps, B * W, num_steps, dtype=torch.int32, device=dev)
            res.trace_parent = torch.empty(num_steps, B * W, dtype=torch.int32, device=dev)
            res.trace_score = torch.empty(num_steps, B * W, dtype=torch.float32, device=dev)
            tr = _native.BeamTrace(res.trace_logits.data_ptr(), res.trace_tokens_in.data_ptr(), res.trace_parent.data_ptr(), res.trace_score.data_ptr())
        if lexicon is not None:
            table = lexicon.table(dev)
            if roots is not None:
                roots = roots.to(dev, torch.int32).contiguous()
            res.words = torch.empty(B, W, dtype=torch.int32, device=dev)
        if automaton is not None:
            table, weight = automaton.table(dev)
            if roots is not None:
                roots = roots.to(dev, torch.int32).contiguous()
            res.words = torch.empty(B, W, dtype=torch.int32, device=dev)
            res.model_scores = torch.empty(B, W, dtype=torch.float32, device=dev)
            res.priors = torch.empty(B, W, dtype=torch.float32, device=dev)
        if refine is not None:
            res.ar_scores = torch.empty(B, W, dtype=torch.float32, device=dev)
            if trace:
                res.trace_refine_tokens_in = torch.empty(refine_iters, B * W, num_steps, dtype=torch.int32, device=dev)
                res.trace_refine_logits = torch.empty(refine_iters, B * W, num_steps, classes, dtype=torch.float32, device=dev)
                rtr = _native.BeamRefineTrace(res.trace_refine_tokens_in.data_ptr(), res.trace_refine_logits.data_ptr())
        # the entry of this combination, its workspace, and what it takes after the arguments all three share
        lex_args = [None, 0, None, None] if table is None else [_native.ptr(table), table.shape[0], _native.ptr(roots), _native.ptr(res.words)]
        if refine is not None:
            entry, ws = lib.parseq_forward_beam_refine, self._workspace(lib.parseq_beam_refine_workspace_bytes, plan, B, W, num_steps, int(table is not None))
            extra = lex_args + [BEAM_REFINE_MODES[refine], refine_iters, _native.ptr(res.ar_scores), C.byref(rtr) if rtr is not None else None]
        elif automaton is not None:
            entry, ws = lib.parseq_forward_beam_automaton, self._workspace(lib.parseq_beam_automaton_workspace_bytes, plan, B, W, num_steps)
            extra = [_native.ptr(table), _native.ptr(weight), table.shape[0], _native.ptr(roots), float(alpha), float(beta), _native.ptr(res.words),
                     _native.ptr(res.model_scores), _native.ptr(res.priors)]
        elif lexicon is not None:
            entry, ws, extra = lib.parseq_forward_beam_lexicon, self._workspace(lib.parseq_beam_lexicon_workspace_bytes, plan, B, W, num_steps), lex_args
        else:
            entry, ws, extra = lib.parseq_forward_beam, self._workspace(lib.parseq_beam_workspace_bytes, plan, B, W, num_steps), []
        _native.check(entry(plan, _native.ptr(images), _native.dtype_code(images.dtype), B, W, num_steps, _native.ptr(res.tokens), _native.ptr(res.scores),
                            _native.ptr(res.lengths), _native.ptr(res.finished), C.byref(tr) if tr is not None else None, _native.ptr(ws), ws.numel(),
                            _native.stream_ptr(self._device), *extra))
        return res

    def lexicon_match(self, tokenizer: Tokenizer, images: Tensor, lexicon, n: int, lists=None, rescore: bool = True, keep_reading: bool = False,
                      ignore_case: bool = False) -> LexiconMatchResult:
        """Read freely, then choose among the list's nearest words: the reading `forward` gives for `images`, the `n`
        words of `lexicon` nearest to it in Levenshtein distance, and — with `rescore` — the pseudo-log-likelihood of each of them
        (section 20's 'score'), best first; without it they stay in (distance, word id) order.  `lists` (a list index of `Lexicon.forest`
        per crop) gives every crop its own list.  `keep_reading` lets the reading itself compete (word -1) unless it is a word of the list.
        `ignore_case` matches a cased charset against the list case-insensitively; what is scored is the word's own spelling.  One library
        call on a plan of B * W rows, no host synchronisation; `tokenizer.decode_beams(result, lexicon)` reads the result."""
        classes = self._cfg['num_tokens'] - 2
        self._check_localizable('lexicon_match')
        check_lexicon_match(n, keep_reading, lexicon, self.max_label_length, classes)
        images = self._check_images(images)
        B, dev = images.shape[0], images.device
        W, L = n + (1 if keep_reading else 0), self.max_label_length + 1
        t = lexicon.match_table(dev, ignore_case)
        ranges = lexicon.crop_ranges(lists, B, dev)
        plan = self._plan(B * W)
        self._memory_replaced()
        self._check_tokenizer(tokenizer)
        res = LexiconMatchResult(
            torch.empty(B, W, L, dtype=torch.int32, device=dev), torch.empty(B, W, dtype=torch.float32, device=dev),
            torch.empty(B, W, dtype=torch.int32, device=dev), torch.empty(B, W, dtype=torch.uint8, device=dev),
            words=torch.empty(B, W, dtype=torch.int32, device=dev), distances=torch.empty(B, W, dtype=torch.int32, device=dev),
            reading_tokens=torch.empty(B, L, dtype=torch.int32, device=dev), reading_lengths=torch.empty(B, dtype=torch.int32, device=dev))
        args = _native.LexiconMatchArgs(t['table'].data_ptr(), t['own'].data_ptr(), t['row_ids'].data_ptr(), ranges.data_ptr() if ranges is not None else None,
                                        t['fold'].data_ptr() if t['fold'] is not None else None, lexicon.num_rows, n, int(bool(rescore)), int(bool(keep_reading)))
        lib = _native.lib()
        ws = self._workspace(lib.parseq_forward_lexicon_match_workspace_bytes, plan, B, C.byref(args))
        flags = (_native.FLAG_DECODE_AR if self.decode_ar else 0) | _native.FLAG_LATENCY
        _native.check(lib.parseq_forward_lexicon_match(plan, _native.ptr(images), _native.dtype_code(images.dtype), B, flags, int(self.refine_iters), C.byref(args),
                                                       _native.ptr(res.tokens), _native.ptr(res.scores), _native.ptr(res.lengths), _native.ptr(res.finished),
                                                       _native.ptr(res.words), _native.ptr(res.distances), _native.ptr(res.reading_tokens),
                                                       _native.ptr(res.reading_lengths), _native.ptr(ws), ws.numel(), _native.stream_ptr(self._device)))
        return res

    def orient(self, tokenizer: Tokenizer, views: Tensor, criterion: str = 'mean', prior=None, max_length: Optional[int] = None,
               slot: Optional[int] = None) -> OrientedResult:
        """Orientation-robust reading: `views` [B, K, 3, H, W] holds K turned views of every crop
        (`preprocess.orientation_views` makes them); all B * K rows go through one `forward` — every position, the early exit never applies —
        and of each crop the view with the largest key wins: the length-normalised log-probability of its reading ('mean'), or its sum
        ('sum', the log of the reference's confidence), plus `prior[k]` (K values in nats).  Ties go to the lowest view.  One library call,
        no host synchronisation; everything stays on the device.  `max_length` and `slot` as in `forward`."""
        B, K, prior = check_orient(tuple(getattr(views, 'shape', ())), criterion, prior)
        num_steps = self._num_steps(max_length)
        images = self._check_images(views.flatten(0, 1))
        plan = self._plan(B * K, 0 if slot is None else slot)
        self._memory_replaced(plan)
        self._check_tokenizer(tokenizer)
        dev, C_ = images.device, self._cfg['num_tokens'] - 2
        pr = torch.tensor(prior, dtype=torch.float32).to(dev) if prior is not None else None
        res = OrientedResult(torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, K, dtype=torch.float64, device=dev),
                             torch.empty(B, num_steps, C_, dtype=torch.float32, device=dev), torch.empty(B, num_steps, dtype=torch.int32, device=dev),
                             torch.empty(B, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.float32, device=dev),
                             torch.empty((B,) + tuple(images.shape[1:]), dtype=images.dtype, device=dev))
        lib = _native.lib()
        ws = self._workspace(lib.parseq_forward_oriented_workspace_bytes, plan, B, K, num_steps)
        flags = (_native.FLAG_DECODE_AR if self.decode_ar else 0) | (_native.FLAG_LATENCY if slot is None else 0)
        _native.check(lib.parseq_forward_oriented(plan, _native.ptr(images), _native.dtype_code(images.dtype), B, K, flags, int(self.refine_iters), num_steps,
                                                  _native.ORIENT_CRITERIA[criterion], _native.ptr(pr), _native.ptr(res.view), _native.ptr(res.keys),
                                                  _native.ptr(res.logits), _native.ptr(res.ids), _native.ptr(res.lengths), _native.ptr(res.confidence),
                                                  _native.ptr(res.images), _native.ptr(ws), ws.numel(), _native.stream_ptr(self._device)))
        return res

    def score(self, tokenizer: Tokenizer, images: Tensor, candidates: Tensor, masks: Tensor, flags: int = 0, char_logprobs: bool = True):
        """The joint log-probability of given readings: `candidates` int32 [B, N, L] rows `c_0 .. c_{n-1}, <eos>,
        <pad> ..` (a first <pad>: absent) and `masks` uint8 [K, L, L], the query mask of every decoding order, both on the device.  One
        library call on a plan of B * N rows — encode once, K teacher-forced decoder passes, the combination and the rank — no host
        synchronisation.  Returns (scores [B, N], order_scores [B, N, K], char_logprobs [B, N, K, L] or None, rank, lengths, valid)."""
        self._check_localizable('score')
        images = self._check_images(images)
        B, dev = images.shape[0], images.device
        if candidates.dtype != torch.int32 or candidates.ndim != 3 or candidates.shape[0] != B or not candidates.is_cuda:
            raise ValueError(f'score: candidates must be device int32 [B = {B}, N, L], got {candidates.dtype} {tuple(candidates.shape)}')
        N, L = candidates.shape[1], candidates.shape[2]
        if masks.dtype != torch.uint8 or masks.ndim != 3 or tuple(masks.shape[1:]) != (L, L) or not masks.is_cuda:
            raise ValueError(f'score: masks must be device uint8 [K, {L}, {L}], got {masks.dtype} {tuple(masks.shape)}')
        K = masks.shape[0]
        if not 1 <= N <= _native.SCORE_MAX_CANDIDATES or not 1 <= K <= _native.SCORE_MAX_ORDERS:
            raise ValueError(f'score: N = {N} candidates (1 .. {_native.SCORE_MAX_CANDIDATES}), K = {K} orders (1 .. {_native.SCORE_MAX_ORDERS})')
        candidates, masks = candidates.contiguous(), masks.contiguous()
        plan = self._plan(B * N)
        self._memory_replaced()
        self._check_tokenizer(tokenizer)
        out = (torch.empty(B, N, dtype=torch.float32, device=dev), torch.empty(B, N, K, dtype=torch.float32, device=dev),
               torch.empty(B, N, K, L, dtype=torch.float32, device=dev) if char_logprobs else None, torch.empty(B, N, dtype=torch.int32, device=dev),
               torch.empty(B, N, dtype=torch.int32, device=dev), torch.empty(B, N, dtype=torch.uint8, device=dev))
        lib = _native.lib()
        ws = self._workspace(lib.parseq_score_workspace_bytes, plan, B, N, L, K)
        _native.check(lib.parseq_score(plan, _native.ptr(images), _native.dtype_code(images.dtype), B, _native.ptr(candidates), N, L, _native.ptr(masks), K,
                                       int(flags), *[_native.ptr(t) for t in out], _native.ptr(ws), ws.numel(), _native.stream_ptr(self._device)))
        return out

    def _check_localizable(self, what: str) -> None:
        if self._cfg['dec_depth'] != 1:
            raise ValueError(f"{what} needs dec_depth == 1, this model has dec_depth = {self._cfg['dec_depth']}")

    def attention_maps(self, tokens: Tensor, memory: Optional[Tensor] = None, tgt_padding_mask: Optional[Tensor] = None) -> Tensor:
        """The map of a reading: head-averaged cross-attention [B, L, S] (fp32) of ONE cloze pass — the pass a
        refinement iteration of `forward` runs (model.py:154-167) — over `tokens` [B, L]: one reading per row, its characters, then <eos>,
        then anything; 2 <= L <= max_label_length + 1.  The content is [<bos>, tokens[:, :-1]]; `tgt_padding_mask` [B, L] (True = masked) is the
        key padding of that content, by default everything from the first <eos> on.  Row i of image b sums to 1 for i <= len(b) (the <eos>
        position included) and is zero after it.  `memory` as in `decode`."""
        self._check_localizable('attention_maps')
        if tokens.dim() != 2:
            raise RuntimeError(f'tokens must be [B, L], got {list(tokens.shape)}')
        B, L = tokens.shape
        if not 2 <= L <= self.max_label_length + 1:
            raise ValueError(f'attention_maps: {L} positions outside [2, max_label_length + 1 = {self.max_label_length + 1}]')
        plan = self._plan(B)
        self._bind_memory(memory, B, plan)
        tok = tokens.to(device=self._device, dtype=torch.int32)
        content = torch.cat([torch.full((B, 1), self._make_native_config().bos_id, dtype=torch.int32, device=self._device), tok[:, :-1]], dim=1).contiguous()
        kpm = tgt_padding_mask.to(device=self._device, dtype=torch.uint8).contiguous() if tgt_padding_mask is not None else None
        if kpm is not None and tuple(kpm.shape) != (B, L):
            raise RuntimeError(f'tgt_padding_mask shape {tuple(kpm.shape)} != ({B}, {L})')
        maps = torch.empty(B, L, self.encoder.pos_embed.shape[1], dtype=torch.float32, device=self._device)
        _native.check(_native.lib().parseq_decode_attention(plan, _native.ptr(content), B, L, _native.ptr(kpm), _native.ptr(maps), None,
                                                            _native.stream_ptr(self._device)))
        return maps

    def localize(self, tokenizer: Tokenizer, images: Tensor, labels=None) -> Localization:
        """Where every character is: the reading `forward` gives for `images` — or, with `labels` (a list of strings),
        those strings aligned instead — with the attention map, centre, box and peak of every position.  One library call, no host
        synchronisation; everything stays on the device (`tokenizer.decode_localization` reads it)."""
        self._check_localizable('localize')
        L = self.max_label_length + 1
        tok_in = None
        if labels is not None:
            labels = list(labels)
            check_labels(labels, self.max_label_length)
        images = self._check_images(images)
        B = images.shape[0]
        dev = images.device
        if labels is not None:
            if len(labels) != B:
                raise ValueError(f'localize: {len(labels)} labels for {B} images')
            enc = tokenizer.encode(labels)[:, 1:]                      # characters, <eos>, <pad>
            tok_in = torch.full((B, L), tokenizer.pad_id, dtype=torch.int32)
            tok_in[:, :enc.shape[1]] = enc
            tok_in = tok_in.to(dev)
        plan = self._plan(B)
        self._memory_replaced()
        self._check_tokenizer(tokenizer)
        S = self.encoder.pos_embed.shape[1]
        loc = Localization(torch.empty(B, L, dtype=torch.int32, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
                           torch.empty(B, L, S, dtype=torch.float32, device=dev), torch.empty(B, L, 2, dtype=torch.float32, device=dev),
                           torch.empty(B, L, 4, dtype=torch.float32, device=dev), torch.empty(B, L, dtype=torch.int32, device=dev),
                           torch.empty(B, L, dtype=torch.float32, device=dev))
        lib = _native.lib()
        ws = self._workspace(lib.parseq_localize_workspace_bytes, plan, B)
        flags = (_native.FLAG_DECODE_AR if self.decode_ar else 0) | _native.FLAG_LATENCY
        _native.check(lib.parseq_localize(plan, _native.ptr(images), _native.dtype_code(images.dtype), B, _native.ptr(tok_in), flags, int(self.refine_iters),
                                          _native.ptr(loc.tokens), _native.ptr(loc.lengths), _native.ptr(loc.maps), _native.ptr(loc.centres),
                                          _native.ptr(loc.boxes), _native.ptr(loc.peak), _native.ptr(loc.peak_mass), _native.ptr(ws), ws.numel(),
                                          _native.stream_ptr(self._device)))
        return loc

    def read_lines(self, tokenizer: Tokenizer, images, overlap: float = 0.25, aspect: float = 1.0, min_sep: float = 0.25,
                   max_chars: Optional[int] = None, max_batch: int = 512) -> LineResult:
        """Whole text lines: `images` is a list of uint8 [H, W, 3] device tensors of any width.  Every line is cut
        into the overlapping windows of `preprocess.line_windows(H, W, img_size, overlap, aspect)`; all windows of all lines are column
        slices resized in ONE `resize_batch` launch; every call of parseq_read_lines then reads, localises and stitches as many whole lines
        as fit in `max_batch` rows, without a host synchronisation.  Two readings of one character in neighbouring windows are told apart
        from a doubled letter by position: centres closer than `min_sep` line heights are the same character.  `max_chars`: the slots per
        line (default: what the windows of the longest line could hold, at most 2048)."""
        from . import preprocess
        self._check_localizable('read_lines')
        check_lines(overlap, aspect, min_sep, max_chars, max_batch)
        images = preprocess._checked(list(images), 'read_lines')
        img_size = self._cfg['img_size']
        win, first = preprocess.line_plan([(im.shape[0], im.shape[1]) for im in images], img_size, overlap, aspect)
        chunks = chunk_lines(first, max_batch)
        N, R, L, dev = len(images), len(win), self.max_label_length + 1, images[0].device
        if max_chars is None:
            max_chars = min(_native.LINE_MAX_OUT, max(first[l + 1] - first[l] for l in range(N)) * self.max_label_length)
        batch = self._check_images(preprocess.resize_batch(preprocess.line_views(images, win, first), img_size))
        plan = self._plan(max(first[b] - first[a] for a, b in chunks))
        self._memory_replaced()
        self._check_tokenizer(tokenizer)
        # one upload: the window table, every call's own line_first (counted from the call's first row) and the separations
        firsts = [first[l] - first[a] for a, b in chunks for l in range(a, b + 1)]
        table = torch.tensor([v for row in win for v in row] + firsts, dtype=torch.int32).to(dev)
        sep = torch.tensor([float(min_sep) * im.shape[0] for im in images], dtype=torch.float64).to(dev)
        win_d, firsts_d = table[:3 * R].view(R, 3), table[3 * R:]
        w = LineWindows(torch.empty(R, L, dtype=torch.int32, device=dev), torch.empty(R, dtype=torch.int32, device=dev),
                        torch.empty(R, L, 2, dtype=torch.float32, device=dev), torch.empty(R, L, 4, dtype=torch.float32, device=dev),
                        torch.empty(R, L, dtype=torch.float32, device=dev), win_d, torch.tensor(first, dtype=torch.int32).to(dev), batch)
        M = max_chars
        res = LineResult(torch.empty(N, dtype=torch.int32, device=dev), torch.empty(N, M, dtype=torch.int32, device=dev),
                         torch.empty(N, M, dtype=torch.float32, device=dev), torch.empty(N, M, 4, dtype=torch.float32, device=dev),
                         torch.empty(N, M, dtype=torch.float64, device=dev), torch.empty(N, M, 2, dtype=torch.int32, device=dev),
                         torch.empty(N, dtype=torch.float32, device=dev), w)
        lib = _native.lib()
        flags = (_native.FLAG_DECODE_AR if self.decode_ar else 0) | _native.FLAG_LATENCY
        pos = 0
        for a, b in chunks:
            r0, rows = first[a], first[b] - first[a]
            ws = self._workspace(lib.parseq_read_lines_workspace_bytes, plan, rows)
            _native.check(lib.parseq_read_lines(
                plan, _native.ptr(batch[r0:]), _native.dtype_code(batch.dtype), rows, flags, int(self.refine_iters), _native.ptr(win_d[r0:]),
                _native.ptr(firsts_d[pos:]), b - a, _native.ptr(sep[a:]), M, _native.ptr(w.tokens[r0:]), _native.ptr(w.lengths[r0:]), _native.ptr(w.probs[r0:]),
                _native.ptr(w.centres[r0:]), _native.ptr(w.boxes[r0:]), _native.ptr(res.lengths[a:]), _native.ptr(res.tokens[a:]), _native.ptr(res.probs[a:]),
                _native.ptr(res.boxes[a:]), _native.ptr(res.x[a:]), _native.ptr(res.src[a:]), _native.ptr(res.confidence[a:]), _native.ptr(ws), ws.numel(),
                _native.stream_ptr(self._device)))
            pos += b - a + 1
        return res

    # ---- native plumbing ---------------------------------------------------------------------------------------
    def _special_ids(self, tokenizer):
        self._tok_ids = getattr(self, '_tok_ids', None) or (tokenizer.bos_id, tokenizer.eos_id, tokenizer.pad_id)
        return self._tok_ids

    def _check_tokenizer(self, tokenizer) -> None:
        if (tokenizer.bos_id, tokenizer.eos_id, tokenizer.pad_id) != self._special_ids(tokenizer):
            raise RuntimeError('tokenizer special ids changed after the native model was built')

    def _num_steps(self, max_length: Optional[int]) -> int:
        """`max_length` as `forward` takes it (None: the model's) -> the positions decoded, the <eos> included."""
        return (self.max_label_length if max_length is None else min(max_length, self.max_label_length)) + 1

    def _memory_replaced(self, plan=None) -> None:
        """A call that encodes its own images: the plan's cached K / V now belong to them, not to an `encode()` result.  With `plan`,
        only if the remembered memory is that plan's (`forward` on another slot leaves it alone)."""
        key = getattr(self, '_memory_key', None)
        if plan is None or (key is not None and key[2] == plan.value):
            self._memory_key = None

    def _workspace(self, sizer, *args) -> Tensor:
        """The caller's workspace of a library call, sized by its `*_workspace_bytes` function (0: a refusal, raised with the library's
        message): a block of torch's caching allocator, stream-ordered."""
        nbytes = sizer(*args)
        if nbytes == 0:
            _native.check(-1)
        return torch.empty(nbytes, dtype=torch.uint8, device=self._device)

    def _make_native_config(self):
        tok_ids = getattr(self, '_tok_ids', None)
        if tok_ids is None:
            n = self._cfg['num_tokens']
            tok_ids = (n - 2, 0, n - 1)      # Tokenizer layout: [E]=0 ... [B]=n-2, [P]=n-1 (strhub/data/utils.py:107-111)
            self._tok_ids = tok_ids
        c = self._cfg
        return _native.ParseqConfig(
            img_h=c['img_size'][0], img_w=c['img_size'][1], patch_h=c['patch_size'][0], patch_w=c['patch_size'][1],
            embed_dim=c['embed_dim'], enc_depth=c['enc_depth'], enc_heads=c['enc_num_heads'],
            enc_mlp_ratio=c['enc_mlp_ratio'], dec_depth=c['dec_depth'], dec_heads=c['dec_num_heads'],
            dec_mlp_ratio=c['dec_mlp_ratio'], num_tokens=c['num_tokens'], max_label_length=self.max_label_length,
            bos_id=tok_ids[0], eos_id=tok_ids[1], pad_id=tok_ids[2], enc_ln_eps=1e-6, dec_ln_eps=1e-5,
            arch=_native.ARCH_PARSEQ)
