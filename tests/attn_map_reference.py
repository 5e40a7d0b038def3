"""CPU restatement of character localisation.   *** TEST INFRASTRUCTURE ***

`attention_map` restates the cloze pass of the reference's refinement iteration (strhub/models/parseq/model.py:154-167 through
modules.py:55-79) up to the last layer's cross-attention of the query stream and returns what `DecoderLayer.forward_stream` calls
`ca_weights`: the soft-max probabilities averaged over the heads (nn.MultiheadAttention's `average_attn_weights`).  It is built on the
oracle's `_ln` / `_linear` / `token_embedding` (and `encode` for the memory) and pinned by tests/golden/attn_*.npz, which
tools/make_golden_attn.py mints by running the reference's own forward.  `geometry` restates the reduction of a map to centres, boxes
and peaks in NumPy float64.
"""
from __future__ import annotations

import json
import math
import os

import numpy as np
import torch

from oracle.parseq_oracle import _linear, _ln, _r, encode, token_embedding  # noqa: F401  (encode: re-exported for the tests)


GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
GRIDS = [(8, 16, 4, 8), (14, 14, 16, 16)]      # (gh, gw, ph, pw): PARSeq 32 x 128 / patch 4 x 8, patch16-224


def load_attn_golden(name):
    """(arrays, settings) of tests/golden/attn_<name>.* (tools/make_golden_attn.py)."""
    with open(os.path.join(GOLDEN_DIR, f'attn_{name}.json')) as f:
        meta = json.load(f)
    return np.load(os.path.join(GOLDEN_DIR, f'attn_{name}.npz')), meta


def block_map(gh, gw, r0, c0, k, m):
    """[1, 1, S]: uniform over rows r0 .. r0 + k - 1, columns c0 .. c0 + m - 1."""
    a = np.zeros((gh, gw))
    a[r0:r0 + k, c0:c0 + m] = 1.0 / (k * m)
    return a.reshape(1, 1, gh * gw)


def content_of(cfg, tokens: torch.Tensor) -> torch.Tensor:
    """[<bos>, tokens[:, :-1]]: the content rows of a batch of readings [B, L] (characters, <eos>, anything)."""
    bos = torch.full((tokens.shape[0], 1), cfg.bos_id, dtype=torch.long)
    return torch.cat([bos, tokens[:, :-1].long()], dim=1)


def cross_attention_queries(sd: dict, cfg, tgt_in: torch.Tensor, rounding=None, tgt_padding_mask=None) -> torch.Tensor:
    """The projected, unscaled cross-attention queries [B, L, E] of the cloze pass over the content rows `tgt_in` [B, L] (<bos> first):
    at depth 1 they depend on the content and the position queries alone, not on the memory."""
    assert cfg.dec_depth == 1
    tgt_in = tgt_in.long()
    B, L = tgt_in.shape
    E, H = cfg.embed_dim, cfg.dec_num_heads
    hd = E // H
    p = 'decoder.layers.0.'
    eps = cfg.dec_ln_eps
    if tgt_padding_mask is None:
        tgt_padding_mask = (tgt_in == cfg.eos_id).int().cumsum(-1) > 0                     # model.py:163
    query_mask = torch.triu(torch.ones(L, L, dtype=torch.bool), 1)                         # model.py:117, 157: the cloze mask
    query_mask[torch.triu(torch.ones(L, L, dtype=torch.bool), 2)] = False
    pos_queries = sd['pos_queries']
    content = torch.cat([token_embedding(sd, cfg, tgt_in[:, :1]), pos_queries[:, :L - 1] + token_embedding(sd, cfg, tgt_in[:, 1:])], dim=1)
    query = pos_queries[:, :L].expand(B, -1, -1)
    # self-attention of the query stream (modules.py:61-65)
    qn = _ln(query, sd[p + 'norm_q.weight'], sd[p + 'norm_q.bias'], eps)
    cn = _ln(content, sd[p + 'norm_c.weight'], sd[p + 'norm_c.bias'], eps)
    w, b = sd[p + 'self_attn.in_proj_weight'], sd[p + 'self_attn.in_proj_bias']
    q = _linear(qn, w[:E], b[:E], rounding)
    kv = _linear(cn, w[E:], b[E:], rounding)
    k, v = _r(kv[..., :E], rounding, 'dec.kv'), _r(kv[..., E:], rounding, 'dec.kv')
    heads = lambda t: t.reshape(B, -1, H, hd).transpose(1, 2)                               # noqa: E731
    s = (heads(q) * math.sqrt(1.0 / hd)) @ heads(k).transpose(-2, -1)
    s = s.masked_fill(query_mask[None, None], float('-inf')).masked_fill(tgt_padding_mask[:, None, None, :], float('-inf'))
    o = (torch.softmax(s, -1) @ heads(v)).transpose(1, 2).reshape(B, L, E)
    t = query + _linear(o, sd[p + 'self_attn.out_proj.weight'], sd[p + 'self_attn.out_proj.bias'], rounding)
    # the query of the cross-attention (modules.py:66-68)
    w, b = sd[p + 'cross_attn.in_proj_weight'], sd[p + 'cross_attn.in_proj_bias']
    return _linear(_ln(t, sd[p + 'norm1.weight'], sd[p + 'norm1.bias'], eps), w[:E], b[:E], rounding)


def attention_map(sd: dict, cfg, tgt_in: torch.Tensor, memory: torch.Tensor, rounding=None, tgt_padding_mask=None) -> torch.Tensor:
    """The head-averaged cross-attention [B, L, S] of the cloze pass over the content rows `tgt_in` [B, L] (<bos> first).  Rows at
    padded positions (from one past the <eos> position on) are zero."""
    tgt_in = tgt_in.long()
    B, L = tgt_in.shape
    E, H = cfg.embed_dim, cfg.dec_num_heads
    hd = E // H
    if tgt_padding_mask is None:
        tgt_padding_mask = (tgt_in == cfg.eos_id).int().cumsum(-1) > 0
    q = cross_attention_queries(sd, cfg, tgt_in, rounding, tgt_padding_mask)
    w, b = sd['decoder.layers.0.cross_attn.in_proj_weight'], sd['decoder.layers.0.cross_attn.in_proj_bias']
    k = _r(_linear(memory, w[E:2 * E], b[E:2 * E], rounding), rounding, 'dec.kv')
    heads = lambda t: t.reshape(B, -1, H, hd).transpose(1, 2)                               # noqa: E731
    s = (heads(q) * math.sqrt(1.0 / hd)) @ heads(k).transpose(-2, -1)
    a = torch.softmax(s, -1).mean(dim=1)                                                   # average_attn_weights over the heads
    return a.masked_fill(tgt_padding_mask[:, :, None], 0.0)


def geometry(maps, lengths, gh: int, gw: int, ph: int, pw: int):
    """NumPy float64: (centres [B, L, 2], boxes [B, L, 4], peak [B, L] int, peak_mass [B, L]) of maps [B, L, gh * gw]; row i of image b is
    valid iff i <= lengths[b]; invalid rows give zeros and peak -1."""
    a = np.asarray(maps, dtype=np.float64)
    B, L, S = a.shape
    assert S == gh * gw
    t = np.arange(S)
    x = (t % gw + 0.5) * pw
    y = (t // gw + 0.5) * ph
    cx, cy = (a * x).sum(-1), (a * y).sum(-1)
    vx = (a * (x[None, None] - cx[..., None]) ** 2).sum(-1) + pw * pw / 12.0               # second pass, never E[x^2] - cx^2
    vy = (a * (y[None, None] - cy[..., None]) ** 2).sum(-1) + ph * ph / 12.0
    hx, hy = np.sqrt(3.0 * vx), np.sqrt(3.0 * vy)
    W, Hh = float(gw * pw), float(gh * ph)
    boxes = np.stack([np.clip(cx - hx, 0, W), np.clip(cy - hy, 0, Hh), np.clip(cx + hx, 0, W), np.clip(cy + hy, 0, Hh)], -1)
    centres = np.stack([cx, cy], -1)
    peak = a.argmax(-1)                                                                      # first maximum
    mass = np.take_along_axis(a, peak[..., None], -1)[..., 0]
    valid = np.arange(L)[None, :] <= np.asarray(lengths).reshape(B, 1)
    centres = np.where(valid[..., None], centres, 0.0)
    boxes = np.where(valid[..., None], boxes, 0.0)
    return centres, boxes, np.where(valid, peak, -1).astype(np.int64), np.where(valid, mass, 0.0)
