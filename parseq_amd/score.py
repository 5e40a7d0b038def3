"""Scoring given readings: the host side — the decoding orders, the candidates as token rows, the result — and the
two kernels after the decoder pass on a caller's tensors.  `system.PARSeq.score` is the way in; the device work is `parseq_score`."""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

MAX_CANDIDATES, MAX_ORDERS = 16, 16      # PARSEQ_SCORE_MAX_CANDIDATES, PARSEQ_SCORE_MAX_ORDERS
COMBINE = {'mix': 0, 'mean': 1}          # PARSEQ_SCORE_MIX, PARSEQ_SCORE_MEAN
LENGTH_NORM = 2                          # PARSEQ_SCORE_LENGTH_NORM


@dataclass
class ScoreResult:
    """What `PARSeq.score` returns, on the device but for `perms`; N candidates per crop in the caller's order, K decoding orders."""
    scores: Tensor             # fp32 [B, N] the combined log-probability (-inf: absent or invalid)
    order_scores: Tensor       # fp32 [B, N, K] the joint log-probability under every order, <eos> included
    char_logprobs: Tensor      # fp32 [B, N, K, L] its terms: position i <= length is character i (i = length: <eos>), 0 past it
    rank: Tensor               # int32 [B, N] the candidates of a crop best first
    lengths: Tensor            # int32 [B, N] characters of the candidate
    valid: Tensor              # uint8 [B, N] 0: absent or invalid
    perms: Tensor              # int64 [K, T + 2] on the host: the orders that were used

    def best(self) -> Tuple[Tensor, Tensor]:
        """(index [B] of every crop's best candidate, its score [B]), on the device."""
        idx = self.rank[:, 0].long()
        return idx, self.scores.gather(1, idx[:, None])[:, 0]


def score_flags(combine: str, normalize: bool) -> int:
    if combine not in COMBINE:
        raise ValueError(f"score: combine must be 'mix' or 'mean', got {combine!r}")
    return COMBINE[combine] | (LENGTH_NORM if normalize else 0)


def forward_perm(T: int) -> Tensor:
    return torch.arange(T + 2)


def mirrored_perm(T: int) -> Tensor:
    """Row 1 of the reference's gen_tgt_perms: <bos>, then <eos>, then the characters right to left."""
    return torch.cat([torch.zeros(1, dtype=torch.long), torch.arange(T + 1, 0, -1)])


def parse_orders(orders, T: int, system=None, seed: Optional[int] = None) -> Tensor:
    """`orders` of `PARSeq.score` -> position orderings int64 [K, T + 2] as `gen_tgt_perms` lays them out (column 0 is <bos>).
    'forward', 'mirrored', 'both'; an int K: the first K rows `gen_tgt_perms` gives a label of T characters with the system's settings,
    numpy's draws from `np.random.default_rng(seed)` and torch's under `seed` too when it is given; or a [K, T + 2] tensor of permutations."""
    if T < 1:
        raise ValueError(f'score: T = {T}, at least 1')
    if isinstance(orders, str):
        named = {'forward': [forward_perm(T)], 'mirrored': [mirrored_perm(T)], 'both': [forward_perm(T), mirrored_perm(T)]}
        if orders not in named:
            raise ValueError(f"score: orders must be 'forward', 'mirrored', 'both', an int or a tensor, got {orders!r}")
        return torch.stack(named[orders])
    if isinstance(orders, bool):
        raise ValueError('score: orders must not be a bool')
    if isinstance(orders, (int, np.integer)):
        K = int(orders)
        if K < 1 or K > MAX_ORDERS:
            raise ValueError(f'score: {K} orders, it must be in 1 .. {MAX_ORDERS}')
        if system is None:
            raise ValueError('score: an int for orders needs the system whose gen_tgt_perms settings apply')
        from .system import gen_tgt_perms
        rng = np.random.default_rng(seed)
        dummy = torch.zeros(1, T + 2, dtype=torch.long)
        with torch.random.fork_rng(devices=[]):
            if seed is not None:
                torch.manual_seed(int(seed))
            perms = gen_tgt_perms(dummy, system.max_gen_perms, system.perm_forward, system.perm_mirrored, rng)
        if len(perms) < K:
            raise ValueError(f'score: {K} orders asked, gen_tgt_perms gives {len(perms)} for {T} characters')
        return perms[:K].clone()
    perms = torch.as_tensor(orders).detach().cpu().long()
    if perms.ndim != 2 or perms.shape[1] != T + 2:
        raise ValueError(f'score: an orders tensor must be [K, {T + 2}] for candidates of at most {T} characters, got {tuple(perms.shape)}')
    if not 1 <= perms.shape[0] <= MAX_ORDERS:
        raise ValueError(f'score: {perms.shape[0]} orders, it must be in 1 .. {MAX_ORDERS}')
    want = torch.arange(T + 2)
    for row in perms:
        if int(row[0]) != 0 or not torch.equal(row.sort().values, want):
            raise ValueError(f'score: every order must be a permutation of 0 .. {T + 1} that starts with 0 (<bos>), got {row.tolist()}')
    return perms


def query_masks(perms: Tensor) -> Tensor:
    """uint8 [K, L, L], L = T + 1: the query mask of every order (`generate_attn_masks(perm)[1]`), 1 = masked."""
    from .system import generate_attn_masks
    return torch.stack([generate_attn_masks(p)[1] for p in perms.cpu()]).to(torch.uint8)


def encode_candidates(tokenizer, candidates: Sequence[Sequence[str]], max_label_length: int) -> Tuple[np.ndarray, int]:
    """Candidate strings -> (int32 [B, N, L] rows `c_0 .. c_{n-1}, <eos>, <pad> ..`, T).  N is the longest list (shorter ones are filled with
    absent rows, all <pad>), T = max(longest string, 1), L = T + 1.  ValueError: no crop, no candidate, more than MAX_CANDIDATES of them,
    a string longer than `max_label_length`, a character outside the tokenizer's charset."""
    if len(candidates) == 0:
        raise ValueError('score: no crops')
    lists = [[c] if isinstance(c, str) else list(c) for c in candidates]
    N = max(len(c) for c in lists)
    if N < 1 or N > MAX_CANDIDATES:
        raise ValueError(f'score: {N} candidates for a crop, it must be in 1 .. {MAX_CANDIDATES}')
    stoi = tokenizer._stoi
    specials = (tokenizer.BOS, tokenizer.EOS, tokenizer.PAD)
    T = 1
    for cs in lists:
        for s in cs:
            if not isinstance(s, str):
                raise ValueError(f'score: a candidate must be a string, got {s!r}')
            foreign = sorted({ch for ch in s if ch not in stoi or ch in specials})
            if foreign:
                raise ValueError(f'score: candidate {s!r} has characters outside the training charset: {foreign}')
            T = max(T, len(s))
    if T > max_label_length:
        raise ValueError(f'score: a candidate of {T} characters, max_label_length is {max_label_length}')
    out = np.full((len(lists), N, T + 1), tokenizer.pad_id, dtype=np.int32)
    for b, cs in enumerate(lists):
        for j, s in enumerate(cs):
            out[b, j, :len(s)] = [stoi[ch] for ch in s]
            out[b, j, len(s)] = tokenizer.eos_id
    return out, T


def score_rows(logits: Tensor, targets: Tensor, lengths: Tensor, valid: Tensor, orders: int, order: int, order_scores: Tensor,
               char_logprobs: Optional[Tensor] = None) -> None:
    """`parseq_op_score_rows` on device tensors: logits fp32 [rows, L, C], targets int32 [rows, L], lengths int32 [rows], valid uint8 [rows];
    fills order `order` of order_scores fp32 [rows, orders] and of char_logprobs fp32 [rows, orders, L]."""
    from . import _native
    rows, L, C_ = logits.shape
    for t, dt in ((logits, torch.float32), (targets, torch.int32), (lengths, torch.int32), (valid, torch.uint8), (order_scores, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError('score_rows: contiguous device tensors of the documented types')
    if targets.numel() != rows * L or lengths.numel() != rows or valid.numel() != rows or order_scores.numel() != rows * orders:
        raise ValueError('score_rows: shapes disagree')
    if char_logprobs is not None and (char_logprobs.dtype != torch.float32 or not char_logprobs.is_contiguous() or char_logprobs.numel() != rows * orders * L):
        raise ValueError('score_rows: char_logprobs must be contiguous fp32 [rows, orders, L]')
    with _native.guard(logits):
        _native.check(_native.lib().parseq_op_score_rows(_native.ptr(logits), rows, L, C_, _native.ptr(targets), _native.ptr(lengths), _native.ptr(valid),
                                                         orders, order, _native.ptr(order_scores), _native.ptr(char_logprobs), _native.stream_ptr(logits)))


def score_rank(order_scores: Tensor, lengths: Tensor, valid: Tensor, combine: str = 'mix', normalize: bool = False) -> Tuple[Tensor, Tensor]:
    """`parseq_op_score_rank` on device tensors: order_scores fp32 [B, N, K], lengths int32 [B, N], valid uint8 [B, N] -> (scores fp32 [B, N],
    rank int32 [B, N])."""
    from . import _native
    flags = score_flags(combine, normalize)
    B, N, K = order_scores.shape
    for t, dt in ((order_scores, torch.float32), (lengths, torch.int32), (valid, torch.uint8)):
        if t.dtype != dt or not t.is_contiguous() or not t.is_cuda:
            raise ValueError('score_rank: contiguous device tensors of the documented types')
    if tuple(lengths.shape) != (B, N) or tuple(valid.shape) != (B, N):
        raise ValueError('score_rank: lengths and valid must be [B, N]')
    scores = torch.empty(B, N, dtype=torch.float32, device=order_scores.device)
    rank = torch.empty(B, N, dtype=torch.int32, device=order_scores.device)
    with _native.guard(order_scores):
        _native.check(_native.lib().parseq_op_score_rank(_native.ptr(order_scores), _native.ptr(lengths), _native.ptr(valid), B, N, K, flags,
                                                         _native.ptr(scores), _native.ptr(rank), _native.stream_ptr(order_scores)))
    return scores, rank


def decode_scores(result: ScoreResult, candidates: Sequence[Sequence[str]]) -> List[List[Tuple[str, float, List[List[float]]]]]:
    """Per crop the candidates best first: (string, score, per-character log-probabilities [K][n + 1], the last of each the <eos>'s).
    Absent and invalid rows are left out.  One copy to the host."""
    B, N, K, L = result.char_logprobs.shape
    packed = torch.cat([result.scores.reshape(B * N, 1), result.char_logprobs.reshape(B * N, K * L),
                        result.rank.reshape(B * N, 1).float(), result.lengths.reshape(B * N, 1).float(), result.valid.reshape(B * N, 1).float()], dim=1).cpu()
    scores = packed[:, 0].reshape(B, N).tolist()
    lps = packed[:, 1:1 + K * L].reshape(B, N, K, L)
    rank = packed[:, 1 + K * L].reshape(B, N).long().tolist()
    lengths = packed[:, 2 + K * L].reshape(B, N).long().tolist()
    valid = packed[:, 3 + K * L].reshape(B, N).long().tolist()
    out = []
    for b in range(B):
        cs = [candidates[b]] if isinstance(candidates[b], str) else list(candidates[b])
        out.append([(cs[j], scores[b][j], lps[b, j, :, :lengths[b][j] + 1].tolist()) for j in rank[b] if valid[b][j] and j < len(cs)])
    return out
