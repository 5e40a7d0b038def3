"""CPU restatement of scoring given readings on the oracle's encode / decode / head and a float64 log-soft-max.
Candidates are lists of class ids (no <eos>); None is an absent candidate."""
import math

import numpy as np
import torch

from oracle import parseq_oracle as O

NEG_INF = float('-inf')


def is_valid(cand, C, eos_id):
    return cand is not None and all(0 <= t < C and t != eos_id for t in cand)


def candidate_rows(cands, L, eos_id, pad_id):
    """Per-crop lists of candidates -> int32 [B, N, L] rows `c .., <eos>, <pad> ..` (an absent one all <pad>), as parseq_score takes them.
    An invalid candidate (a token outside the classes, an inner <eos>) is written as it is."""
    B, N = len(cands), max(len(c) for c in cands)
    out = np.full((B, N, L), pad_id, dtype=np.int32)
    for b, cs in enumerate(cands):
        for j, c in enumerate(cs):
            if c is not None:
                out[b, j, :len(c)] = c
                out[b, j, len(c)] = eos_id
    return out


def layout(cands, L, C, bos_id, eos_id, pad_id):
    """(tgt_in int64 [B N, L], targets [B N, L] (-1: not summed), lengths [B N], valid [B N]): what the staging kernel must produce."""
    B, N = len(cands), max(len(c) for c in cands)
    tgt_in = torch.full((B * N, L), pad_id, dtype=torch.long)
    tgt_in[:, 0] = bos_id
    targets = torch.full((B * N, L), -1, dtype=torch.long)
    lengths = torch.zeros(B * N, dtype=torch.long)
    valid = torch.zeros(B * N, dtype=torch.bool)
    for b, cs in enumerate(cands):
        for j, c in enumerate(cs):
            if not is_valid(c, C, eos_id):
                continue
            r, n = b * N + j, len(c)
            tgt_in[r, 1:n + 1] = torch.tensor(c, dtype=torch.long)
            targets[r, :n] = torch.tensor(c, dtype=torch.long)
            targets[r, n] = eos_id
            lengths[r], valid[r] = n, True
    return tgt_in, targets, lengths, valid


def rows_reference(logits, targets, lengths, valid):
    """float64: char_lp [rows, L] (0 where not summed) and their sums in ascending position (-inf for rows that are not valid)."""
    lp = logits.double().log_softmax(-1)
    rows, L, C = logits.shape
    char_lp = torch.zeros(rows, L, dtype=torch.float64)
    sums = torch.full((rows,), NEG_INF, dtype=torch.float64)
    for r in range(rows):
        if not valid[r]:
            continue
        s = 0.0
        for i in range(int(lengths[r]) + 1):
            t = int(targets[r, i])
            v = float(lp[r, i, t]) if 0 <= t < C else NEG_INF
            char_lp[r, i] = v
            s += v
        sums[r] = NEG_INF if s != s else s
    return char_lp, sums


def combine(order_scores, mean=False):
    """float64 [.., K] -> the combined score, float32: the log of the mixture, or the mean of the logs; NaN counts as -inf."""
    s = np.asarray(order_scores, dtype=np.float64)
    s = np.where(np.isnan(s), NEG_INF, s)
    K = s.shape[-1]
    out = np.full(s.shape[:-1], NEG_INF, dtype=np.float64)
    for idx in np.ndindex(*s.shape[:-1]):
        row = s[idx]
        if mean:
            acc = 0.0
            for v in row:
                acc += v
            out[idx] = acc / K
        else:
            m = row.max()
            if m > NEG_INF:
                acc = 0.0
                for v in row:
                    acc += math.exp(v - m)
                out[idx] = m + math.log(acc) - math.log(K)
    out = out.astype(np.float32)
    return np.where(np.isnan(out), np.float32(NEG_INF), out)


def rank(scores, lengths, valid, normalize=False):
    """scores float32 [B, N] -> rank int [B, N]: best first, the higher key, then the lower index; rows that are not valid have key -inf."""
    scores = np.where(np.asarray(valid, dtype=bool), np.asarray(scores, dtype=np.float32), np.float32(NEG_INF))
    B, N = scores.shape
    out = np.zeros((B, N), dtype=np.int64)
    for b in range(B):
        keys = []
        for j in range(N):
            k = float(scores[b, j])
            if normalize and k > NEG_INF:
                k = k / (max(int(lengths[b][j]), 0) + 1)
            keys.append(k)
        out[b] = sorted(range(N), key=lambda j: (-keys[j], j))
    return out


def score(sd, cfg, images, cands, perms, mean=False, normalize=False, rounding=None):
    """The whole call on the oracle: dict of order_scores float64 [B, N, K], char_lp [B, N, K, L], scores float32 [B, N], rank, lengths, valid."""
    B, N = len(cands), max(len(c) for c in cands)
    cands = [list(c) + [None] * (N - len(c)) for c in cands]
    L = perms.shape[1] - 1
    C = cfg.num_tokens - 2
    tgt_in, targets, lengths, valid = layout(cands, L, C, cfg.bos_id, cfg.eos_id, cfg.pad_id)
    memory = O.encode(sd, cfg, images, rounding).repeat_interleave(N, dim=0)
    padding = (tgt_in == cfg.pad_id) | (tgt_in == cfg.eos_id)
    K = len(perms)
    order_scores = torch.empty(B * N, K, dtype=torch.float64)
    char_lp = torch.empty(B * N, K, L, dtype=torch.float64)
    for k, perm in enumerate(perms):
        qmask = O.attn_masks_from_perm(perm)[1]
        logits = O.head(sd, O.decode(sd, cfg, tgt_in, memory, None, padding, tgt_query_mask=qmask, rounding=rounding), rounding)
        char_lp[:, k], order_scores[:, k] = rows_reference(logits, targets, lengths, valid)
    order_scores = order_scores.view(B, N, K).numpy()
    lengths, valid = lengths.view(B, N).numpy(), valid.view(B, N).numpy()
    scores = combine(order_scores, mean)
    scores = np.where(valid, scores, np.float32(NEG_INF))
    return dict(order_scores=order_scores, char_lp=char_lp.view(B, N, K, L).numpy(), scores=scores, rank=rank(scores, lengths, valid, normalize),
                lengths=lengths, valid=valid)
