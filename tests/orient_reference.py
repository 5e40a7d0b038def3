"""The choice among K turned views of a crop restated in numpy.

Rows b K .. b K + K - 1 are the views of crop b.  From what post-processing gives every row — fp32 probabilities of the greedy reading per
position, the index of the first <eos> (L: none) — the key of a view is, in float64 and with n = min(length + 1, L),
    s = sum_{i < n} log(float64(p_i)), added in position order;   'sum': s;   'mean': s / n;   + float64(prior[k]) when there is a prior.
A NaN key counts as -inf (and is returned as -inf).  The winner is the first k of the largest key; view 0 when every key is -inf.
"""
import numpy as np


def keys(probs, lengths, views: int, criterion: str = 'mean', prior=None):
    """probs fp32 [B * K, L], lengths int [B * K] -> float64 [B, K]."""
    probs = np.asarray(probs, dtype=np.float32)
    lengths = np.asarray(lengths).astype(np.int64)
    rows, L = probs.shape
    assert rows % views == 0 and criterion in ('mean', 'sum')
    out = np.empty(rows, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        for r in range(rows):
            n = min(int(lengths[r]) + 1, L)
            s = np.float64(0.0)
            for i in range(n):
                s = s + np.log(np.float64(probs[r, i]))
            if criterion == 'mean':
                s = s / np.float64(n)
            if prior is not None:
                s = s + np.float64(np.float32(prior[r % views]))
            out[r] = -np.inf if np.isnan(s) else s
    return out.reshape(rows // views, views)


def winners(k):
    """float64 [B, K] keys -> int [B]: the first index of the largest key, 0 when all are -inf."""
    view = np.zeros(k.shape[0], dtype=np.int64)
    for b in range(k.shape[0]):
        best = -np.inf
        for j in range(k.shape[1]):
            if k[b, j] > best:
                best, view[b] = k[b, j], j
    return view


def select(probs, lengths, views: int, criterion: str = 'mean', prior=None):
    """(keys float64 [B, K], view int [B])."""
    k = keys(probs, lengths, views, criterion, prior)
    return k, winners(k)


def top_two_gap(k):
    """float64 [B]: the largest key minus the second largest of every crop (inf for a single view; nan where both are -inf)."""
    if k.shape[1] == 1:
        return np.full(k.shape[0], np.inf)
    s = np.sort(k, axis=1)
    with np.errstate(invalid='ignore'):
        return s[:, -1] - s[:, -2]
