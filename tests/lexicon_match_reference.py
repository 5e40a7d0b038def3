"""Lexicon matching as DESIGN.md section 23 defines it, restated on the CPU.   *** TEST INFRASTRUCTURE ***

A plain Levenshtein DP (unit costs), one row of the table per character of the reading, vectorised over the words with numpy; then the
selection: the n nearest words by (distance, word id), dead slots beyond the list, and the reading as one more candidate.

  distances      reading x every word of a list -> int array
  nearest        the n best (word id, distance) of one reading
  match          the same for B readings, with per-reading row ranges and a class folding map
  candidates     the W = n (+ 1) hypotheses of one crop in (distance, id) order, the reading included under `keep_reading`
"""
from __future__ import annotations

from typing import List, Optional, Sequence, Tuple

import numpy as np

DEAD = 0x7FFFFFFF      # PARSEQ_LEXICON_MATCH_DEAD


def pack(words: Sequence[Sequence[int]]) -> Tuple[np.ndarray, np.ndarray]:
    """(ids int64 [n, longest] padded with -2, lengths int64 [n]) of words given as lists of class ids."""
    longest = max((len(w) for w in words), default=0)
    ids = np.full((len(words), max(longest, 1)), -2, dtype=np.int64)
    for r, w in enumerate(words):
        ids[r, :len(w)] = w
    return ids, np.array([len(w) for w in words], dtype=np.int64)


def distances(reading: Sequence[int], ids: np.ndarray, lengths: np.ndarray) -> np.ndarray:
    """Levenshtein distance of `reading` to every word: D[i][j] over the reading's first i and the word's first j characters,
    D[i][j] = min(D[i-1][j] + 1, D[i][j-1] + 1, D[i-1][j-1] + (reading[i-1] != word[j-1])); the answer is D[len(reading)][len(word)]."""
    n, width = ids.shape
    prev = np.tile(np.arange(width + 1, dtype=np.int64), (n, 1))      # D[0][j] = j
    for i, ch in enumerate(reading, 1):
        cur = np.empty_like(prev)
        cur[:, 0] = i
        sub = prev[:, :-1] + (ids != ch)
        dele = prev[:, 1:] + 1
        best = np.minimum(sub, dele)
        for j in range(1, width + 1):      # the insertion runs along the row
            cur[:, j] = np.minimum(best[:, j - 1], cur[:, j - 1] + 1)
        prev = cur
    return prev[np.arange(n), lengths]


def cut(reading: Sequence[int], eos_id: int, length: Optional[int] = None) -> List[int]:
    """The reading proper: its first `length` ids, up to the first <eos>."""
    r = list(reading)[:length]
    return r[:r.index(eos_id)] if eos_id in r else r


def nearest(reading: Sequence[int], ids: np.ndarray, lengths: np.ndarray, word_ids: Sequence[int], n: int) -> Tuple[List[int], List[int]]:
    """(word ids, distances) of the n nearest rows by (distance, word id); -1 / DEAD beyond the list."""
    if len(word_ids) == 0:
        return [-1] * n, [DEAD] * n
    d = distances(reading, ids, lengths)
    order = sorted(range(len(word_ids)), key=lambda r: (int(d[r]), word_ids[r]))[:n]
    pad = n - len(order)
    return [word_ids[r] for r in order] + [-1] * pad, [int(d[r]) for r in order] + [DEAD] * pad


def match(readings, reading_lengths, words: Sequence[Sequence[int]], word_ids: Sequence[int], n: int, eos_id: int, ranges=None, fold=None):
    """B readings (rows of class ids; `reading_lengths` may be None) against the rows `words` (lists of class ids, already folded when `fold`
    is given) — row r has word id word_ids[r], ascending.  `ranges[b]` = (begin, end) restricts reading b to those rows; `fold` maps the
    reading's classes.  Returns (ids [B][n], distances [B][n])."""
    out_ids, out_d = [], []
    for b, reading in enumerate(readings):
        r = cut(reading, eos_id, None if reading_lengths is None else int(reading_lengths[b]))
        if fold is not None:
            r = [int(fold[c]) if 0 <= c < len(fold) else c for c in r]
        lo, hi = (0, len(words)) if ranges is None else (max(int(ranges[b][0]), 0), min(int(ranges[b][1]), len(words)))
        sub = list(words[lo:hi]) if lo < hi else []
        ids, lengths = pack(sub)
        i, d = nearest(r, ids, lengths, list(word_ids[lo:hi]) if lo < hi else [], n)
        out_ids.append(i)
        out_d.append(d)
    return out_ids, out_d


def candidates(ids: Sequence[int], dist: Sequence[int], keep_reading: bool) -> List[Tuple[int, int, bool]]:
    """The hypotheses of one crop in (distance, id) order as (word id, distance, is the reading): with `keep_reading` the reading comes
    first at distance 0 unless a word has distance 0, in which case the extra slot is dead (-1, DEAD, False) and last."""
    out = [(i, d, False) for i, d in zip(ids, dist)]
    if not keep_reading:
        return out
    if dist[0] != 0:
        return [(-1, 0, True)] + out
    return out + [(-1, DEAD, False)]
