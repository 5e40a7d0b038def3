"""Cloze refinement of beam hypotheses as DESIGN.md section 20 defines it, restated on the CPU.   *** TEST INFRASTRUCTURE ***

float64 log-soft-max and sums, plain Python for the cut, the duplicate rule and the ranking.  Logits need not be finite: the arg-max
follows argmax_take's rule (`first_argmax_rows`), and a row whose new score is not a number (one of its summed positions holds a NaN, a
+inf or nothing but -inf) comes out dead, like one whose score is -inf.  A hypothesis is its L tokens t[0 .. L) (class
ids, pad_id after its <eos>), a score (-inf: dead), a length, a finished flag, a trie node, a word id and the score the search gave it.

  refine_image   one iteration on the W rows of one image (what `parseq_op_beam_refine` does per workgroup)
  refine_rows    the same over B images
  refine_search  `iters` iterations over any `logits_of(it, tgt_in) -> [rows, L, C]` callable
  tgt_in_of      the decoder input of a set of rows: [<bos>, t[0 .. L - 2]]
  oracle_refine_logits   `logits_of` over the CPU oracle (memory once; decode + head under the cloze and key padding masks)

Beside the result every iteration reports its margins: the float64 score gaps between adjacent ranks of live rows and between a removed
duplicate and the row that survived it.  A decision whose margin is below the arithmetic's error bound is not safe against another
arithmetic; an exact 0 is a tie the index rule decides.
"""
from __future__ import annotations

from dataclasses import dataclass, field
from typing import Callable, List

import torch

NEG_INF = float('-inf')
MODES = ('score', 'edit')


@dataclass
class Rows:
    tokens: List[List[int]]
    scores: List[float]
    finished: List[int]
    lengths: List[int]
    nodes: List[int]
    words: List[int]
    ar_scores: List[float]
    src: List[int] = field(default_factory=list)          # per output row: the input row it was
    last: List[int] = field(default_factory=list)         # per output row: the last summed position (-1: dead)
    gaps: List[float] = field(default_factory=list)       # the iteration's margins (see the module text)


def first_argmax(row: torch.Tensor) -> int:
    """The lowest class id among the maxima (argmax_take's rule on finite logits)."""
    return int((row == row.max()).nonzero()[0])


def first_argmax_rows(logits: torch.Tensor) -> torch.Tensor:
    """argmax_take's rule on any input, over the last dimension: the first NaN where there is one, else the lowest class id among the
    maxima (so 0 for a row of -inf)."""
    C = logits.shape[-1]
    idx = torch.arange(C)
    nan = torch.isnan(logits)
    clean = torch.where(nan, torch.full_like(logits, NEG_INF), logits)
    first_max = torch.where(clean == clean.amax(-1, keepdim=True), idx, C).amin(-1)
    return torch.where(nan.any(-1), torch.where(nan, idx, C).amin(-1), first_max)


def refine_image(logits, mode: str, rows: Rows, eos_id: int, pad_id: int) -> Rows:
    """One iteration on one image.  logits [W, L, C] (any float dtype; the values are taken as they are)."""
    assert mode in MODES
    logits = torch.as_tensor(logits)
    W, L, _ = logits.shape
    logp = torch.log_softmax(logits.double(), -1)
    picks_all = first_argmax_rows(logits).tolist()
    new = []      # per input row: (score, tokens, finished, length, last)
    for w in range(W):
        if rows.scores[w] == NEG_INF:
            new.append((NEG_INF, None, 0, 0, -1))
            continue
        if mode == 'score':
            t, fin, length = list(rows.tokens[w]), rows.finished[w], rows.lengths[w]
            last = length if fin else L - 1
        else:
            picks = picks_all[w]
            length = picks.index(eos_id) if eos_id in picks else L
            fin = 1 if length < L else 0
            last = length if fin else L - 1
            t = [picks[i] if i <= last else pad_id for i in range(L)]
        s = 0.0
        for i in range(last + 1):
            s += float(logp[w, i, t[i]])
        if s != s:      # a NaN, +inf or all -inf logit row among the summed positions: no score, so no hypothesis
            s = NEG_INF
        new.append((s, t, fin, length, last))
    gaps = []
    dead = [n[0] == NEG_INF for n in new]
    if mode == 'edit':
        for w in range(W):
            for v in range(W):
                if v == w or dead[w] or new[v][0] == NEG_INF or new[w][0] == NEG_INF:
                    continue
                if new[v][1:4] == new[w][1:4] and (new[v][0] > new[w][0] or (new[v][0] == new[w][0] and v < w)):
                    dead[w] = True
        for w in range(W):      # the margin of every removal: against the best of its group
            if dead[w] and new[w][0] != NEG_INF:
                best = max(new[v][0] for v in range(W) if new[v][0] != NEG_INF and new[v][1:4] == new[w][1:4])
                gaps.append(best - new[w][0])
    order = sorted(range(W), key=lambda w: (dead[w], 0.0 if dead[w] else -new[w][0], w))
    live = [w for w in order if not dead[w]]
    gaps += [new[a][0] - new[b][0] for a, b in zip(live, live[1:])]
    out = Rows([], [], [], [], [], [], [], gaps=gaps)
    for w in order:
        out.src.append(w)
        out.nodes.append(rows.nodes[w])
        out.ar_scores.append(rows.ar_scores[w])
        if dead[w]:
            out.tokens.append([pad_id] * L); out.scores.append(NEG_INF); out.finished.append(0); out.lengths.append(0)
            out.words.append(-1); out.last.append(-1)
        else:
            s, t, fin, length, last = new[w]
            out.tokens.append(t); out.scores.append(s); out.finished.append(fin); out.lengths.append(length)
            out.words.append(rows.words[w]); out.last.append(last)
    return out


def slice_rows(rows: Rows, lo: int, hi: int) -> Rows:
    return Rows(rows.tokens[lo:hi], rows.scores[lo:hi], rows.finished[lo:hi], rows.lengths[lo:hi], rows.nodes[lo:hi], rows.words[lo:hi],
                rows.ar_scores[lo:hi])


def refine_rows(logits, mode: str, rows: Rows, B: int, W: int, eos_id: int, pad_id: int) -> List[Rows]:
    """One iteration over B images: logits [B * W, L, C], the rows of image b at b * W .. b * W + W - 1.  One `Rows` per image."""
    logits = torch.as_tensor(logits)
    return [refine_image(logits[b * W:(b + 1) * W], mode, slice_rows(rows, b * W, (b + 1) * W), eos_id, pad_id) for b in range(B)]


def concat_rows(per_image: List[Rows]) -> Rows:
    out = Rows([], [], [], [], [], [], [])
    for r in per_image:
        for name in ('tokens', 'scores', 'finished', 'lengths', 'nodes', 'words', 'ar_scores', 'last'):
            getattr(out, name).extend(getattr(r, name))
        out.src.append(r.src)
        out.gaps.append(r.gaps)
    return out


def tgt_in_of(tokens, bos_id: int) -> torch.Tensor:
    """int64 [rows, L]: <bos>, then the tokens but the last."""
    t = torch.as_tensor(tokens, dtype=torch.int64)
    return torch.cat([torch.full((t.shape[0], 1), bos_id, dtype=torch.int64), t[:, :-1]], 1)


def refine_search(logits_of: Callable[[int, torch.Tensor], torch.Tensor], mode: str, iters: int, rows: Rows, B: int, W: int, bos_id: int,
                  eos_id: int, pad_id: int) -> List[Rows]:
    """`iters` iterations from the state a search left (`rows.ar_scores` = its scores); the state after every iteration, rows concatenated
    over the images, `src` and `gaps` per image.  A dead row's tokens are pad_id, so its tgt_in is [<bos>, pad_id ...]."""
    states = []
    for it in range(iters):
        logits = logits_of(it, tgt_in_of(rows.tokens, bos_id))
        rows = concat_rows(refine_rows(logits, mode, rows, B, W, eos_id, pad_id))
        states.append(rows)
    return states


def rows_of_search(tokens, scores, finished, lengths, words=None, pad_id=None) -> Rows:
    """The state a search left, from its outputs [B, W, ...] (tensors): a dead hypothesis' tokens are pad_id there already."""
    tok = torch.as_tensor(tokens).long().flatten(0, 1).tolist()
    sc = [float(s) for s in torch.as_tensor(scores).double().flatten()]
    n = len(sc)
    wd = [-1] * n if words is None else torch.as_tensor(words).long().flatten().tolist()
    return Rows(tok, sc, torch.as_tensor(finished).long().flatten().tolist(), torch.as_tensor(lengths).long().flatten().tolist(), [-1] * n, wd, list(sc))


def oracle_refine_logits(sd, cfg, images, W: int, num_steps: int, rounding=None):
    """`f(tgt_in) -> [rows, num_steps, C]` over the CPU oracle: the refinement pass of oracle.forward (parseq_oracle.py:304-318) on explicit
    decoder inputs, row r against the memory of image r // W."""
    from oracle import parseq_oracle as O
    with torch.inference_mode():
        memory = O.encode(sd, cfg, images, rounding).repeat_interleave(W, 0)
    L = num_steps
    query_mask = torch.triu(torch.ones((L, L), dtype=torch.bool), 1)
    query_mask[torch.triu(torch.ones(L, L, dtype=torch.bool), 2)] = False

    def f(tgt_in):
        with torch.inference_mode():
            pad = (tgt_in == cfg.eos_id).int().cumsum(-1) > 0
            q = sd['pos_queries'][:, :L].expand(tgt_in.shape[0], -1, -1)
            out = O.decode(sd, cfg, tgt_in, memory, None, pad, q, query_mask, rounding=rounding)
            return O.head(sd, out, rounding).clone()
    return f
