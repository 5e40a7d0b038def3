"""Beam search over a weighted automaton as DESIGN.md section 24 defines it, restated on the CPU.   *** TEST INFRASTRUCTURE ***

tests/lexicon_reference.py with a weight on every arc: float64 log-soft-max over ALL classes, float64 sums, plain Python sorting.  A live
unfinished beam w at state n offers (w, c) where the table allows it (lexicon_reference.allowed) and weight[n][c] is finite, at the model
score m = score[w] + logp[w][c] and the fused value f = m + (alpha (wsum[w] + weight[n][c]) + beta k), k = step + 1 for a character and
step for <eos>; a finished beam carries at score + (alpha wsum + beta length).  The ranking is by f, then the lower parent, then the lower
class.  A beam keeps score (the model's sum) and wsum apart; f is recomputed from them, never accumulated.  A candidate or carry one of
whose four operations leaves the range of fp32 (a finite alpha can overflow a product) is not allowed.

  step_image    one selection step of one image on explicit state (what `parseq_op_beam_step_automaton` does per workgroup)
  beam_search   the whole search over any `step_logits(histories) -> [rows, C]` callable
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

import lexicon_reference as LR

NEG_INF = LR.NEG_INF
FLT_MAX = 3.4028234663852886e38      # the largest finite fp32


def fused(m: float, wsum: float, k: int, alpha: float, beta: float) -> float:
    """m + (alpha wsum + beta k); -inf ("no candidate") if a product or a sum is outside fp32's range."""
    p, q = alpha * wsum, beta * k
    f = m + (p + q)
    return f if all(abs(v) <= FLT_MAX for v in (p, q, p + q, f)) else NEG_INF


def allowed(next_table, weight, node: int, c: int, eos_id: int) -> bool:
    return LR.allowed(next_table, node, c, eos_id) and math.isfinite(weight[node][c])


def rank_candidates(logits, scores, wsums, finished, lengths, nodes, next_table, weight, step: int, eos_id: int, alpha: float, beta: float):
    """Every candidate (f, parent, class, model score, weight sum) of one image, best first."""
    logp = torch.log_softmax(torch.as_tensor(logits).double(), -1)
    cands = []
    for w, s in enumerate(scores):
        if s == NEG_INF:
            continue
        if finished[w]:
            f = fused(float(s), float(wsums[w]), lengths[w], alpha, beta)
            if f > NEG_INF:
                cands.append((f, w, -1, float(s), float(wsums[w])))
            continue
        for c, lp in enumerate(logp[w].tolist()):
            if allowed(next_table, weight, nodes[w], c, eos_id):
                m, ws = float(s) + lp, float(wsums[w]) + float(weight[nodes[w]][c])
                f = fused(m, ws, step if c == eos_id else step + 1, alpha, beta)
                if f > NEG_INF:
                    cands.append((f, w, c, m, ws))
    cands.sort(key=lambda t: (-t[0], t[1], t[2]))
    return cands


@dataclass
class StepResult(LR.StepResult):
    wsums: List[float] = field(default_factory=list)
    fused: List[float] = field(default_factory=list)


def step_image(logits, scores, wsums, finished, lengths, hist, nodes, words, next_table, weight, step: int, eos_id: int, pad_id: int,
               alpha: float, beta: float) -> StepResult:
    """`scores` in and out are the model's sums; `fused` out the values the ranking used; `gap` the smallest gap in f among the best W + 1."""
    W = len(scores)
    cands = rank_candidates(logits, scores, wsums, finished, lengths, nodes, next_table, weight, step, eos_id, alpha, beta)
    top = cands[:W + 1]
    gap = min((top[k][0] - top[k + 1][0] for k in range(len(top) - 1)), default=math.inf)
    out = StepResult([], [], [], [], [], [], gap)
    for r in range(W):
        if r < len(cands):
            f, par, cls, s, ws = cands[r]
            row = list(hist[par])
            fin = 1 if (cls < 0 or cls == eos_id) else 0
            length = lengths[par] if cls < 0 else (step if cls == eos_id else step + 1)
            if cls < 0:
                node, word = nodes[par], words[par]
            elif cls == eos_id:
                node, word = nodes[par], int(next_table[nodes[par]][eos_id])
            else:
                node, word = int(next_table[nodes[par]][cls]), -1
        else:
            f, s, ws, par, cls, row, fin, length, node, word = NEG_INF, NEG_INF, 0.0, -1, -1, list(hist[r]), 0, 0, -1, -1
        pick = cls if cls >= 0 else pad_id
        if step + 1 < len(row):
            row[step + 1] = pick
        out.scores.append(s); out.finished.append(fin); out.lengths.append(length); out.hist.append(row)
        out.parent.append(par); out.picked.append(pick); out.nodes.append(node); out.words.append(word)
        out.wsums.append(ws); out.fused.append(f)
    return out


@dataclass
class BeamSearchResult(LR.BeamSearchResult):
    """`scores` and `step_scores` are the fused values (what the device reports and traces)."""
    model_scores: Optional[torch.Tensor] = None   # float64 [B, W]
    priors: Optional[torch.Tensor] = None         # float64 [B, W]


def beam_search(step_logits: Callable[[torch.Tensor], torch.Tensor], B: int, W: int, num_steps: int, bos_id: int, eos_id: int, pad_id: int,
                next_table, weight, alpha: float, beta: float, roots=None) -> BeamSearchResult:
    next_table = torch.as_tensor(next_table).tolist()
    weight = torch.as_tensor(weight).double().tolist()
    roots = [0] * B if roots is None else [int(r) for r in roots]
    hist = [[[bos_id] + [pad_id] * num_steps for _ in range(W)] for _ in range(B)]
    scores = [[0.0] + [NEG_INF] * (W - 1) for _ in range(B)]
    nodes = [[roots[b]] + [-1] * (W - 1) for b in range(B)]
    for b in range(B):
        if not 0 <= roots[b] < len(next_table):
            scores[b][0], nodes[b][0] = NEG_INF, -1
    wsums = [[0.0] * W for _ in range(B)]
    fvals = [[NEG_INF] * W for _ in range(B)]
    words = [[-1] * W for _ in range(B)]
    finished = [[0] * W for _ in range(B)]
    lengths = [[0] * W for _ in range(B)]
    res = BeamSearchResult(None, None, None, None, torch.empty(B, num_steps, dtype=torch.float64))
    for i in range(num_steps):
        flat = torch.tensor([row for img in hist for row in img], dtype=torch.int64)
        res.tokens_in.append(flat[:, :num_steps].clone())
        logits = torch.as_tensor(step_logits(flat[:, :i + 1])).reshape(B, W, -1)
        parents = []
        for b in range(B):
            st = step_image(logits[b], scores[b], wsums[b], finished[b], lengths[b], hist[b], nodes[b], words[b], next_table, weight, i, eos_id,
                            pad_id, alpha, beta)
            scores[b], wsums[b], fvals[b], finished[b], lengths[b] = st.scores, st.wsums, st.fused, st.finished, st.lengths
            hist[b], nodes[b], words[b] = st.hist, st.nodes, st.words
            parents.append(st.parent)
            res.gaps[b, i] = st.gap
        res.parents.append(torch.tensor(parents, dtype=torch.int64))
        res.step_scores.append(torch.tensor(fvals, dtype=torch.float64))
    res.scores = torch.tensor(fvals, dtype=torch.float64)
    res.model_scores = torch.tensor(scores, dtype=torch.float64)
    res.priors = torch.tensor(wsums, dtype=torch.float64)
    res.finished = torch.tensor(finished, dtype=torch.int64)
    res.lengths = torch.tensor(lengths, dtype=torch.int64)
    res.words = torch.tensor(words, dtype=torch.int64)
    res.nodes = torch.tensor(nodes, dtype=torch.int64)
    tokens = torch.tensor(hist, dtype=torch.int64)[:, :, 1:]
    tokens[res.model_scores == NEG_INF] = pad_id
    res.tokens = tokens
    return res
