"""Beam search as DESIGN.md section 18 defines it, restated on the CPU.   *** TEST INFRASTRUCTURE ***

Written over any `step_logits(histories) -> [rows, C]` callable (`histories`: int64 [B * W, i + 1], <bos> first, row b * W + w), with
float64 log-soft-max and scores, plain Python sorting for the ranking.  Beside the result it reports, per image and step, the smallest
score gap between adjacent ranks among the best W + 1 candidates: the margin by which the step's decisions are safe against an
arithmetic that differs from this one.

  step_image    one selection step of one image on explicit state (what `parseq_op_beam_step` does per workgroup)
  beam_search   the whole search
  oracle_step_logits   the adapter over the CPU oracle (encode once, teacher-forced causal decode + head per step)
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List

import torch

NEG_INF = float('-inf')


@dataclass
class StepResult:
    scores: List[float]
    finished: List[int]
    lengths: List[int]
    hist: List[List[int]]
    parent: List[int]
    picked: List[int]
    gap: float


def rank_candidates(logits, scores, finished):
    """Every candidate (score, parent, class) of one image, best first: higher score, then lower parent, then lower class; a finished
    beam offers itself once as class -1, a dead beam (score -inf) nothing.  A candidate whose value is not finite is not a candidate: a -inf
    logit's class, and every class of a row that holds a NaN or a +inf or nothing but -inf (its log-sum is not a number)."""
    logp = torch.log_softmax(torch.as_tensor(logits).double(), -1)
    cands = []
    for w, s in enumerate(scores):
        if s == NEG_INF:
            continue
        if finished[w]:
            cands.append((float(s), w, -1))
        else:
            cands += [(float(s) + lp, w, c) for c, lp in enumerate(logp[w].tolist()) if math.isfinite(float(s) + lp)]
    cands.sort(key=lambda t: (-t[0], t[1], t[2]))
    return cands


def step_image(logits, scores, finished, lengths, hist, step: int, eos_id: int, pad_id: int) -> StepResult:
    """The W beams of one image after step `step`.  logits [W, C]; scores / finished / lengths: W values; hist: W rows (lists of equal
    length >= step + 1).  A slot without a candidate is dead: score -inf, parent -1, length 0, its own row's history kept.  Position
    step + 1 of a new history (if the rows have one) holds the picked class, pad_id for a carry or a dead slot."""
    W = len(scores)
    cands = rank_candidates(logits, scores, finished)
    top = cands[:W + 1]
    gap = min((top[k][0] - top[k + 1][0] for k in range(len(top) - 1)), default=math.inf)
    out = StepResult([], [], [], [], [], [], gap)
    for r in range(W):
        if r < len(cands):
            s, par, cls = cands[r]
            row = list(hist[par])
            fin = 1 if (cls < 0 or cls == eos_id) else 0
            length = lengths[par] if cls < 0 else (step if cls == eos_id else step + 1)
        else:
            s, par, cls, row, fin, length = NEG_INF, -1, -1, list(hist[r]), 0, 0
        pick = cls if cls >= 0 else pad_id
        if step + 1 < len(row):
            row[step + 1] = pick
        out.scores.append(s); out.finished.append(fin); out.lengths.append(length); out.hist.append(row)
        out.parent.append(par); out.picked.append(pick)
    return out


@dataclass
class BeamSearchResult:
    tokens: torch.Tensor          # int64 [B, W, num_steps]; a dead beam's are all pad_id
    scores: torch.Tensor          # float64 [B, W]
    lengths: torch.Tensor         # int64 [B, W]
    finished: torch.Tensor        # int64 [B, W]
    gaps: torch.Tensor            # float64 [B, num_steps]
    parents: List[torch.Tensor] = field(default_factory=list)       # per step int64 [B, W]
    tokens_in: List[torch.Tensor] = field(default_factory=list)     # per step int64 [B * W, num_steps]: the histories the step ran on
    step_scores: List[torch.Tensor] = field(default_factory=list)   # per step float64 [B, W]: after the step


def beam_search(step_logits: Callable[[torch.Tensor], torch.Tensor], B: int, W: int, num_steps: int, bos_id: int, eos_id: int,
                pad_id: int) -> BeamSearchResult:
    hist = [[[bos_id] + [pad_id] * num_steps for _ in range(W)] for _ in range(B)]
    scores = [[0.0] + [NEG_INF] * (W - 1) for _ in range(B)]
    finished = [[0] * W for _ in range(B)]
    lengths = [[0] * W for _ in range(B)]
    res = BeamSearchResult(None, None, None, None, torch.empty(B, num_steps, dtype=torch.float64))
    for i in range(num_steps):
        flat = torch.tensor([row for img in hist for row in img], dtype=torch.int64)
        res.tokens_in.append(flat[:, :num_steps].clone())
        logits = step_logits(flat[:, :i + 1])
        logits = torch.as_tensor(logits).reshape(B, W, -1)
        parents = []
        for b in range(B):
            st = step_image(logits[b], scores[b], finished[b], lengths[b], hist[b], i, eos_id, pad_id)
            scores[b], finished[b], lengths[b], hist[b] = st.scores, st.finished, st.lengths, st.hist
            parents.append(st.parent)
            res.gaps[b, i] = st.gap
        res.parents.append(torch.tensor(parents, dtype=torch.int64))
        res.step_scores.append(torch.tensor(scores, dtype=torch.float64))
    res.scores = torch.tensor(scores, dtype=torch.float64)
    res.finished = torch.tensor(finished, dtype=torch.int64)
    res.lengths = torch.tensor(lengths, dtype=torch.int64)
    tokens = torch.tensor(hist, dtype=torch.int64)[:, :, 1:]
    tokens[res.scores == NEG_INF] = pad_id
    res.tokens = tokens
    return res


def oracle_step_logits(sd, cfg, images, W: int, rounding=None):
    """`step_logits` over the CPU oracle: the memory of every crop once, then per step the teacher-forced decode of every beam's history
    under the causal mask (the AR loop's, oracle.forward) and the head, at the step's position."""
    from oracle import parseq_oracle as O
    with torch.inference_mode():
        memory = O.encode(sd, cfg, images, rounding).repeat_interleave(W, 0)
    npos = cfg.max_label_length + 1
    mask = torch.triu(torch.ones((npos, npos), dtype=torch.bool), 1)

    def step_logits(histories):
        i = histories.shape[1] - 1
        j = i + 1
        with torch.inference_mode():
            q = sd['pos_queries'][:, i:j].expand(histories.shape[0], -1, -1)
            out = O.decode(sd, cfg, histories, memory, mask[:j, :j], tgt_query=q, tgt_query_mask=mask[i:j, :j], rounding=rounding)
            return O.head(sd, out, rounding)[:, 0].clone()
    return step_logits
