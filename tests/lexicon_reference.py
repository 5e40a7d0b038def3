"""Lexicon-constrained beam search as DESIGN.md section 19 defines it, restated on the CPU.   *** TEST INFRASTRUCTURE ***

tests/beam_reference.py with the trie: float64 log-soft-max over ALL classes and scores, plain Python sorting for the ranking; a live
unfinished beam at node n offers (w, c) only where next[n][c] >= 0 (a character's child id past the table counts as not allowed, as does
every class of a beam whose own node is outside the table).  A new beam's node is next[node_parent][c]; picking <eos> keeps the node and
records the word id next[node][eos_id]; a finished carry keeps both; a dead slot holds -1 / -1.

  naive_trie    a trie table from the set of prefixes, by the definition (no breadth-first numbering: compared through a walk)
  step_image    one selection step of one image on explicit state (what `parseq_op_beam_step_lexicon` does per workgroup)
  beam_search   the whole search over any `step_logits(histories) -> [rows, C]` callable
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Callable, List, Optional

import torch

import beam_reference as R

NEG_INF = R.NEG_INF


def allowed(next_table, node: int, c: int, eos_id: int) -> bool:
    n_nodes = len(next_table)
    if not 0 <= node < n_nodes:
        return False
    t = int(next_table[node][c])
    return t >= 0 and (c == eos_id or t < n_nodes)


def rank_candidates(logits, scores, finished, nodes, next_table, eos_id: int):
    """beam_reference.rank_candidates, the fresh candidates filtered by the trie; the scores are the unconstrained ones."""
    logp = torch.log_softmax(torch.as_tensor(logits).double(), -1)
    cands = []
    for w, s in enumerate(scores):
        if s == NEG_INF:
            continue
        if finished[w]:
            cands.append((float(s), w, -1))
        else:
            cands += [(float(s) + lp, w, c) for c, lp in enumerate(logp[w].tolist()) if allowed(next_table, nodes[w], c, eos_id)]
    cands.sort(key=lambda t: (-t[0], t[1], t[2]))
    return cands


@dataclass
class StepResult(R.StepResult):
    nodes: List[int] = field(default_factory=list)
    words: List[int] = field(default_factory=list)


def step_image(logits, scores, finished, lengths, hist, nodes, words, next_table, step: int, eos_id: int, pad_id: int) -> StepResult:
    W = len(scores)
    cands = rank_candidates(logits, scores, finished, nodes, next_table, eos_id)
    top = cands[:W + 1]
    gap = min((top[k][0] - top[k + 1][0] for k in range(len(top) - 1)), default=math.inf)
    out = StepResult([], [], [], [], [], [], gap)
    for r in range(W):
        if r < len(cands):
            s, par, cls = cands[r]
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
            s, par, cls, row, fin, length, node, word = NEG_INF, -1, -1, list(hist[r]), 0, 0, -1, -1
        pick = cls if cls >= 0 else pad_id
        if step + 1 < len(row):
            row[step + 1] = pick
        out.scores.append(s); out.finished.append(fin); out.lengths.append(length); out.hist.append(row)
        out.parent.append(par); out.picked.append(pick); out.nodes.append(node); out.words.append(word)
    return out


@dataclass
class BeamSearchResult(R.BeamSearchResult):
    words: Optional[torch.Tensor] = None          # int64 [B, W]: the word id of a finished hypothesis, -1 otherwise
    nodes: Optional[torch.Tensor] = None          # int64 [B, W]


def beam_search(step_logits: Callable[[torch.Tensor], torch.Tensor], B: int, W: int, num_steps: int, bos_id: int, eos_id: int, pad_id: int,
                next_table, roots=None) -> BeamSearchResult:
    next_table = torch.as_tensor(next_table).tolist()
    roots = [0] * B if roots is None else [int(r) for r in roots]
    hist = [[[bos_id] + [pad_id] * num_steps for _ in range(W)] for _ in range(B)]
    scores = [[0.0] + [NEG_INF] * (W - 1) for _ in range(B)]
    nodes = [[roots[b]] + [-1] * (W - 1) for b in range(B)]
    for b in range(B):
        if not 0 <= roots[b] < len(next_table):      # a root outside the table: every beam of the image dead from the start
            scores[b][0], nodes[b][0] = NEG_INF, -1
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
            st = step_image(logits[b], scores[b], finished[b], lengths[b], hist[b], nodes[b], words[b], next_table, i, eos_id, pad_id)
            scores[b], finished[b], lengths[b], hist[b], nodes[b], words[b] = st.scores, st.finished, st.lengths, st.hist, st.nodes, st.words
            parents.append(st.parent)
            res.gaps[b, i] = st.gap
        res.parents.append(torch.tensor(parents, dtype=torch.int64))
        res.step_scores.append(torch.tensor(scores, dtype=torch.float64))
    res.scores = torch.tensor(scores, dtype=torch.float64)
    res.finished = torch.tensor(finished, dtype=torch.int64)
    res.lengths = torch.tensor(lengths, dtype=torch.int64)
    res.words = torch.tensor(words, dtype=torch.int64)
    res.nodes = torch.tensor(nodes, dtype=torch.int64)
    tokens = torch.tensor(hist, dtype=torch.int64)[:, :, 1:]
    tokens[res.scores == NEG_INF] = pad_id
    res.tokens = tokens
    return res


def naive_trie(encoded_words, num_classes: int, eos_id: int):
    """{prefix tuple: {class: True}} and {word tuple: first id} from (id, class-id sequence) pairs: the definition, by prefix sets."""
    prefixes, ends = {()}, {}
    for k, ids in encoded_words:
        ids = tuple(ids)
        for n in range(1, len(ids) + 1):
            prefixes.add(ids[:n])
        ends.setdefault(ids, k)
    return prefixes, ends


def teacher_forced_scores(step_logits, seqs, bos_id: int, eos_id: int, pad_id: int) -> List[float]:
    """Per row r the float64 sum of log_softmax(logits)[t] over the positions of seqs[r] + <eos>, the row's own history fed back: what a
    search that drops nothing must report for that word.  `step_logits` is the adapter beam_search takes (all rows at once per step)."""
    targets = [list(s) + [eos_id] for s in seqs]
    steps = max(len(t) for t in targets)
    hist = torch.full((len(seqs), steps + 1), pad_id, dtype=torch.int64)
    hist[:, 0] = bos_id
    for r, t in enumerate(targets):
        hist[r, 1:len(t) + 1] = torch.tensor(t)
    total = [0.0] * len(seqs)
    for i in range(steps):
        logp = torch.log_softmax(torch.as_tensor(step_logits(hist[:, :i + 1])).double(), -1)
        for r, t in enumerate(targets):
            if i < len(t):
                total[r] += logp[r, t[i]].item()
    return total
