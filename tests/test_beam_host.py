"""CPU tests of the beam-search restatement (tests/beam_reference.py) that the GPU tests of tests/test_beam.py compare against: it
equals a brute-force enumeration where nothing is pruned, its width-1 search is the oracle's greedy AR decode, and its ranking rule
resolves equal scores as DESIGN.md section 18 states."""
import itertools
import math

import torch

import beam_reference as R
from oracle import parseq_oracle as O
from oracle.synth import CONFIGS, synth_state_dict

EOS, BOS, PAD = 0, 3, 4


def _made_up_logits(history):
    """Three logits that are a fixed function of the history: a seeded draw keyed by the history's digits."""
    g = torch.Generator().manual_seed(1 + sum((int(t) + 1) * 7 ** k for k, t in enumerate(history)))
    return torch.randn(3, generator=g, dtype=torch.float64) * 2.0


def test_restatement_equals_brute_force_when_nothing_is_pruned():
    """3 classes (class 0 = <eos>), 3 steps, W = 27: at most 3, 7 and 15 candidates per step, so no hypothesis is ever dropped and the
    search must return every hypothesis — the sequences that end at their first <eos> and the unfinished ones of full length — in
    score order, followed by dead slots."""
    steps, W = 3, 27
    step_logits = lambda h: torch.stack([_made_up_logits(row.tolist()) for row in h])      # noqa: E731
    got = R.beam_search(step_logits, 1, W, steps, BOS, EOS, PAD)
    want = []
    for n in range(1, steps + 1):
        for seq in itertools.product(range(3), repeat=n):
            ended = seq[-1] == EOS
            if EOS in seq[:-1] or (not ended and n < steps):
                continue
            score, hist = 0.0, [BOS]
            for t in seq:
                score += torch.log_softmax(_made_up_logits(hist), -1)[t].item()
                hist.append(t)
            want.append((score, list(seq) + [PAD] * (steps - n), n - 1 if ended else n, int(ended)))
    want.sort(key=lambda t: -t[0])
    assert len(want) == 15
    assert min(a[0] - b[0] for a, b in zip(want, want[1:])) > 1e-9      # no ties: the ranking is the scores' alone
    for r, (score, toks, length, fin) in enumerate(want):
        assert got.tokens[0, r].tolist() == toks
        assert abs(got.scores[0, r].item() - score) < 1e-12
        assert got.lengths[0, r].item() == length and got.finished[0, r].item() == fin
    assert (got.scores[0, 15:] == -math.inf).all() and (got.tokens[0, 15:] == PAD).all() and (got.lengths[0, 15:] == 0).all()


def test_width_one_is_the_oracles_greedy_decode(golden):
    name = 'parseq-tiny'
    g, _ = golden(name)
    cfg, sd = CONFIGS[name], synth_state_dict(CONFIGS[name], 0)
    images = g['images']
    with torch.inference_mode():
        logits = O.forward(sd, cfg, images, 25, decode_ar=True, refine_iters=0)
    ids, lengths = O.postprocess(logits, cfg.eos_id)[:2]
    got = R.beam_search(R.oracle_step_logits(sd, cfg, images, 1), images.shape[0], 1, 26, cfg.bos_id, cfg.eos_id, cfg.pad_id)
    for b in range(images.shape[0]):
        n = int(lengths[b])
        assert got.lengths[b, 0].item() == n
        assert got.tokens[b, 0, :n].tolist() == ids[b, :n].tolist()
        assert got.finished[b, 0].item() == int(n < 26)
        if n < 26:
            assert got.tokens[b, 0, n].item() == cfg.eos_id and (got.tokens[b, 0, n + 1:] == cfg.pad_id).all()
        want = torch.log_softmax(logits[b, :min(n + 1, 26)].double(), -1).max(-1).values.sum().item()
        assert abs(got.scores[b, 0].item() - want) < 1e-9


def test_equal_scores_from_two_parents():
    """Two beams with the same score and the same logits row: every candidate pair ties, the lower parent goes first, then the lower class."""
    row = [0.0, 2.0, 2.0, -1.0]
    st = R.step_image(torch.tensor([row, row]), [-1.5, -1.5], [0, 0], [2, 2], [[BOS, 1, 2, PAD], [BOS, 2, 1, PAD]], 2, EOS, PAD)
    assert st.parent == [0, 0] and st.picked == [1, 2] and st.gap == 0.0
    assert st.hist == [[BOS, 1, 2, 1], [BOS, 1, 2, 2]]
    st = R.step_image(torch.tensor([row, row, row]), [-1.5, -1.5, -1.5], [0, 0, 0], [2, 2, 2], [[BOS, 1, 2, PAD], [BOS, 2, 1, PAD], [BOS, 2, 2, PAD]], 2, EOS, PAD)
    assert st.parent == [0, 0, 1] and st.picked == [1, 2, 1]


def test_finished_carry_ties_with_a_fresh_candidate():
    """A finished beam whose score equals a fresh candidate's: on the same parent index the carry (class -1) goes first; against a
    lower parent's candidate the parent decides."""
    lp = torch.log_softmax(torch.tensor([0.0, 1.0, 3.0], dtype=torch.float64), -1)
    tie = -2.0 + lp[2].item()                      # beam 0's best candidate
    st = R.step_image(torch.tensor([[0.0, 1.0, 3.0], [0.0, 0.0, 0.0]]), [-2.0, tie], [0, 1], [1, 0], [[BOS, 1, PAD], [BOS, EOS, PAD]], 1, EOS, PAD)
    assert st.scores[0] == st.scores[1] == tie
    assert st.parent == [0, 1] and st.picked == [2, PAD] and st.finished == [0, 1] and st.lengths == [2, 0]
    # the carry on parent 0, the live beam on parent 1: the carry's parent is lower
    st = R.step_image(torch.tensor([[0.0, 0.0, 0.0], [0.0, 1.0, 3.0]]), [tie, -2.0], [1, 0], [0, 1], [[BOS, EOS, PAD], [BOS, 1, PAD]], 1, EOS, PAD)
    assert st.parent == [0, 1] and st.picked == [PAD, 2] and st.finished == [1, 0]
