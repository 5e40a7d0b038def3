"""Host tests of scoring given readings: the CPU restatement (tests/score_reference.py) against the oracle's own
greedy decode, the algebra of the two combinations, the rank rule, the parsing of orders and candidates, the refusals of the flags and
the bookkeeping of `LabelAudit` — nothing here needs a device."""
import argparse
import math

import numpy as np
import pytest
import torch

import score_reference as R
from oracle import parseq_oracle as O
from oracle.synth import CONFIGS, synth_images, synth_state_dict
from parseq_amd import score as S
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.evaluate import LabelAudit
from parseq_amd.search_flags import (add_audit_flag, add_evaluation_flags, add_line_flags, add_orientation_flags, add_score_flags, load_candidates,
                                      resolve_audit, resolve_evaluation_flags, resolve_score)
from parseq_amd.tokenizer import Tokenizer

NEG_INF = float('-inf')
TOK = Tokenizer(CHARSET_94_FULL)


# ---- the restatement -----------------------------------------------------------------------------------------------------------------------
def test_forward_score_of_the_greedy_reading_is_the_log_confidence():
    """Teacher-forcing the oracle's own greedy AR reading under the forward order walks the AR loop again: every term is the log of the
    probability `postprocess` multiplies into the confidence, to 1e-5 (fp32 soft-max against a float64 log-soft-max of the same fp32 logits,
    whose own difference between the step-by-step and the one-pass decode is of the order of 1e-6)."""
    cfg = CONFIGS['parseq-tiny']
    sd = synth_state_dict(cfg, 0)
    images = synth_images(4, cfg, seed=21)
    with torch.inference_mode():
        logits = O.forward(sd, cfg, images, cfg.max_label_length, decode_ar=True, refine_iters=0)
        ids, lengths, probs, conf = O.postprocess(logits, cfg.eos_id)
        assert int(lengths.max()) <= cfg.max_label_length and int(lengths.max()) >= 1
        cands = [[ids[b, :int(lengths[b])].tolist()] for b in range(4)]
        T = int(lengths.max())
        got = R.score(sd, cfg, images, cands, S.parse_orders('forward', T))
    for b in range(4):
        n = int(lengths[b])
        want = probs[b, :n + 1].double().log()
        assert np.abs(got['char_lp'][b, 0, 0, :n + 1] - want.numpy()).max() <= 1e-5
        assert abs(float(got['scores'][b, 0]) - math.log(float(conf[b]))) <= 1e-5 * (n + 1)
    assert got['valid'].all() and got['lengths'][:, 0].tolist() == lengths.tolist()


def test_mix_and_mean_algebra():
    g = np.random.default_rng(0)
    s = -10 * g.random((5, 4, 6))
    mix, mean = R.combine(s), R.combine(s, mean=True)
    assert (mix >= mean - 1e-6).all()                                        # Jensen: the log of the mean is at least the mean of the logs
    assert (mix <= s.max(-1) + 1e-6).all() and (mix >= s.max(-1) - math.log(6) - 1e-6).all()
    np.testing.assert_allclose(mix, np.log(np.exp(s).mean(-1)), rtol=1e-6)
    np.testing.assert_allclose(mean, s.mean(-1), rtol=1e-6)
    same = np.repeat(s[..., :1], 3, axis=-1)
    np.testing.assert_allclose(R.combine(same), s[..., 0].astype(np.float32), rtol=1e-7)      # K equal orders: that order
    one = s[..., :1].astype(np.float32)
    assert np.array_equal(R.combine(one), one[..., 0]) and np.array_equal(R.combine(one, mean=True), one[..., 0])      # K = 1: the bits
    # -inf and NaN: an order that cannot produce the string adds nothing to the mixture and sinks the mean
    assert R.combine(np.array([[-2.0, NEG_INF]]))[0] == np.float32(-2.0 - math.log(2)) and R.combine(np.array([[-2.0, NEG_INF]]), mean=True)[0] == NEG_INF
    assert R.combine(np.array([[float('nan'), -3.0]]))[0] == np.float32(-3.0 - math.log(2))
    assert R.combine(np.array([[NEG_INF, NEG_INF]]))[0] == NEG_INF
    # probabilities: the mixture over all candidates of a tiny closed set sums to one when every order's does
    p = g.dirichlet(np.ones(7), size=3)          # 3 orders, each a distribution over 7 strings
    assert abs(np.exp(R.combine(np.log(p).T.astype(np.float64))).sum() - 1.0) <= 1e-6


def test_rank_rule():
    scores = np.array([[-3.0, -1.0, -3.0, NEG_INF, -2.0, -1.0],
                       [-5.0, -5.0, -5.0, -5.0, -5.0, -5.0],
                       [NEG_INF] * 6], dtype=np.float32)
    valid = np.ones((3, 6), dtype=bool)
    valid[0, 4] = False          # absent: last, whatever its score slot holds
    lengths = np.array([[2, 0, 5, 1, 1, 3], [1, 2, 3, 4, 5, 6], [0] * 6])
    assert R.rank(scores, lengths, valid).tolist() == [[1, 5, 0, 2, 3, 4], [0, 1, 2, 3, 4, 5], [0, 1, 2, 3, 4, 5]]
    # per character: -3 / 3, -1 / 1, -3 / 6, -, -, -1 / 4   and   -5 / (n + 1): the longest first
    assert R.rank(scores, lengths, valid, normalize=True).tolist() == [[5, 2, 0, 1, 3, 4], [5, 4, 3, 2, 1, 0], [0, 1, 2, 3, 4, 5]]
    for row in R.rank(scores, lengths, valid):
        assert sorted(row.tolist()) == list(range(6))


def test_layout_is_the_training_step_layout():
    cands = [[[5, 9, 11], [], None, [5, 97], [5, 0, 9]]]
    tgt_in, targets, lengths, valid = R.layout(cands, 5, 95, 95, 0, 96)
    assert tgt_in.tolist() == [[95, 5, 9, 11, 96], [95, 96, 96, 96, 96], [95, 96, 96, 96, 96], [95, 96, 96, 96, 96], [95, 96, 96, 96, 96]]
    assert targets.tolist() == [[5, 9, 11, 0, -1], [0, -1, -1, -1, -1], [-1] * 5, [-1] * 5, [-1] * 5]
    assert lengths.tolist() == [3, 0, 0, 0, 0] and valid.tolist() == [True, True, False, False, False]
    # the key padding of training_step on tokenizer.encode: <pad> and <eos> inputs; here the <eos> input slot holds <pad>
    enc = TOK.encode(['abc', ''])[:, :-1]
    pad_train = (enc == TOK.pad_id) | (enc == TOK.eos_id)
    rows = torch.from_numpy(S.encode_candidates(TOK, [['abc'], ['']], 25)[0][:, 0]).long()
    mine = R.layout([[r[:list(r).index(0)].tolist()] for r in rows], 4, 95, TOK.bos_id, TOK.eos_id, TOK.pad_id)[0]
    assert torch.equal(mine == TOK.pad_id, pad_train)


# ---- orders and candidates -------------------------------------------------------------------------------------------------------------------
class _Sys:
    max_gen_perms, perm_forward, perm_mirrored = 3, True, True


def test_parse_orders():
    assert S.parse_orders('forward', 3).tolist() == [[0, 1, 2, 3, 4]]
    assert S.parse_orders('mirrored', 3).tolist() == [[0, 4, 3, 2, 1]]
    assert S.parse_orders('both', 1).tolist() == [[0, 1, 2], [0, 2, 1]]
    from parseq_amd.system import gen_tgt_perms
    for T in (3, 7):
        torch.manual_seed(5)
        want = gen_tgt_perms(torch.zeros(1, T + 2, dtype=torch.long), 3, True, True, np.random.default_rng(5))
        state = torch.random.get_rng_state()
        torch.manual_seed(99)
        before = torch.random.get_rng_state()
        got = S.parse_orders(4, T, _Sys(), seed=5)
        assert torch.equal(got, want[:4]) and torch.equal(torch.random.get_rng_state(), before)      # the caller's generator is left alone
        torch.random.set_rng_state(state)
        assert got[0].tolist() == list(range(T + 2)) and got[1].tolist() == [0] + list(range(T + 1, 0, -1))
    t = torch.tensor([[0, 2, 1, 3, 4], [0, 4, 1, 2, 3]])
    assert torch.equal(S.parse_orders(t, 3), t)
    for bad in ('backward', True, 0, 17, torch.tensor([[0, 1, 2]]), torch.tensor([[1, 0, 2, 3, 4]]), torch.tensor([[0, 1, 1, 3, 4]]), torch.zeros(0, 5)):
        with pytest.raises(ValueError):
            S.parse_orders(bad, 3, _Sys())
    with pytest.raises(ValueError, match='gen_tgt_perms gives'):
        S.parse_orders(7, 3, _Sys())          # 3 characters: 3! / 2 pairs = 6 orderings
    with pytest.raises(ValueError):
        S.parse_orders(2, 3)                  # an int needs the system's settings
    m = S.query_masks(S.parse_orders('both', 3))
    assert m.dtype == torch.uint8 and tuple(m.shape) == (2, 4, 4)
    assert m[0].tolist() == torch.triu(torch.ones(4, 4, dtype=torch.uint8), 1).tolist()
    assert torch.equal(m[1].bool(), O.attn_masks_from_perm(torch.tensor([0, 4, 3, 2, 1]))[1])


def test_encode_candidates():
    rows, T = S.encode_candidates(TOK, [['ab', 'abcd'], ['', 'a', 'b'], 'xyz'], 25)
    assert T == 4 and rows.shape == (3, 3, 5) and rows.dtype == np.int32
    a, b = TOK._stoi['a'], TOK._stoi['b']
    assert rows[0, 0].tolist() == [a, b, TOK.eos_id, TOK.pad_id, TOK.pad_id] and rows[0, 2].tolist() == [TOK.pad_id] * 5      # ragged: absent
    assert rows[1, 0].tolist() == [TOK.eos_id] + [TOK.pad_id] * 4 and rows[2, 0, :4].tolist() == [TOK._stoi[c] for c in 'xyz'] + [TOK.eos_id]
    assert S.encode_candidates(TOK, [['']], 25)[1] == 1          # T is at least 1: two positions
    with pytest.raises(ValueError, match='charset'):
        S.encode_candidates(TOK, [['ab', 'aéb']], 25)
    with pytest.raises(ValueError, match='charset'):
        S.encode_candidates(Tokenizer('0123456789'), [['12a']], 25)
    for bad in ([], [[]], [['a'] * 17], [['a' * 26]], [[5]]):
        with pytest.raises(ValueError):
            S.encode_candidates(TOK, bad, 25)
    with pytest.raises(ValueError):
        S.score_flags('sum', False)
    assert (S.score_flags('mix', False), S.score_flags('mean', False), S.score_flags('mix', True), S.score_flags('mean', True)) == (0, 1, 2, 3)


def test_score_result_best_and_decode_scores():
    scores = torch.tensor([[-3.0, -1.0, NEG_INF], [-2.0, -4.0, -9.0]])
    lp = torch.arange(2 * 3 * 2 * 4, dtype=torch.float32).view(2, 3, 2, 4)
    res = S.ScoreResult(scores, torch.zeros(2, 3, 2), lp, torch.tensor([[1, 0, 2], [0, 1, 2]], dtype=torch.int32),
                        torch.tensor([[2, 3, 0], [1, 0, 2]], dtype=torch.int32), torch.tensor([[1, 1, 0], [1, 1, 1]], dtype=torch.uint8), S.parse_orders('both', 3))
    idx, best = res.best()
    assert idx.tolist() == [1, 0] and best.tolist() == [-1.0, -2.0]
    out = TOK.decode_scores(res, [['ab', 'abc'], ['a', '', 'ab']])
    assert [[(s, v) for s, v, _ in crop] for crop in out] == [[('abc', -1.0), ('ab', -3.0)], [('a', -2.0), ('', -4.0), ('ab', -9.0)]]
    assert out[0][0][2] == [lp[0, 1, 0, :4].tolist(), lp[0, 1, 1, :4].tolist()] and out[1][1][2] == [[lp[1, 1, 0, 0].item()], [lp[1, 1, 1, 0].item()]]


# ---- the flags ---------------------------------------------------------------------------------------------------------------------------------
def _read_parser():
    import read
    return read.build_parser()


def _refused(parser, argv, resolve):
    with pytest.raises(SystemExit):
        resolve(parser, parser.parse_args(argv))


def test_read_flags(tmp_path, capsys):
    p = _read_parser()
    base = ['ckpt', '--images', 'a.png']
    assert resolve_score(p, p.parse_args(base)) is None
    f = resolve_score(p, p.parse_args(base + ['--candidates', 'c.txt', '--orders', 'both', '--length-norm']))
    assert f == ('c.txt', None, 'both', True)
    assert resolve_score(p, p.parse_args(base + ['--expect', 'ab', '--orders', '6'])) == (None, ['ab'], 6, False)
    assert resolve_score(p, p.parse_args(base + ['--expect', 'ab', '--regions', 'r.txt'])).orders == 'forward'
    for extra in (['--nbest', '3'], ['--beam', '4'], ['--lexicon', 'w.txt'], ['--lexicon', 'w.txt', '--match'], ['--lm', 'c.txt'], ['--pattern', 'a+'],
                  ['--refine-beams', 'score'], ['--auto-rotate', 'flip'], ['--upright-bias', '0.1'], ['--lines'], ['--line-sep', '0.1'], ['--boxes'],
                  ['--candidates', 'c.txt'], ['--orders', 'sideways'], ['--orders', '0'], ['--orders', '17']):
        _refused(p, base + ['--expect', 'ab'] + extra, resolve_score)
    _refused(p, base + ['--orders', 'both'], resolve_score)
    _refused(p, base + ['--length-norm'], resolve_score)
    capsys.readouterr()
    path = tmp_path / 'c.txt'
    path.write_text('ab\tabc\n\nx y\tz\r\n', encoding='utf-8')
    assert load_candidates(str(path)) == [['ab', 'abc'], [''], ['x y', 'z']]


def test_audit_flags(capsys):
    import test as T
    p = T.build_parser()
    a = p.parse_args(['ckpt'])
    assert resolve_audit(p, a, resolve_evaluation_flags(p, a)) is None
    a = p.parse_args(['ckpt', '--audit'])
    assert resolve_audit(p, a, None) == (20, 'forward', False)
    a = p.parse_args(['ckpt', '--audit', '3', '--orders', 'both', '--length-norm'])
    assert resolve_audit(p, a, None) == (3, 'both', True)
    for argv in (['--audit', '0'], ['--audit', '--auto-rotate', 'flip'], ['--orders', 'both'], ['--audit', '--orders', 'x']):
        a = p.parse_args(['ckpt'] + argv)
        with pytest.raises(SystemExit):
            resolve_audit(p, a, None)
    for argv in (['--beam', '4'], ['--lexicon', 'w.txt'], ['--pattern', 'a+']):
        a = p.parse_args(['ckpt', '--audit'] + argv)
        with pytest.raises(SystemExit):
            resolve_audit(p, a, resolve_evaluation_flags(p, a))
    capsys.readouterr()


# ---- LabelAudit ----------------------------------------------------------------------------------------------------------------------------------
class _Model:
    max_label_length = 6


class _System:
    tokenizer = Tokenizer('0123456789abcdefghijklmnopqrstuvwxyz')
    model = _Model()
    max_gen_perms, perm_forward, perm_mirrored = 3, True, True


def test_label_audit_bookkeeping():
    audit = LabelAudit(_System(), orders='both')
    tok = _System.tokenizer
    assert audit.perms.tolist() == S.parse_orders('both', 6).tolist()
    rows, ok = audit.label_rows(['ab1', 'aB', '', 'abcdefg'])
    assert ok.tolist() == [True, False, True, False]          # 'B' is outside the training charset; seven characters are too many
    assert rows[0].tolist() == [tok._stoi['a'], tok._stoi['b'], tok._stoi['1'], tok.eos_id] + [tok.pad_id] * 3 and (rows[1] == tok.pad_id).all()
    ids = torch.tensor([[11, 12, 0, 5, 5], [11, 12, 13, 14, 15], [0, 3, 3, 3, 3]], dtype=torch.int32)
    got = audit.reading_rows(ids, torch.tensor([2, 5, 0], dtype=torch.int32))
    P = tok.pad_id
    assert got.tolist() == [[11, 12, 0, P, P, P, P], [11, 12, 13, 14, 15, 0, P], [0] + [P] * 6]
    full = audit.reading_rows(torch.full((1, 7), 9, dtype=torch.int32), torch.tensor([7], dtype=torch.int32))
    assert full.tolist() == [[9] * 7]                         # no <eos>: a row the staging kernel calls invalid
    # two batches of planted scores: (label score, reading score), validity, mismatch
    audit.add_scores(['ab', 'cd', 'ef'], torch.tensor([[-5.0, -1.0], [-2.0, -2.5], [-3.0, -3.0]]), torch.ones(3, 2, dtype=torch.uint8),
                     torch.tensor([True, True, False]), torch.tensor([[11, 13, 0], [13, 14, 0], [15, 16, 0]], dtype=torch.int32), torch.tensor([2, 2, 2]))
    audit.add_scores(['gh', 'iJ', 'kl', 'mn'], torch.tensor([[-9.0, -5.0], [NEG_INF, -1.0], [-4.0, NEG_INF], [-7.0, -3.0]]),
                     torch.tensor([[1, 1], [0, 1], [1, 0], [1, 1]], dtype=torch.uint8), torch.tensor([True, True, True, True]),
                     torch.tensor([[17, 17, 18, 0], [19, 20, 0, 5], [1, 2, 3, 4], [23, 24, 0, 0]], dtype=torch.int32), torch.tensor([3, 2, 4, 2]))
    rep = audit.result()
    assert rep.labels == ['ab', 'cd', 'ef', 'gh', 'iJ', 'kl', 'mn'] and rep.readings == ['ac', 'cd', 'ef', 'ggh', 'ij', '0123', 'mn']
    assert rep.mismatch.tolist() == [True, True, False, True, True, True, True] and rep.unscorable == 2
    np.testing.assert_array_equal(np.isnan(rep.suspicion), [False, False, True, False, True, True, False])
    assert rep.suspicion[[0, 1, 3, 6]].tolist() == [4.0, -0.5, 4.0, 4.0]
    top = audit.top(3)
    assert [r['index'] for r in top] == [0, 3, 6] and top[0] == dict(index=0, label='ab', reading='ac', label_score=-5.0, reading_score=-1.0, suspicion=4.0)
    assert [r['index'] for r in rep.top(10)] == [0, 3, 6, 1] and rep.top(0) == []
    audit.reset()
    assert audit.result().labels == [] and audit.top(5) == []
