"""Host tests of the cloze refinement of beam hypotheses: the properties of the CPU restatement
(tests/beam_refine_reference.py) on hand-made logits, the refusals of the Python surface that need no device, read.py's argument errors."""
import math

import pytest
import torch

import beam_refine_reference as RR

NEG_INF = float('-inf')
EOS, BOS, PAD = 0, 4, 5      # four classes: <eos> and three characters


def one_hot_logits(picks, C=4, low=-200.0):
    """[len(picks), C]: 0 at the pick, `low` elsewhere — the log-soft-max is 0 / low exactly."""
    lg = torch.full((len(picks), C), low, dtype=torch.float64)
    for i, c in enumerate(picks):
        lg[i, c] = 0.0
    return lg


def rows_of(tokens, scores, finished=None, lengths=None, words=None):
    n = len(scores)
    return RR.Rows([list(t) for t in tokens], list(scores), list(finished or [0] * n), list(lengths or [len(tokens[0])] * n), list(range(10, 10 + n)),
                   list(words or [-1] * n), list(scores))


def test_edit_cuts_at_the_first_eos():
    lg = torch.tensor([[[0., 1., 3., 0.], [2., 1., 0., 0.], [0., 0., 0., 5.], [0., 5., 0., 0.]]])      # arg-max 2, <eos>, 3, 1
    out = RR.refine_image(lg, 'edit', rows_of([[1, 1, 1, 1]], [-3.0]), EOS, PAD)
    assert out.tokens == [[2, EOS, PAD, PAD]] and out.lengths == [1] and out.finished == [1] and out.last == [1]
    lp = torch.log_softmax(lg[0].double(), -1)
    assert out.scores[0] == pytest.approx(float(lp[0, 2] + lp[1, 0]), abs=1e-12)
    assert out.ar_scores == [-3.0] and out.src == [0]
    # no <eos>: every position is read and summed
    lg[0, 1, 0] = -1.0
    out = RR.refine_image(lg, 'edit', rows_of([[1, 1, 1, 1]], [-3.0]), EOS, PAD)
    assert out.tokens == [[2, 1, 3, 1]] and out.lengths == [4] and out.finished == [0] and out.last == [3]
    assert out.scores[0] == pytest.approx(float(lp[0, 2] + torch.log_softmax(lg[0, 1].double(), -1)[1] + lp[2, 3] + lp[3, 1]), abs=1e-12)
    # <eos> first: the empty reading, its score the <eos> term alone
    lg[0, 0, 0] = 9.0
    out = RR.refine_image(lg, 'edit', rows_of([[1, 1, 1, 1]], [-3.0]), EOS, PAD)
    assert out.tokens == [[EOS, PAD, PAD, PAD]] and out.lengths == [0] and out.finished == [1] and out.last == [0]
    # equal maxima: the lower class id
    assert RR.first_argmax(torch.tensor([1.0, 7.0, 7.0, 3.0])) == 1


def test_pseudo_log_likelihood_by_hand():
    """Two positions, two classes: p(c1 | .) = 3/4 at position 0, p(<eos> | .) = 1/2 at position 1."""
    lg = torch.tensor([[[0.0, math.log(3.0)], [0.0, 0.0]]], dtype=torch.float64)
    out = RR.refine_image(lg, 'score', rows_of([[1, EOS]], [-0.7], finished=[1], lengths=[1]), EOS, PAD)
    assert out.scores[0] == pytest.approx(math.log(0.75) + math.log(0.5), abs=1e-15)
    assert out.tokens == [[1, EOS]] and out.finished == [1] and out.lengths == [1] and out.ar_scores == [-0.7]
    # finished one position earlier: only the <eos> term at position 0 counts, whatever the later logits say
    out = RR.refine_image(lg, 'score', rows_of([[EOS, PAD]], [-0.7], finished=[1], lengths=[0]), EOS, PAD)
    assert out.scores[0] == pytest.approx(math.log(0.25), abs=1e-15)
    # unfinished: both positions
    out = RR.refine_image(lg, 'score', rows_of([[1, 1]], [-0.7], finished=[0], lengths=[2]), EOS, PAD)
    assert out.scores[0] == pytest.approx(math.log(0.75) + math.log(0.5), abs=1e-15) and out.last == [1]


def test_duplicates_keep_the_better_then_the_lower_row():
    same = one_hot_logits([1, 2, EOS])
    worse = same.clone()
    worse[0, 3] = -1.0      # same arg-max reading, lower log-probability at position 0
    other = one_hot_logits([3, EOS, 1])
    lg = torch.stack([worse, same, other, same])
    out = RR.refine_image(lg, 'edit', rows_of([[1] * 3] * 4, [-1.0, -2.0, -3.0, -4.0], words=[7, 8, 9, 6]), EOS, PAD)
    # rows 0, 1, 3 read "12": row 1 and 3 score 0, row 0 less; row 1 survives (the lower of the two best), row 2 reads "3"
    assert out.src == [1, 2, 0, 3]
    assert out.tokens == [[1, 2, EOS], [3, EOS, PAD], [PAD] * 3, [PAD] * 3]
    assert out.scores[:2] == [0.0, 0.0] and out.scores[2:] == [NEG_INF, NEG_INF]
    assert out.lengths == [2, 1, 0, 0] and out.finished == [1, 1, 0, 0] and out.words == [8, 9, -1, -1]
    assert out.ar_scores == [-2.0, -3.0, -1.0, -4.0] and out.nodes == [11, 12, 10, 13]      # both travel, also with a removed row
    assert sorted(out.gaps) == [0.0, 0.0, pytest.approx(-float(torch.log_softmax(worse[0], -1)[1]))]
    # 'score' never merges: equal strings stay, in row order at equal scores
    out = RR.refine_image(torch.stack([same, same]), 'score', rows_of([[1, 2, EOS]] * 2, [-1.0, -2.0], finished=[1, 1], lengths=[2, 2]), EOS, PAD)
    assert out.src == [0, 1] and out.scores == [0.0, 0.0] and out.tokens == [[1, 2, EOS]] * 2


def test_ties_and_dead_rows():
    a, b = one_hot_logits([1, 2, 3]), one_hot_logits([3, 2, 1])
    low = one_hot_logits([2, 2, 2])
    low[1, 1] = -0.5
    lg = torch.stack([low, a, a, b, a])
    rows = rows_of([[2, 2, 2], [9, 9, 9], [1, 2, 3], [3, 2, 1], [8, 8, 8]], [-5.0, NEG_INF, -1.0, -6.0, NEG_INF])
    for mode in RR.MODES:
        out = RR.refine_image(lg, mode, rows, EOS, PAD)
        # two different strings at equal scores in row order, the lower score after them, the dead rows last in their order
        assert out.src == [2, 3, 0, 1, 4]
        assert out.scores[0] == out.scores[1] == 0.0 and out.scores[2] < 0 and out.scores[3:] == [NEG_INF, NEG_INF]
        assert out.tokens == [[1, 2, 3], [3, 2, 1], [2, 2, 2], [PAD] * 3, [PAD] * 3]
        assert out.lengths == [3, 3, 3, 0, 0] and out.finished == [0] * 5 and out.last == [2, 2, 2, -1, -1]
        assert out.ar_scores == [-1.0, -6.0, -5.0, NEG_INF, NEG_INF]
        assert out.gaps[0] == 0.0 and out.gaps[1] > 0 and len(out.gaps) == 2
    # every beam dead
    out = RR.refine_image(lg[:2], 'edit', rows_of([[1] * 3] * 2, [NEG_INF, NEG_INF]), EOS, PAD)
    assert out.src == [0, 1] and out.scores == [NEG_INF] * 2 and out.gaps == [] and out.tokens == [[PAD] * 3] * 2


def test_score_mode_is_idempotent():
    g = torch.Generator().manual_seed(5)
    B, W, L, C = 2, 3, 5, 4
    lg = torch.randn(B * W, L, C, generator=g, dtype=torch.float64)
    tokens = torch.randint(1, C, (B * W, L), generator=g).tolist()
    tokens[1][2:] = [EOS, PAD, PAD]
    rows = RR.Rows(tokens, [-1.0, -2.0, NEG_INF, -0.5, -4.0, -3.0], [0, 1, 0, 0, 0, 0], [L, 2, 0, L, L, L], [-1] * 6, [-1] * 6,
                   [-1.0, -2.0, NEG_INF, -0.5, -4.0, -3.0])
    once = RR.concat_rows(RR.refine_rows(lg, 'score', rows, B, W, EOS, PAD))
    # the logits of the second pass belong to the rows in their new order
    perm = [b * W + s for b, src in enumerate(once.src) for s in src]
    twice = RR.concat_rows(RR.refine_rows(lg[perm], 'score', once, B, W, EOS, PAD))
    assert twice.src == [[0, 1, 2]] * B
    for name in ('tokens', 'scores', 'finished', 'lengths', 'ar_scores'):
        assert getattr(once, name) == getattr(twice, name), name
    assert sorted(map(tuple, once.tokens[:W])) == sorted(map(tuple, [tokens[0], tokens[1], [PAD] * L]))


def test_tgt_in_and_search_driver():
    assert RR.tgt_in_of([[1, 2, 3], [EOS, PAD, PAD]], BOS).tolist() == [[BOS, 1, 2], [BOS, EOS, PAD]]
    # two iterations of 'edit': the second runs on the first one's readings
    first, second = one_hot_logits([1, 2, 3]), one_hot_logits([1, EOS, 3])
    seen = []

    def logits_of(it, tgt_in):
        seen.append(tgt_in.tolist())
        return torch.stack([first if it == 0 else second])
    states = RR.refine_search(logits_of, 'edit', 2, rows_of([[3, 3, 3]], [-2.0]), 1, 1, BOS, EOS, PAD)
    assert seen == [[[BOS, 3, 3]], [[BOS, 1, 2]]]
    assert states[0].tokens == [[1, 2, 3]] and states[1].tokens == [[1, EOS, PAD]] and states[1].ar_scores == [-2.0]


def test_python_refusals():
    from parseq_amd.model import check_beam_refine
    check_beam_refine(None, 1)
    check_beam_refine('score', 1, lexicon=object())
    check_beam_refine('edit', 3)
    for args, match in ((('rescore', 1), 'refine must be'), (('edit', 0), 'refine_iters'), (('edit', -2), 'refine_iters'), (('edit', 1.5), 'refine_iters'),
                        (('score', 2), 'idempotent'), ((None, 2), 'without refine'), (('edit', 1, object()), 'lexicon')):
        with pytest.raises(ValueError, match=match):
            check_beam_refine(*args)
    # the public surface refuses before it touches a device
    from parseq_amd import create_model
    m = create_model('parseq-tiny', precision='fp32').eval()
    x = torch.zeros(1, 3, *m.hparams.img_size)
    with pytest.raises(ValueError, match='refine must be'):
        m.beam_search(x, 2, refine='both')
    with pytest.raises(ValueError, match='idempotent'):
        m.beam_search(x, 2, refine='score', refine_iters=2)
    with pytest.raises(ValueError, match='lexicon'):
        m.beam_search(x, 2, lexicon=object(), refine='edit')
    with pytest.raises(ValueError, match='refine_iters'):
        m.model.beam_search(m.tokenizer, x, 2, refine='edit', refine_iters=0)


@pytest.mark.parametrize('argv, message', [
    (['--refine-beams', 'edit'], '--refine-beams needs --nbest'),
    (['--refine-iters', '2', '--nbest', '3'], '--refine-iters needs --refine-beams'),
    (['--nbest', '3', '--refine-beams', 'score', '--refine-iters', '2'], 'runs once'),
    (['--nbest', '3', '--refine-beams', 'edit', '--refine-iters', '0'], 'at least 1'),
    (['--lexicon', 'words.txt', '--refine-beams', 'edit'], 'not allowed with --lexicon'),
    (['--nbest', '3', '--refine-beams', 'polish'], 'invalid choice'),
])
def test_read_cli_argument_errors(argv, message, monkeypatch, capsys):
    pytest.importorskip('PIL.Image')
    import read as read_cli

    def no_model(*a, **kw):
        raise AssertionError('the model must not be loaded after an argument error')
    monkeypatch.setattr(read_cli, 'load_from_checkpoint', no_model)
    with pytest.raises(SystemExit) as e:
        read_cli.main(['pretrained=parseq', '--images', 'a.png', *argv])
    assert e.value.code == 2 and message in capsys.readouterr().err


def test_read_cli_accepts_the_flags():
    pytest.importorskip('PIL.Image')
    import read as read_cli
    parser = read_cli.build_parser()
    assert read_cli.resolve_refine(parser, parser.parse_args(['x', '--nbest', '2'])) == (None, 1)
    assert read_cli.resolve_refine(parser, parser.parse_args(['x', '--nbest', '2', '--refine-beams', 'edit', '--refine-iters', '3'])) == ('edit', 3)
    assert read_cli.resolve_refine(parser, parser.parse_args(['x', '--lexicon', 'w.txt', '--refine-beams', 'score'])) == ('score', 1)
