"""Host tests of line reading: the window plan of parseq_amd/preprocess.py against its definition and against
the numpy restatement, literal cases of the restated stitch, the recovery property that argues for the rule, and what needs no device of
`read_lines`, `decode_lines` and read.py's flags."""
import math

import numpy as np
import pytest
import torch

import line_reference as R
from parseq_amd.model import LineResult, check_lines, chunk_lines
from parseq_amd.preprocess import LINE_MAX_WINDOWS, line_plan, line_windows
from parseq_amd.search_flags import resolve_lines

IMG = (32, 128)


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def test_a_line_no_wider_than_a_window_is_one_window():
    assert line_windows(32, 100, IMG) == [(0, 100)]
    assert line_windows(32, 128, IMG) == [(0, 128)]
    assert line_windows(48, 192, IMG) == [(0, 192)]
    assert line_windows(1, 1, IMG) == [(0, 1)]


def test_one_column_more_gives_two_windows():
    assert line_windows(32, 129, IMG) == [(0, 128), (1, 128)]


def test_plan_properties_on_random_sizes():
    rng = np.random.default_rng(0)
    for _ in range(500):
        h, w = int(rng.integers(1, 200)), int(rng.integers(1, 3000))
        overlap, aspect = float(rng.choice([0.0, 0.1, 0.25, 0.5, 0.75])), float(rng.choice([0.25, 0.8, 1.0, 1.5, 4.0]))
        ww = max(1, math.floor(h * IMG[1] / IMG[0] * aspect + 0.5))
        ov = math.floor(ww * overlap + 0.5)
        s = max(1, ww - ov)
        K = 1 if w <= ww else -(-(w - ww) // s) + 1
        if K > LINE_MAX_WINDOWS:
            with pytest.raises(ValueError):
                line_windows(h, w, IMG, overlap, aspect)
            continue
        got = line_windows(h, w, IMG, overlap, aspect)
        assert got == R.line_windows(h, w, IMG, overlap, aspect)
        assert len(got) == K
        assert got[0][0] == 0 and got[-1][0] + got[-1][1] == w
        for (xa, wa), (xb, wb) in zip(got, got[1:]):
            assert xa < xb and wa == wb == ww
            assert xa + wa - xb >= ov                       # neighbours share at least ov columns ...
            assert xb <= xa + wa                            # ... and leave no gap, so the union is [0, w)


def test_window_limit():
    s = 96
    assert len(line_windows(32, 128 + 63 * s, IMG)) == 64
    with pytest.raises(ValueError, match='65 windows'):
        line_windows(32, 128 + 63 * s + 1, IMG)


@pytest.mark.parametrize('kw', [dict(overlap=-0.01), dict(overlap=0.76), dict(overlap=float('nan')), dict(aspect=0.2), dict(aspect=4.5), dict(aspect=float('nan'))])
def test_plan_refuses_parameters(kw):
    with pytest.raises(ValueError):
        line_windows(32, 500, IMG, **kw)


def test_plan_refuses_sizes():
    for h, w in ((0, 10), (10, 0), (-1, 5)):
        with pytest.raises(ValueError):
            line_windows(h, w, IMG)


def test_line_plan_table_and_chunks():
    win, first = line_plan([(32, 100), (32, 500), (48, 1000)], IMG)
    assert first == [0, 1, 6, 13]
    assert win[0] == (0, 100, 32) and win[1:6] == [(0, 128, 32), (96, 128, 32), (192, 128, 32), (288, 128, 32), (372, 128, 32)]
    assert all(r[1:] == (192, 48) for r in win[6:]) and win[-1][0] == 1000 - 192
    assert chunk_lines(first, 512) == [(0, 3)]
    assert chunk_lines(first, 8) == [(0, 2), (2, 3)]
    assert chunk_lines([0, 5, 10, 15], 8) == [(0, 1), (1, 2), (2, 3)]
    with pytest.raises(ValueError, match='line 1 has 5 windows'):
        chunk_lines(first, 4)


def test_read_lines_refusals_without_a_device():
    check_lines(0.25, 1.0, 0.25, None, 512)
    for bad in ((0.8, 1.0, 0.25, None, 512), (0.25, 5.0, 0.25, None, 512), (0.25, 1.0, -1.0, None, 512), (0.25, 1.0, float('nan'), None, 512),
                (0.25, 1.0, float('inf'), None, 512), (0.25, 1.0, 0.25, 0, 512), (0.25, 1.0, 0.25, 2049, 512), (0.25, 1.0, 0.25, None, 0)):
        with pytest.raises(ValueError):
            check_lines(*bad)


# ---- literal cases of the stitch ---------------------------------------------------------------------------------------------------------
def _line(windows, x0s, ww=128, h=32, L=8):
    """Arrays of one line from per-window lists of (token, X in source pixels, probability); boxes are centre -+ 1 in x, rows 2 .. 30."""
    K = len(windows)
    tokens, probs = np.zeros((K, L), np.int32), np.full((K, L), 0.5, np.float32)
    centres, boxes, lengths = np.zeros((K, L, 2), np.float32), np.zeros((K, L, 4), np.float32), np.zeros(K, np.int32)
    for k, chars in enumerate(windows):
        lengths[k] = len(chars)
        for i, (tok, X, p) in enumerate(chars):
            cx = (X - x0s[k]) * IMG[1] / ww
            tokens[k, i], probs[k, i], centres[k, i] = tok, p, (cx, 16.0)
            boxes[k, i] = (cx - 1, 2, cx + 1, 30)
    win = np.array([(x0, ww, h) for x0 in x0s], np.int32)
    return tokens, lengths, probs, centres, boxes, win


def _stitch(windows, x0s, min_sep=8.0, max_out=16, C=95, **kw):
    return R.stitch_line(*_line(windows, x0s, **kw), C, IMG, min_sep, max_out)


def _src(out):
    return [tuple(r) for r in out['src'][:min(out['len'], len(out['src']))].tolist()]


X0 = (0, 96, 192)          # windows of 128 columns: cuts at 112 and 208; with min_sep 8 the bands are (-inf, 116), [108, 212), [204, inf)


def test_band_edges_lo_is_kept_hi_is_not():
    out = _stitch([[(5, 116.0, 0.9)], [(6, 108.0, 0.9), (7, 107.99, 0.9), (8, 212.0, 0.9)], []], X0)
    assert _src(out) == [(1, 0)]
    assert out['tokens'][:2].tolist() == [6, -1] and out['x'][0] == 108.0
    out = _stitch([[(5, 115.99, 0.9)], [], [(9, 204.0, 0.9)]], X0)
    assert _src(out) == [(0, 0), (2, 0)]


def test_a_nan_centre_is_dropped_everywhere():
    nan, inf = float('nan'), float('inf')
    out = _stitch([[(5, nan, 0.9), (6, -inf, 0.9), (7, inf, 0.9)], [(5, nan, 0.9)], [(5, nan, 0.9), (8, inf, 0.9), (9, -inf, 0.9)]], X0)
    assert _src(out) == [(0, 1)]                       # -inf passes -inf <= X in window 0; +inf < +inf is false even in the last window
    out = _stitch([[(5, nan, 0.9), (4, 3.0, 0.9)]], (0,))
    assert _src(out) == [(0, 1)]


def test_equal_and_nan_probabilities_keep_the_left_reading():
    nan = float('nan')
    for pa, pb in ((0.7, 0.7), (nan, 0.9), (0.2, nan), (nan, nan)):
        out = _stitch([[(5, 110.0, pa)], [(5, 111.0, pb)], []], X0)
        assert _src(out) == [(0, 0)]
    out = _stitch([[(5, 110.0, 0.7)], [(5, 111.0, 0.8)], []], X0)
    assert _src(out) == [(1, 0)]
    out = _stitch([[(5, 110.0, 0.7)], [(6, 111.0, 0.8)], []], X0)          # another token: no duplicate
    assert _src(out) == [(0, 0), (1, 0)]


def test_nearest_unmatched_reading_is_the_match_and_ties_go_left():
    # window 0 holds the token at 109 and 113, window 1 at 111 (a tie: the lower position, 109) and at 112 (109 is taken: 113)
    out = _stitch([[(5, 109.0, 0.9), (5, 113.0, 0.1)], [(5, 111.0, 0.5), (5, 112.0, 0.5)], []], X0)
    assert _src(out) == [(0, 0), (1, 1)]


def test_min_sep_zero_disables_the_duplicate_step():
    chars = [[(5, 111.9, 0.9)], [(5, 112.1, 0.9)], []]
    assert _src(_stitch(chars, X0, min_sep=8.0)) == [(0, 0)]
    assert _src(_stitch(chars, X0, min_sep=0.0)) == [(0, 0), (1, 0)]


def test_single_survivor_chain():
    """Three windows of 8 columns at 0, 4, 8: cuts 6 and 10, bands (-inf, 10), [2, 14), [6, inf) — one character at 8 is kept by all three.
    Each seam decides on its own: the middle reading can displace the left one and still lose to the right one; and where it loses to both,
    both outer readings stay.  This is the accepted imperfection of section 29, restated, not repaired."""
    def run(p0, p1, p2):
        return _src(_stitch([[(5, 8.0, p0)], [(5, 8.0, p1)], [(5, 8.0, p2)]], (0, 4, 8), ww=8, h=2))
    assert run(0.5, 0.9, 0.95) == [(2, 0)]
    assert run(0.5, 0.9, 0.1) == [(1, 0)]
    assert run(0.9, 0.5, 0.95) == [(0, 0), (2, 0)]


def test_truncation_keeps_the_true_count():
    chars = [[(5 + i, 10.0 * i + 5, 0.9) for i in range(7)]]
    out = _stitch(chars, (0,), max_out=3)
    assert out['len'] == 7 and out['tokens'].tolist() == [5, 6, 7] and out['src'].tolist() == [[0, 0], [0, 1], [0, 2]]
    full = _stitch(chars, (0,), max_out=16)
    assert full['confidence'] == out['confidence']


def test_candidates_lengths_and_confidence():
    tokens, lengths, probs, centres, boxes, win = _line([[(5, 10.0, 0.5), (95, 20.0, 0.5), (-1, 30.0, 0.5), (7, 40.0, 0.25)]], (0,))
    probs[0, 4] = 0.5                                                         # the <eos> position
    out = R.stitch_line(tokens, lengths, probs, centres, boxes, win, 95, IMG, 8.0, 8)
    assert _src(out) == [(0, 0), (0, 3)] and out['confidence'] == np.float32(0.5 * 0.25 * 0.5)
    assert out['boxes'][0].tolist() == [9.0, 2.0, 11.0, 30.0]
    # a length is clamped to [0, L]; at L = 8 the four unused positions (token 0 at x = 0) are candidates too, and there is no <eos> factor
    for n, want in ((-3, []), (0, []), (1, [(0, 0)]), (99, [(0, 0), (0, 3), (0, 4), (0, 5), (0, 6), (0, 7)])):
        lengths[0] = n
        assert _src(R.stitch_line(tokens, lengths, probs, centres, boxes, win, 95, IMG, 8.0, 8)) == want
    assert R.stitch_line(tokens, lengths, probs, centres, boxes, win, 95, IMG, 8.0, 8)['confidence'] == np.float32(0.5 * 0.25 * 0.5 ** 4)


def test_boxes_scale_with_the_window():
    out = _stitch([[(5, 100.0, 0.9)]], (40,), ww=256, h=64)
    assert out['x'][0] == 100.0 and out['boxes'][0].tolist() == [98.0, 4.0, 102.0, 60.0]


# ---- the recovery property ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('seed', range(200))
def test_planted_line_is_recovered(seed):
    """The argument for the rule (derivation in DESIGN.md section 29).  Characters stand at known centres, neighbours at least 2 min_sep apart;
    a window reports every character inside it by a margin e, e + 2 delta <= ov / 2, and maybe the ones nearer its edge; every estimate is off
    by less than delta = min_sep / 2.  Then the stitched string is the planted one."""
    rng = np.random.default_rng(seed)
    h = int(rng.choice([16, 32, 48]))
    overlap = float(rng.choice([0.25, 0.5]))
    w = int(rng.integers(h * 4 + 1, h * 40))
    wins = R.line_windows(h, w, IMG, overlap)
    ww = wins[0][1]
    ov = math.floor(ww * overlap + 0.5)
    min_sep = 0.25 * h
    delta = min_sep / 2
    e = ov / 2 - 2 * delta
    assert e >= 0
    centres_true, toks, x = [], [], e + float(rng.uniform(0, 2 * min_sep))      # (nothing stands within e of the line's ends: no window must report it)
    while x <= w - e:
        centres_true.append(x)
        toks.append(toks[-1] if toks and rng.random() < 0.3 else int(rng.integers(1, 6)))       # doubled letters, a small alphabet
        x += float(rng.uniform(2 * min_sep, 3.5 * min_sep)) + 1e-6
    L = 1 + max(sum(1 for c in centres_true if x0 <= c <= x0 + ww) for x0, _ in wins)
    K = len(wins)
    tokens, probs = np.zeros((K, L), np.int32), rng.uniform(0.05, 1.0, (K, L)).astype(np.float32)
    cen, boxes, lengths = np.zeros((K, L, 2), np.float32), np.zeros((K, L, 4), np.float32), np.zeros(K, np.int32)
    for k, (x0, _) in enumerate(wins):
        i = 0
        for c, t in zip(centres_true, toks):
            inside = x0 + e <= c <= x0 + ww - e
            if inside or (x0 <= c <= x0 + ww and rng.random() < 0.5):
                est = c + float(rng.uniform(-0.99, 0.99)) * delta
                tokens[k, i], cen[k, i, 0] = t, (est - x0) * IMG[1] / ww
                i += 1
        lengths[k] = i
    win = np.array([(x0, ww, h) for x0, _ in wins], np.int32)
    out = R.stitch_line(tokens, lengths, probs, cen, boxes, win, 95, IMG, min_sep, len(toks) + 8)
    assert out['len'] == len(toks)
    assert out['tokens'][:out['len']].tolist() == toks


# ---- decode_lines and the flags ------------------------------------------------------------------------------------------------------------
def test_decode_lines_on_a_hand_made_result():
    from parseq_amd.tokenizer import Tokenizer
    tok = Tokenizer('abc')
    ids = tok.encode(['abca', 'c'])[:, 1:]                     # characters, <eos>, <pad>
    tokens = torch.full((2, 3), -1, dtype=torch.int32)
    tokens[0] = ids[0, :3].to(torch.int32)                       # four survivors, three slots
    tokens[1, 0] = int(ids[1, 0])
    boxes = torch.arange(24, dtype=torch.float32).reshape(2, 3, 4)
    res = LineResult(torch.tensor([4, 1], dtype=torch.int32), tokens, torch.zeros(2, 3), boxes, torch.zeros(2, 3, dtype=torch.float64),
                     torch.zeros(2, 3, 2, dtype=torch.int32), torch.tensor([0.5, 0.25]), None)
    assert tok.decode_lines(res) == (['abc', 'c'], [0.5, 0.25])
    labels, conf, chars = tok.decode_lines(res, boxes=True)
    assert labels == ['abc', 'c'] and conf == [0.5, 0.25]
    assert chars[0] == [('a', (0.0, 1.0, 2.0, 3.0)), ('b', (4.0, 5.0, 6.0, 7.0)), ('c', (8.0, 9.0, 10.0, 11.0))] and chars[1] == [('c', (12.0, 13.0, 14.0, 15.0))]


def _resolve(argv):
    import read as read_cli
    parser = read_cli.build_parser()
    args, _ = parser.parse_known_args(['pretrained=parseq', '--images', 'a.png'] + argv)
    return resolve_lines(parser, args)


def test_line_flags_parse():
    assert _resolve([]) is None
    assert _resolve(['--lines']) == (0.25, 0.25)
    assert _resolve(['--lines', '--line-overlap', '0.5', '--line-sep', '0']) == (0.5, 0.0)
    assert _resolve(['--lines', '--boxes', '--regions', 'a.txt']) == (0.25, 0.25)


@pytest.mark.parametrize('argv', [['--line-overlap', '0.5'], ['--line-sep', '0.1'], ['--lines', '--nbest', '3'], ['--lines', '--beam', '4'],
                                  ['--lines', '--lexicon', 'w.txt'], ['--lines', '--lexicon', 'w.txt', '--match'], ['--lines', '--lm', 'c.txt'],
                                  ['--lines', '--pattern', 'a+'], ['--lines', '--refine-beams', 'edit'], ['--lines', '--auto-rotate', 'flip'],
                                  ['--lines', '--upright-bias', '0.1'], ['--lines', '--polygons', 'p.txt'], ['--lines', '--line-overlap', '0.8'],
                                  ['--lines', '--line-sep', '-1'], ['--lines', '--line-sep', 'nan'], ['--lines', '--lm-weight', '0.5'],
                                  ['--lines', '--char-bonus', '0.5'], ['--lines', '--refine-iters', '2'], ['--lines', '--priors']])
def test_line_flags_refuse(argv, capsys):
    with pytest.raises(SystemExit):
        _resolve(argv)
