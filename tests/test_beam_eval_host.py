"""Host tests of N-best evaluation: the CPU restatement (tests/beam_eval_reference.py) against a brute-force statement
of the definitions on hand-written cases, the synthetic cases' coverage, `BeamEvalResult`, test.py's flags, refusals and tables, and the flag
resolution read.py shares with it."""
import importlib.util
import io
import math
import multiprocessing as mp
import os
import socket

import numpy as np
import pytest

import beam_eval_reference as R
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.tokenizer import CharsetAdapter, Tokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float('-inf')
LOWER_36 = '0123456789abcdefghijklmnopqrstuvwxyz'


def load_script(name, path):
    spec = importlib.util.spec_from_file_location(name, os.path.join(ROOT, path))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def dp_distance(a, b):
    """Full-table Levenshtein distance, the slow obvious way."""
    d = [[0] * (len(b) + 1) for _ in range(len(a) + 1)]
    for i in range(len(a) + 1):
        d[i][0] = i
    for j in range(len(b) + 1):
        d[0][j] = j
    for i in range(1, len(a) + 1):
        for j in range(1, len(b) + 1):
            d[i][j] = min(d[i - 1][j] + 1, d[i][j - 1] + 1, d[i - 1][j - 1] + (a[i - 1] != b[j - 1]))
    return d[len(a)][len(b)]


def brute_force(tokens, scores, lengths, confs, labels, tok, keep, fold):
    """The definitions once more, image by image, with nothing shared with the restatement: characters as code points, the adapter as a
    per-character rule (`fold` then membership in `keep`), the full-table distance."""
    classes = len(tok) - 2
    totals = dict(num_samples=0, correct=0, label_length=0, top1_distance=0, oracle_correct=0, oracle_distance=0, live=0, miss=0, ned=0.0, confidence=0.0,
                  oracle_ned=0.0)
    first_hit = [0] * 17
    for rows, row_scores, row_lengths, row_confs, label in zip(tokens, scores, lengths, confs, labels):
        gt = [ord(c) for c in label]
        seen = []                                                      # (m, distance, ned, confidence) of the live hypotheses, in slot order
        for ids, score, length, conf in zip(rows, row_scores, row_lengths, row_confs):
            if score == NEG_INF:
                continue
            chars = [fold(tok._itos[i]) for i in ids[:min(max(length, 0), len(ids), 32)] if 1 <= i < classes]
            pred = [ord(c) for c in chars if c in keep]
            d = dp_distance(pred, gt)
            seen.append((len(pred), d, d / max(len(pred), len(gt), 1), conf))
        totals['num_samples'] += 1
        totals['live'] += len(seen)
        if not seen:
            seen = [(0, len(gt), len(gt) / max(len(gt), 1), NEG_INF)]      # the empty reading; exp(-inf) = 0
            hits = []
        else:
            hits = [k for k, s in enumerate(seen) if s[1] == 0]
        totals['correct'] += int(bool(hits) and hits[0] == 0)
        totals['label_length'] += seen[0][0]
        totals['top1_distance'] += seen[0][1]
        totals['ned'] += seen[0][2]
        totals['confidence'] += math.exp(seen[0][3])
        totals['oracle_distance'] += min(s[1] for s in seen)
        totals['oracle_ned'] += min(s[2] for s in seen)
        totals['oracle_correct'] += int(bool(hits))
        totals['miss'] += int(not hits)
        if hits:
            first_hit[hits[0]] += 1
    return totals, first_hit


def hand_case():
    """Hand-written images over the 94-character tokenizer, test charset 0-9a-z, W = 4, T = 6."""
    tok = Tokenizer(CHARSET_94_FULL)
    pad, T = tok.pad_id, 6
    ids = lambda text, fill=pad: (tok._tok2ids(text) + [fill] * T)[:T]
    dead = ([pad] * T, NEG_INF, 0, NEG_INF)
    images = [
        # exact at rank 0, 1, 2, 3
        ('cat', [(ids('cat'), -0.1, 3, -0.1), (ids('cab'), -0.5, 3, -0.5), (ids('ca'), -0.9, 2, -0.9), (ids('bat'), -1.5, 3, -1.5)]),
        ('cat', [(ids('cab'), -0.1, 3, -0.1), (ids('cat'), -0.5, 3, -0.5), (ids('ca'), -0.9, 2, -0.9), (ids('bat'), -1.5, 3, -1.5)]),
        ('cat', [(ids('cab'), -0.1, 3, -0.1), (ids('ca'), -0.5, 2, -0.5), (ids('cat'), -0.9, 3, -0.9), (ids('bat'), -1.5, 3, -1.5)]),
        ('cat', [(ids('cab'), -0.1, 3, -0.1), (ids('ca'), -0.5, 2, -0.5), (ids('bat'), -0.9, 3, -0.9), (ids('cat'), -1.5, 3, -1.5)]),
        # none exact
        ('horse', [(ids('house'), -0.2, 5, -0.2), (ids('hose'), -0.4, 4, -0.4), (ids('h'), -0.6, 1, -0.6), (ids('mouse'), -2.0, 5, -2.0)]),
        # a dead slot in the middle (the exact one stands at live rank 1, slot 2) and at the end
        ('dog', [(ids('dig'), -0.3, 3, -0.3), dead, (ids('dog'), -0.7, 3, -0.7), dead]),
        # a dead first slot whose tokens spell the label: the top-1 is slot 1
        ('dog', [(ids('dog'), NEG_INF, 3, -0.1), (ids('dug'), -0.7, 3, -0.7), dead, dead]),
        # every slot dead
        ('bird', [dead, dead, dead, dead]),
        # two hypotheses equal after lower-casing: the first of them is the hit
        ('abc', [(ids('xbc'), -0.1, 3, -0.1), (ids('ABC'), -0.2, 3, -0.2), (ids('abc'), -0.3, 3, -0.3), (ids('aBc'), -0.4, 3, -0.4)]),
        # a live hypothesis of length 0 first (tokens after the length are not read), then the label
        ('a', [(ids('', tok._stoi['a']), -0.1, 0, -0.1), (ids('a'), -0.2, 1, -0.2), (ids('a'), -0.3, -2, -0.3), (ids('ab'), -0.4, 9, -0.4)]),
        # punctuation only: the adapter drops every character
        ('ok', [(ids('!?'), -0.1, 2, -0.1), (ids('o!k'), -0.2, 3, -0.2), (ids('#'), -0.3, 1, -0.3), (ids('ok!?'), -0.4, 4, -0.4)]),
        # ids outside the classes (<bos>, <pad>, beyond, negative) and <eos> inside the length
        ('no', [([tok.bos_id, tok._stoi['n'], 999, tok._stoi['o'], -3, tok.eos_id], -0.1, 6, -0.1), dead, dead, dead]),
    ]
    labels = [label for label, _ in images]
    cols = [[[slot[k] for slot in slots] for _, slots in images] for k in range(4)]
    return tok, cols[0], cols[1], cols[2], cols[3], labels


def test_restatement_equals_brute_force_on_hand_written_cases():
    tok, tokens, scores, lengths, confs, labels = hand_case()
    adapter = CharsetAdapter(LOWER_36)
    got = R.evaluate(tokens, scores, lengths, confs, labels, tok, adapter)
    totals, first_hit = brute_force(tokens, scores, lengths, confs, labels, tok, set(LOWER_36), str.lower)
    for k in R.INT_NAMES:
        assert got['totals'][k] == totals[k], k
    for k in R.FLOAT_NAMES:
        assert got['totals'][k] == pytest.approx(totals[k], rel=1e-14), k
    assert got['first_hit'] == first_hit
    # and what the cases were written to show
    rows = got['image_rows']
    assert [r[4] for r in rows] == [0, 1, 2, 3, -1, 1, -1, -1, 1, 1, 1, 0]
    assert first_hit[:4] == [2, 5, 1, 1] and totals['miss'] == 3 and totals['correct'] == 2
    assert rows[5][6:] == [2, 0] and rows[6][6:] == [1, 1] and rows[6][:4] == [3, 3, 1, 0]         # dead slots: live counts and top-1 slots
    assert rows[7] == [0, 4, 4, 0, -1, 4, 0, -1] and got['image_ned'][7] == 1.0 and got['image_confidence'][7] == 0.0
    assert rows[9][:4] == [0, 1, 1, 0] and got['hyp_rows'][9 * 4 + 2] == [0, 1, 1, 0] and got['hyp_rows'][9 * 4 + 3] == [2, 1, 1, 0]
    assert rows[10][:4] == [0, 2, 2, 0] and got['hyp_rows'][10 * 4 + 2] == [0, 2, 2, 0]
    assert rows[11][:4] == [2, 2, 0, 1]
    assert got['hyp_rows'][5 * 4 + 1] == [-1, -1, -1, 0] and got['hyp_ned'][5 * 4 + 1] == -1.0
    assert rows[4][5] == 1 and rows[4][2] == 1 and got['image_oracle_ned'][4] == 1 / 5 and got['hyp_rows'][4 * 4 + 2] == [1, 5, 4, 0]


def test_an_adapter_that_drops_every_character():
    tok, tokens, scores, lengths, confs, labels = hand_case()
    got = R.evaluate(tokens, scores, lengths, confs, labels, tok, CharsetAdapter('%'))
    totals, first_hit = brute_force(tokens, scores, lengths, confs, labels, tok, set('%'), lambda c: c)
    assert got['totals']['label_length'] == 0 == totals['label_length'] and got['totals']['miss'] == len(labels) and first_hit == [0] * 17
    assert got['totals']['top1_distance'] == sum(map(len, labels)) == totals['top1_distance'] == got['totals']['oracle_distance']
    assert got['totals']['ned'] == float(len(labels))


def charsets(C):
    if C == 37:
        test = ''.join(c for c in R.CHARSET_36 if c not in R.DROPPED_36)
        return Tokenizer(R.CHARSET_36), CharsetAdapter(test), test, (set(test), lambda c: c)
    return Tokenizer(CHARSET_94_FULL), CharsetAdapter(R.CHARSET_36), R.CHARSET_36, (set(R.CHARSET_36), str.lower)


@pytest.mark.parametrize('B,W,T,G,C', [(5, 1, 26, 64, 37), (257, 2, 26, 25, 37), (40, 16, 26, 65, 95), (40, 17, 32, 256, 37)])
def test_synthetic_cases_cover_what_they_promise(B, W, T, G, C):
    """The generator of the GPU test's inputs: the restatement, the brute force and the evaluator's own host path agree on it, and for
    W >= 2 the rank coverage and every row kind are there."""
    from parseq_amd.evaluate import host_beam_metrics
    tok, adapter, test, (keep, fold) = charsets(C)
    case = R.synthetic_case(B, W, T, G, tok, test, np.random.default_rng(B * 1000 + W * 10 + T))
    got = R.evaluate(*case, tok, adapter)
    totals, first_hit = brute_force(*case, tok, keep, fold)
    assert [got['totals'][k] for k in R.INT_NAMES] == [totals[k] for k in R.INT_NAMES] and got['first_hit'] == first_hit
    for k in R.FLOAT_NAMES:
        assert got['totals'][k] == pytest.approx(totals[k], rel=1e-12)
    if W >= 2:
        assert R.coverage_holds(got, W) and R.kinds_present(case, got, tok, adapter)
    tokens, scores, lengths, confs, labels = case
    slots = [[None if s == NEG_INF else (R.hypothesis_string(ids, k, T, tok, adapter), c) for ids, s, k, c in zip(*image)]
             for image in zip(tokens, scores, lengths, confs)]
    hyp_rows, image_rows, r = host_beam_metrics(slots, labels)
    assert hyp_rows == got['hyp_rows'] and image_rows == got['image_rows'] and list(r.first_hit) == got['first_hit']
    assert (r.num_samples, r.correct, r.label_length_sum, r.top1_distance, r.oracle_correct, r.oracle_distance, r.live, r.miss) == tuple(
        got['totals'][k] for k in R.INT_NAMES)
    assert r.ned_sum == pytest.approx(got['totals']['ned'], rel=1e-12) and r.oracle_ned_sum == pytest.approx(got['totals']['oracle_ned'], rel=1e-12)
    assert r.confidence_sum == pytest.approx(got['totals']['confidence'], rel=1e-12)


def test_derived_properties_from_given_sums():
    from parseq_amd.evaluate import MAX_BEAMS, BeamEvalResult
    hits = (4, 2, 1, 0, 1) + (0,) * (MAX_BEAMS - 5)
    r = BeamEvalResult(num_samples=10, correct=4, label_length_sum=57, top1_distance=13, oracle_correct=8, oracle_distance=3, live=46, miss=2,
                       first_hit=hits, ned_sum=2.5, confidence_sum=6.25, oracle_ned_sum=0.5)
    assert r.accuracy == 0.4 and r.ned == 0.25 and r.confidence == 0.625 and r.label_length == 5.7
    assert [r.hit_at(k) for k in (0, 1, 2, 3, 4, 5, 17, 99)] == [0.0, 0.4, 0.6, 0.7, 0.7, 0.8, 0.8, 0.8]
    assert r.oracle_accuracy == 0.8 == r.hit_at(MAX_BEAMS) and r.oracle_ned == 0.05
    assert r.mrr == pytest.approx((4 + 2 / 2 + 1 / 3 + 1 / 5) / 10, rel=1e-15)
    empty = BeamEvalResult()
    assert (empty.accuracy, empty.ned, empty.confidence, empty.label_length, empty.hit_at(5), empty.oracle_accuracy, empty.mrr) == (0.0,) * 7
    ints, floats = r._words()
    assert len(ints) == 8 + MAX_BEAMS and BeamEvalResult._from_words(ints, floats) == r


def test_evaluator_needs_the_device():
    from parseq_amd import create_model
    from parseq_amd.evaluate import BeamEvaluator
    with pytest.raises(RuntimeError, match='GPU'):
        BeamEvaluator(create_model('parseq-tiny'))


# -------------------------------------------------------------------------------------------------------------------
# the command lines
# -------------------------------------------------------------------------------------------------------------------
def evaluation_parser():
    import argparse
    from parseq_amd.search_flags import add_evaluation_flags
    parser = argparse.ArgumentParser()
    add_evaluation_flags(parser)
    return parser


def resolved(argv):
    from parseq_amd.search_flags import evaluation_width, resolve_evaluation_flags
    parser = evaluation_parser()
    flags = resolve_evaluation_flags(parser, parser.parse_args(argv))
    return None if flags is None else tuple(flags) + (evaluation_width(flags),)


def test_evaluation_flags_resolve_as_read_py_resolves_them():
    # (kind, alpha, beta, match, beam, nbest, refine, refine_iters, W of the table)
    assert resolved([]) is None
    assert resolved(['--beam', '5']) == (None, 1.0, 0.0, None, 5, 5, None, 1, 5)
    assert resolved(['--lexicon', 'w.txt']) == (None, 1.0, 0.0, None, 8, 1, None, 1, 8)
    assert resolved(['--lexicon', 'w.txt', '--beam', '3']) == (None, 1.0, 0.0, None, 3, 3, None, 1, 3)
    assert resolved(['--lexicon', 'w.txt', '--match']) == (None, 1.0, 0.0, 8, 8, 1, None, 1, 8)
    assert resolved(['--lexicon', 'w.txt', '--match', '4']) == (None, 1.0, 0.0, 4, 8, 1, None, 1, 4)
    assert resolved(['--lexicon', 'w.txt', '--priors', '--lm-weight', '0.5', '--beam', '6']) == ('priors', 0.5, 0.0, None, 6, 6, None, 1, 6)
    assert resolved(['--lm', 'c.txt', '--lm-order', '2', '--char-bonus', '0.25']) == ('lm', 1.0, 0.25, None, 8, 1, None, 1, 8)
    assert resolved(['--pattern', '[A-Z]{2}']) == ('pattern', 1.0, 0.0, None, 8, 1, None, 1, 8)
    assert resolved(['--beam', '5', '--refine-beams', 'edit', '--refine-iters', '2']) == (None, 1.0, 0.0, None, 5, 5, 'edit', 2, 5)
    assert resolved(['--lexicon', 'w.txt', '--refine-beams', 'score']) == (None, 1.0, 0.0, None, 8, 1, 'score', 1, 8)


@pytest.mark.parametrize('argv,message', [
    (['--priors'], '--priors needs --lexicon'),
    (['--lm', 'c.txt', '--pattern', 'a'], 'one automaton each'),
    (['--lm-order', '3'], '--lm-order needs --lm'),
    (['--lm', 'c.txt', '--lm-order', '5'], r'--lm-order must be in \[1, 4\]'),
    (['--lm-weight', '0.5', '--beam', '3'], 'need --priors, --lm or --pattern'),
    (['--lm', 'c.txt', '--lexicon', 'w.txt'], 'the search walks one table'),
    (['--lm', 'c.txt', '--refine-beams', 'score'], 'refinement under a weighted automaton'),
    (['--lm', 'c.txt', '--lm-weight', 'nan'], 'must be finite'),
    (['--match', '4'], '--match needs --lexicon'),
    (['--lexicon', 'w.txt', '--match', '4', '--beam', '5'], 'not with --beam'),
    (['--lexicon', 'w.txt', '--match', '17'], r'must be in \[1, 16\]'),
    (['--lexicon', 'w.txt', '--match', '--refine-beams', 'edit'], 'an edited reading can leave the list'),
    (['--refine-beams', 'score'], '--refine-beams needs --beam W or --lexicon FILE'),
    (['--refine-iters', '2'], '--refine-iters needs --refine-beams'),
    (['--beam', '5', '--refine-beams', 'score', '--refine-iters', '2'], 'runs once'),
    (['--lexicon', 'w.txt', '--refine-beams', 'edit'], 'not allowed with --lexicon'),
    (['--beam', '0'], '--beam must be at least 1'),
    (['--lm', 'c.txt', '--beam', '0'], '--beam must be at least 1'),
    (['--lexicon', 'w.txt', '--beam', '-3'], '--beam must be at least 1'),
])
def test_test_py_refuses_what_read_py_refuses(argv, message, capsys):
    cli = load_script('parseq_test_cli_host', 'test.py')
    with pytest.raises(SystemExit) as e:
        cli.main(['no-such.ckpt'] + argv)                  # the refusal comes before the checkpoint is looked at
    assert e.value.code == 2
    import re
    assert re.search(message, capsys.readouterr().err)


PARENT_TABLE = ('| Dataset            | # samples | Accuracy | 1 - NED | Confidence | Label Length |\n'
                '|:------------------:|----------:|---------:|--------:|-----------:|-------------:|\n'
                '| IIIT5k             |      3000 |    98.93 |   99.56 |      97.20 |         5.09 |\n'
                '| a-much-longer-name |         7 |     0.00 |   12.50 |      33.33 |        11.00 |\n'
                '| empty              |         0 |     0.00 |    0.00 |       0.00 |         0.00 |\n'
                '|--------------------|-----------|----------|---------|------------|--------------|\n'
                '| Combined           |      3007 |    98.70 |   99.36 |      97.05 |         5.10 |\n')


def test_the_default_table_is_the_parents():
    """`PARENT_TABLE` is what `print_results_table` printed for these rows before test.py knew a search flag."""
    cli = load_script('parseq_test_cli_host', 'test.py')
    out = io.StringIO()
    cli.print_results_table([cli.Result('IIIT5k', 3000, 98.934, 99.5612, 97.201, 5.089), cli.Result('a-much-longer-name', 7, 0.0, 12.5, 33.333333, 11.0),
                             cli.Result('empty', 0, 0.0, 0.0, 0.0, 0.0)], out)
    assert out.getvalue() == PARENT_TABLE


def test_the_extended_table():
    cli = load_script('parseq_test_cli_host', 'test.py')
    out = io.StringIO()
    cli.print_beam_results_table([cli.BeamTableResult('IIIT5k', 3000, 98.934, 99.5612, 97.201, 5.089, 100.0, 99.6, 0.98765),
                                  cli.BeamTableResult('svt', 1000, 50.0, 60.0, 70.0, 6.5, 80.0, 90.0, 0.625)], 5, out)
    assert out.getvalue() == (
        '| Dataset  | # samples | Accuracy | 1 - NED | Confidence | Label Length |  Hit@5 | Oracle 1 - NED |    MRR |\n'
        '|:--------:|----------:|---------:|--------:|-----------:|-------------:|-------:|---------------:|-------:|\n'
        '| IIIT5k   |      3000 |    98.93 |   99.56 |      97.20 |         5.09 | 100.00 |          99.60 | 0.9877 |\n'
        '| svt      |      1000 |    50.00 |   60.00 |      70.00 |         6.50 |  80.00 |          90.00 | 0.6250 |\n'
        '|----------|-----------|----------|---------|------------|--------------|--------|----------------|--------|\n'
        '| Combined |      4000 |    86.70 |   89.67 |      90.40 |         5.44 |  95.00 |          97.20 | 0.8970 |\n')
    out = io.StringIO()
    cli.print_beam_results_table([cli.BeamTableResult('a', 0, 0.0, 0.0, 0.0, 0.0)], 17, out)
    assert 'Hit@17' in out.getvalue().splitlines()[0] and out.getvalue().splitlines()[-1].split('|')[2].strip() == '0'


# what read.py's main resolved for these command lines before the resolution moved into parseq_amd/search_flags.py:
# (kind, alpha, beta, match, beam, nbest, refine, refine_iters)
READ_PY_BEFORE = [
    (['--images', 'a'], (None, 1.0, 0.0, None, None, 0, None, 1)),
    (['--nbest', '5'], (None, 1.0, 0.0, None, None, 5, None, 1)),
    (['--nbest', '3', '--beam', '8'], (None, 1.0, 0.0, None, 8, 3, None, 1)),
    (['--lexicon', 'w.txt'], (None, 1.0, 0.0, None, 8, 1, None, 1)),
    (['--lexicon', 'w.txt', '--nbest', '3', '--beam', '12'], (None, 1.0, 0.0, None, 12, 3, None, 1)),
    (['--lexicon', 'w.txt', '--match'], (None, 1.0, 0.0, 8, 8, 1, None, 1)),
    (['--lexicon', 'w.txt', '--match', '4', '--nbest', '2'], (None, 1.0, 0.0, 4, 8, 2, None, 1)),
    (['--lexicon', 'w.txt', '--priors', '--lm-weight', '0.5'], ('priors', 0.5, 0.0, None, 8, 1, None, 1)),
    (['--lm', 'c.txt', '--lm-order', '2', '--char-bonus', '0.25', '--nbest', '2'], ('lm', 1.0, 0.25, None, 8, 2, None, 1)),
    (['--pattern', '[A-Z]{2}'], ('pattern', 1.0, 0.0, None, 8, 1, None, 1)),
    (['--nbest', '5', '--refine-beams', 'edit', '--refine-iters', '2'], (None, 1.0, 0.0, None, None, 5, 'edit', 2)),
    (['--lexicon', 'w.txt', '--refine-beams', 'score'], (None, 1.0, 0.0, None, 8, 1, 'score', 1)),
]


@pytest.mark.parametrize('argv,want', READ_PY_BEFORE)
def test_the_shared_resolution_gives_read_py_what_it_built_before(argv, want):
    read_cli = load_script('parseq_read_cli_host', 'read.py')
    from parseq_amd import search_flags
    parser = read_cli.build_parser()
    args, _ = parser.parse_known_args(['x'] + argv)
    assert tuple(search_flags.resolve_flags(parser, args)) == want
    assert read_cli.resolve_flags is search_flags.resolve_flags and read_cli.resolve_search is search_flags.resolve_search
    assert (read_cli.LEXICON_BEAM, read_cli.MATCH_N, read_cli.LM_ORDER) == (8, 8, 3)


def test_read_py_keeps_its_refusal_wording(capsys):
    read_cli = load_script('parseq_read_cli_host', 'read.py')
    with pytest.raises(SystemExit):
        read_cli.main(['x', '--refine-beams', 'score'])
    assert '--refine-beams needs --nbest N or --lexicon FILE' in capsys.readouterr().err


def test_tuner_grid_arguments_and_choice():
    tuner = load_script('parseq_tune_fusion_host', 'tools/tune_fusion.py')
    assert tuner.parse_range('0:1:3') == [0.0, 0.5, 1.0] and tuner.parse_range('0.3:9:1') == [0.3]
    import argparse
    for bad in ('1:2', 'a:b:c', '0:1:0'):
        with pytest.raises(argparse.ArgumentTypeError):
            tuner.parse_range(bad)
    pts = [dict(alpha=a, beta=b, accuracy=acc, ned=ned) for a, b, acc, ned in ((1.0, 0.0, 50.0, 70.0), (0.5, 0.5, 50.0, 70.0), (0.5, 0.0, 50.0, 70.0),
                                                                                (0.0, 0.0, 50.0, 60.0), (0.0, 0.5, 40.0, 99.0))]
    assert tuner.choose(pts) == pts[2] and tuner.choose(pts[:2]) == pts[1] and tuner.choose(pts[3:]) == pts[3]
    with pytest.raises(SystemExit):
        tuner.main(['no-such.ckpt', '--alphas', '0:1:2', '--betas', '0:1:2', '--beam', '3'])          # no automaton to weigh


def _reduce_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ['MASTER_ADDR'], os.environ['MASTER_PORT'] = '127.0.0.1', str(port)
    dist.init_process_group('gloo', rank=rank, world_size=world)
    try:
        from parseq_amd.evaluate import MAX_BEAMS, BeamEvalResult, reduce_beam_result
        tail = (0,) * (MAX_BEAMS - 3)
        mine = [BeamEvalResult(10, 4, 57, 13, 8, 3, 46, 2, (4, 3, 1) + tail, 2.5, 6.25, 0.5),
                BeamEvalResult(6, 6, 30, 0, 6, 0, 30, 0, (6, 0, 0) + tail, 0.0, 5.75, 0.0)][rank]
        r = reduce_beam_result(mine)
        q.put((rank, r._words(), r.accuracy, r.hit_at(2), r.mrr))
    finally:
        dist.destroy_process_group()


def test_two_rank_gloo_reduce_of_the_beam_totals():
    """`BeamEvaluator.reduce` is `reduce_beam_result(self.result(), group)`: every rank ends with the sums of all ranks."""
    with socket.socket() as sk:
        sk.bind(('127.0.0.1', 0))
        port = sk.getsockname()[1]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    procs = [ctx.Process(target=_reduce_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    for _, (ints, floats), accuracy, hit2, mrr in got:
        assert ints == [16, 10, 87, 13, 14, 3, 76, 2, 10, 3, 1] + [0] * 14 and floats == [2.5, 12.0, 0.5]
        assert accuracy == 10 / 16 and hit2 == 13 / 16 and mrr == pytest.approx((10 + 3 / 2 + 1 / 3) / 16, rel=1e-15)
