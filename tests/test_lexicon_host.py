"""CPU tests of the lexicon-constrained beam search: `parseq_amd.lexicon.Lexicon` against a construction by
prefix sets, the float64 restatement (tests/lexicon_reference.py) that tests/test_lexicon_beam.py compares the device against, read.py's
flags, and the refusals that come before any device work."""
import math
import random

import pytest
import torch

import lexicon_reference as LR
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.lexicon import Lexicon
from parseq_amd.tokenizer import Tokenizer

TOK = Tokenizer(CHARSET_94_FULL)
C94 = len(TOK) - 2


def _random_words(n, seed, alphabet=CHARSET_94_FULL, longest=9):
    rng = random.Random(seed)
    # a small alphabet at the front so that prefixes are shared, the whole charset behind it
    pool = alphabet[:6] * 8 + alphabet
    return [''.join(rng.choice(pool) for _ in range(rng.randint(1, longest))) for _ in range(n)]


def _walk(lex, root, ids):
    n = root
    for c in ids:
        n = int(lex.next[n, c])
        if n < 0:
            return -1
    return n


def _check_against_prefix_sets(lex, root, words, first_id=0):
    """next[n][c] >= 0 exactly where prefix + c is a prefix of some word; the <eos> column holds the first id of the word that ends there.
    Every node of the trie is visited from the root, so the count of nodes is checked too."""
    enc = [(first_id + k, TOK._tok2ids(w)) for k, w in enumerate(words)]
    prefixes, ends = LR.naive_trie(enc, C94, TOK.eos_id)
    seen = set()
    for prefix in prefixes:
        n = _walk(lex, root, prefix)
        assert n >= 0, prefix
        seen.add(n)
        for c in range(C94):
            t = int(lex.next[n, c])
            if c == TOK.eos_id:
                assert t == ends.get(prefix, -1), (prefix, t)
            else:
                assert (t >= 0) == (prefix + (c,) in prefixes), (prefix, c)
                assert t < lex.num_nodes
    assert len(seen) == len(prefixes)
    return seen


def test_table_against_prefix_sets():
    words = _random_words(300, 1)
    assert len(set(words)) < len(words)                       # duplicates among them
    lex = Lexicon(words, TOK)
    assert lex.next.dtype == torch.int32 and lex.next.shape[1] == C94 and lex.skipped == 0 and lex.words == words
    seen = _check_against_prefix_sets(lex, 0, words)
    assert seen == set(range(lex.num_nodes))
    assert lex.nbytes == lex.num_nodes * C94 * 4


def test_breadth_first_numbering_and_determinism():
    words = _random_words(200, 2)
    a, b = Lexicon(words, TOK), Lexicon(list(words), TOK)
    assert torch.equal(a.next, b.next)
    # breadth first, children in ascending class order: read row by row, the child ids are 1, 2, 3, ...
    children = a.next.clone()
    children[:, TOK.eos_id] = -1
    flat = children.flatten()
    assert flat[flat >= 0].tolist() == list(range(1, a.num_nodes))
    # the order of the words decides the ids, not the nodes
    shuffled = list(words)
    random.Random(3).shuffle(shuffled)
    c = Lexicon(shuffled, TOK)
    kids = c.next.clone()
    kids[:, TOK.eos_id] = -1
    assert torch.equal(kids, children)


def test_skips_and_duplicates():
    words = ['cat', '', 'café', 'x' * 26, 'cat', 'car', 'y' * 25, 'Cat']
    lex = Lexicon(words, TOK)
    assert lex.skipped == 3 and lex.words == words and len(lex) == 8
    eos = TOK.eos_id
    assert int(lex.next[_walk(lex, 0, TOK._tok2ids('cat')), eos]) == 0        # the duplicate at 4 keeps id 0
    assert int(lex.next[_walk(lex, 0, TOK._tok2ids('car')), eos]) == 5
    assert int(lex.next[_walk(lex, 0, TOK._tok2ids('Cat')), eos]) == 7        # a cased charset: another word
    assert int(lex.next[_walk(lex, 0, TOK._tok2ids('y' * 25)), eos]) == 6
    assert _walk(lex, 0, TOK._tok2ids('x' * 25)) < 0
    assert int(lex.next[_walk(lex, 0, TOK._tok2ids('ca')), eos]) == -1         # a prefix is not a word
    short = Lexicon(words, TOK, max_label_length=3)
    assert short.skipped == 4
    empty = Lexicon([], TOK)
    assert empty.next.shape == (1, C94) and (empty.next == -1).all()


def test_fold_case():
    lower = Tokenizer('0123456789abcdefghijklmnopqrstuvwxyz')
    words = ['Hello', 'WORLD', 'hello', 'a-b']
    lex = Lexicon(words, lower, fold_case=True)
    assert lex.skipped == 1 and lex.next.shape[1] == 37
    n = 0
    for c in lower._tok2ids('hello'):
        n = int(lex.next[n, c])
    assert int(lex.next[n, lower.eos_id]) == 0 and lex.words[0] == 'Hello'   # entered folded, read back as given; 'hello' is its duplicate
    assert Lexicon(words, lower).skipped == 3                                 # without folding the upper-case words are foreign
    cased = Lexicon(['Hello', 'hello'], TOK, fold_case=True)                  # a charset with both cases: nothing is folded
    assert int(cased.next[_walk(cased, 0, TOK._tok2ids('hello')), TOK.eos_id]) == 1


def test_forest_roots_are_disjoint_tries():
    lists = [_random_words(20, 10 + k) for k in range(4)] + [[]]
    lex, roots = Lexicon.forest(lists, TOK)
    assert roots.dtype == torch.int32 and roots.tolist()[0] == 0 and len(roots) == 5
    assert lex.words == [w for ws in lists for w in ws]
    seen, first = [], 0
    for k, ws in enumerate(lists):
        seen.append(_check_against_prefix_sets(lex, int(roots[k]), ws, first))
        first += len(ws)
    assert sum(len(s) for s in seen) == lex.num_nodes and set().union(*seen) == set(range(lex.num_nodes))
    again, roots2 = Lexicon.forest(lists, TOK)
    assert torch.equal(again.next, lex.next) and torch.equal(roots, roots2)
    # one list through forest is the plain lexicon
    one, r = Lexicon.forest([lists[0]], TOK)
    assert torch.equal(one.next, Lexicon(lists[0], TOK).next) and r.tolist() == [0]


# -------------------------------------------------------------------------------------------------------------------
# the float64 restatement
# -------------------------------------------------------------------------------------------------------------------
SMALL = Tokenizer('abcde')          # classes: <eos> = 0, a .. e = 1 .. 5; <bos> = 6, <pad> = 7


def _made_up_logits(history):
    g = torch.Generator().manual_seed(1 + sum((int(t) + 1) * 11 ** k for k, t in enumerate(history)))
    return torch.randn(6, generator=g, dtype=torch.float64) * 2.0


def _step_logits(h):
    return torch.stack([_made_up_logits(row.tolist()) for row in h])


def _logprob(word):
    hist, total = [SMALL.bos_id], 0.0
    for c in SMALL._tok2ids(word) + [SMALL.eos_id]:
        total += torch.log_softmax(_made_up_logits(hist), -1)[c].item()
        hist.append(c)
    return total


FIVE = ['ab', 'abc', 'b', 'bead', 'ace']


def test_restatement_is_exhaustive_when_the_lexicon_fits_the_beam():
    lex = Lexicon(FIVE, SMALL)
    steps = 6
    got = LR.beam_search(_step_logits, 1, 5, steps, SMALL.bos_id, SMALL.eos_id, SMALL.pad_id, lex.next)
    want = sorted(((_logprob(w), k) for k, w in enumerate(FIVE)), reverse=True)
    assert min(a[0] - b[0] for a, b in zip(want, want[1:])) > 1e-9
    assert got.finished[0].tolist() == [1] * 5
    assert got.words[0].tolist() == [k for _, k in want]
    for r, (score, k) in enumerate(want):
        assert abs(got.scores[0, r].item() - score) < 1e-12
        ids = SMALL._tok2ids(FIVE[k])
        assert got.lengths[0, r].item() == len(ids)
        assert got.tokens[0, r].tolist() == ids + [SMALL.eos_id] + [SMALL.pad_id] * (steps - len(ids) - 1)
    # a narrower beam: a subset of those, same scores
    narrow = LR.beam_search(_step_logits, 1, 2, steps, SMALL.bos_id, SMALL.eos_id, SMALL.pad_id, lex.next)
    scores = {k: s for s, k in want}
    for r in range(2):
        if narrow.finished[0, r]:
            k = int(narrow.words[0, r])
            assert k in scores and abs(narrow.scores[0, r].item() - scores[k]) < 1e-12
        else:
            assert narrow.scores[0, r].item() == -math.inf
    assert narrow.finished[0].sum() >= 1
    # per-image tries through roots
    forest, roots = Lexicon.forest([FIVE[:2], FIVE[2:]], SMALL)
    both = LR.beam_search(_step_logits, 2, 3, steps, SMALL.bos_id, SMALL.eos_id, SMALL.pad_id, forest.next, roots)
    assert sorted(both.words[0].tolist()) == [-1, 0, 1] and sorted(both.words[1].tolist()) == [2, 3, 4]
    assert both.scores[0, 2].item() == -math.inf and both.nodes[0, 2].item() == -1


def test_restatement_word_longer_than_the_steps_stays_unfinished():
    lex = Lexicon(['ab', 'bead'], SMALL)
    got = LR.beam_search(_step_logits, 1, 2, 4, SMALL.bos_id, SMALL.eos_id, SMALL.pad_id, lex.next)     # 4 steps: 3 characters and <eos> at most
    by_word = {int(w): r for r, w in enumerate(got.words[0].tolist())}
    assert set(by_word) == {0, -1}
    r = by_word[-1]
    assert got.finished[0, r].item() == 0 and got.lengths[0, r].item() == 4 and got.tokens[0, r].tolist() == SMALL._tok2ids('bead')
    assert got.finished[0, by_word[0]].item() == 1


def test_restatement_ties_and_guards():
    """Two beams with the same score, row and node: the lower parent first, then the lower class (section 18's rule, with the trie only
    removing candidates).  A child id past the table and a node outside it offer nothing."""
    eos, pad, bos = 0, 7, 6
    table = [[-1, 1, 2, -1, -1, -1], [0, -1, -1, -1, -1, -1], [1, -1, -1, -1, -1, -1]]      # words: class 1, class 2
    row = [0.0, 2.0, 2.0, -1.0, 3.0, 0.5]
    st = LR.step_image(torch.tensor([row, row]), [-1.5, -1.5], [0, 0], [2, 2], [[bos, 1, 2, pad], [bos, 2, 1, pad]], [0, 0], [-1, -1], table, 2, eos, pad)
    assert st.parent == [0, 0] and st.picked == [1, 2] and st.gap == 0.0 and st.nodes == [1, 2] and st.words == [-1, -1]
    st3 = LR.step_image(torch.tensor([row] * 3), [-1.5] * 3, [0] * 3, [2] * 3, [[bos, 1, 2, pad]] * 3, [0, 0, 0], [-1] * 3, table, 2, eos, pad)
    assert st3.parent == [0, 0, 1] and st3.picked == [1, 2, 1]
    # the only exit is <eos>: one candidate, the other slot dead
    st = LR.step_image(torch.tensor([row, row]), [-1.0, -math.inf], [0, 0], [1, 0], [[bos, 2, pad, pad], [bos, pad, pad, pad]], [2, -1], [-1, -1], table, 1, eos, pad)
    assert st.parent == [0, -1] and st.picked == [eos, pad] and st.finished == [1, 0] and st.words == [1, -1] and st.nodes == [2, -1]
    assert st.lengths == [1, 0] and st.scores[1] == -math.inf
    # guards
    bad = [[-1, 1, 9, -1, -1, -1], [0, -1, -1, -1, -1, -1]]                                   # child 9 of a 2-node table
    st = LR.step_image(torch.tensor([row]), [0.0], [0], [0], [[bos, pad]], [0], [-1], bad, 0, eos, pad)
    assert st.picked == [1] and st.nodes == [1]
    st = LR.step_image(torch.tensor([row]), [0.0], [0], [0], [[bos, pad]], [5], [-1], bad, 0, eos, pad)
    assert st.parent == [-1] and st.scores == [-math.inf] and st.nodes == [-1]
    dead = LR.beam_search(lambda h: torch.zeros(h.shape[0], 6), 2, 2, 2, bos, eos, pad, table, [0, 3])
    assert (dead.scores[1] == -math.inf).all() and (dead.tokens[1] == pad).all() and (dead.words[1] == -1).all() and dead.scores[0, 0] > -math.inf


# -------------------------------------------------------------------------------------------------------------------
# read.py and the refusals
# -------------------------------------------------------------------------------------------------------------------
def test_read_cli_flags(tmp_path):
    pytest.importorskip('PIL.Image')
    import read as read_cli
    parser = read_cli.build_parser()

    def resolve(*argv):
        args, _ = parser.parse_known_args(['pretrained=parseq', '--images', 'a.png', *argv])
        return args, read_cli.resolve_search(parser, args)
    args, search = resolve('--lexicon', 'w.txt')
    assert args.lexicon == 'w.txt' and search == (8, 1)
    assert resolve('--lexicon', 'w.txt', '--beam', '4', '--nbest', '3')[1] == (4, 3)
    assert resolve('--lexicon', 'w.txt', '--nbest', '12')[1] == (12, 12)
    assert resolve('--lexicon', 'w.txt', '--beam', '16')[1] == (16, 1)
    args, search = resolve()
    assert args.lexicon is None and search == (None, 0)
    assert resolve('--nbest', '3')[1] == (None, 3)
    for argv in (('--lexicon', 'w.txt', '--beam', '2', '--nbest', '3'), ('--beam', '4'), ('--lexicon',)):
        with pytest.raises(SystemExit):
            resolve(*argv)
    f = tmp_path / 'words.txt'
    f.write_text('cat\n\n  dog \r\nNew York\n')
    assert read_cli.load_word_list(str(f)) == ['cat', 'dog', 'New York']


def test_refusals_before_any_device_work():
    """None of these reaches the library: the models live on the CPU, where any device work would raise a RuntimeError instead."""
    from parseq_amd import create_model
    x = torch.zeros(2, 3, 32, 128)
    m = create_model('parseq-tiny')
    lex = Lexicon(['cat', 'dog'], m.tokenizer)
    with pytest.raises(ValueError, match='beam_width'):
        m.beam_search(x, 17, lexicon=lex)
    with pytest.raises(ValueError, match='beam_width'):
        m.beam_search(x, 0, lexicon=lex)
    wrong = Lexicon(['12', '7'], Tokenizer('0123456789'))
    assert wrong.next.shape[1] == 11
    with pytest.raises(ValueError, match='lexicon table'):
        m.beam_search(x, 4, lexicon=wrong)
    with pytest.raises(ValueError, match='roots'):
        m.beam_search(x, 4, lexicon=lex, roots=torch.zeros(3, dtype=torch.int32))
    with pytest.raises(ValueError, match='roots'):
        m.beam_search(x, 4, roots=torch.zeros(2, dtype=torch.int32))
    deep = create_model('parseq-tiny', dec_depth=2)
    with pytest.raises(ValueError, match='dec_depth'):
        deep.beam_search(x, 4, lexicon=Lexicon(['cat'], deep.tokenizer))
    vit = create_model('vitstr')
    with pytest.raises(ValueError, match='ViTSTR'):
        vit.beam_search(torch.zeros(2, 3, *vit.hparams.img_size), 4, lexicon=Lexicon(['cat'], vit.tokenizer))
    with pytest.raises(ValueError, match='no `words`'):
        from parseq_amd.model import BeamResult
        z = torch.zeros(1, 1, 2, dtype=torch.int32)
        m.tokenizer.decode_beams(BeamResult(z, torch.zeros(1, 1), z[:, :, 0], z[:, :, 0].to(torch.uint8)), lex)
