"""CPU tests of lexicon matching: the packed word table of `Lexicon` against the words it entered into the trie, the
class folding map, the CPU restatement (tests/lexicon_match_reference.py) against hand-worked distances, and read.py's refusals."""
import random

import numpy as np
import pytest
import torch

import lexicon_match_reference as MR
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.lexicon import MATCH_DEAD, Lexicon
from parseq_amd.tokenizer import Tokenizer

TOK = Tokenizer(CHARSET_94_FULL)
LOWER = Tokenizer('0123456789abcdefghijklmnopqrstuvwxyz')


def ids_of(tok, word):
    return [tok._stoi[ch] for ch in word]


def trie_words(lex, root=0):
    """{word id: class ids} of every word that ends in the trie below `root`: what the search can finish."""
    out, stack = {}, [(root, [])]
    table = lex.next.numpy()
    while stack:
        node, prefix = stack.pop()
        for c in range(lex.num_classes):
            t = int(table[node, c])
            if t < 0:
                continue
            if c == lex.eos_id:
                out[t] = prefix
            else:
                stack.append((t, prefix + [c]))
    return out


# -------------------------------------------------------------------------------------------------------------------
# the word table
# -------------------------------------------------------------------------------------------------------------------
def test_rows_are_the_entered_words():
    words = ['cat', '', 'dog', 'cat', 'café', 'x' * 26, 'Dog', 'a', 'y' * 25, 'dog']
    lex = Lexicon(words, TOK)
    assert lex.skipped == 3                                   # the empty word, the one outside the charset, the one too long
    entered = trie_words(lex)
    assert sorted(entered) == [0, 2, 6, 7, 8]                 # a repeated word keeps its first id
    rows, ids = lex.rows().numpy(), lex.row_ids.tolist()
    assert rows.shape == (5, 32) and rows.dtype == np.uint8 and lex.num_rows == 5 and lex.rows_nbytes == 160
    assert ids == sorted(entered)
    for r, k in enumerate(ids):
        n = int(rows[r, 31])
        assert n == len(words[k]) and rows[r, :n].tolist() == entered[k] == ids_of(TOK, words[k])
        assert not rows[r, n:31].any()
    assert lex.list_ranges.tolist() == [[0, 5]]
    # the trie and everything else are what they were
    assert lex.words == words and len(lex) == 10 and lex.next.dtype == torch.int32 and lex.table('cpu') is lex.next


def test_rows_under_fold_case_and_longer_labels():
    lex = Lexicon(['Hello', 'hello', 'WORLD', 'z' * 31, 'z' * 32], LOWER, fold_case=True, max_label_length=31)
    assert lex.skipped == 1 and lex.row_ids.tolist() == [0, 2, 3]      # `hello` is `Hello` again
    rows = lex.rows().numpy()
    assert rows[0, :5].tolist() == ids_of(LOWER, 'hello') and rows[0, 31] == 5
    assert rows[2, 31] == 31 and rows[2, :31].tolist() == ids_of(LOWER, 'z') * 31
    with pytest.raises(ValueError, match='31 characters'):
        Lexicon(['ab'], LOWER, max_label_length=32).rows()


def test_forest_ranges():
    lists = [['ab', 'cd', 'ab'], [], ['é', 'ef'], ['gh', 'ij', 'kl']]
    lex, roots = Lexicon.forest(lists, TOK)
    assert lex.row_ids.tolist() == [0, 1, 4, 5, 6, 7]
    assert lex.list_ranges.tolist() == [[0, 2], [2, 2], [2, 3], [3, 6]]
    for (lo, hi), root, first in zip(lex.list_ranges.tolist(), roots.tolist(), (0, 3, 3, 5)):
        assert sorted(trie_words(lex, root)) == lex.row_ids.tolist()[lo:hi]
    assert lex.crop_ranges([3, 1, 0], 3, 'cpu').tolist() == [[3, 6], [2, 2], [0, 2]]
    assert lex.crop_ranges(None, 3, 'cpu') is None
    for bad in ([0, 1], [0, 1, 4], [0, -1, 1]):
        with pytest.raises(ValueError):
            lex.crop_ranges(bad, 3, 'cpu')


def test_random_lists_against_the_trie():
    rng = random.Random(5)
    lists = [[''.join(rng.choice('abC1') for _ in range(rng.randint(0, 4))) for _ in range(rng.randint(0, 40))] for _ in range(6)]
    lex, roots = Lexicon.forest(lists, TOK)
    rows, ids = lex.rows().numpy(), lex.row_ids.tolist()
    assert ids == sorted(ids) and len(set(ids)) == len(ids)
    for (lo, hi), root in zip(lex.list_ranges.tolist(), roots.tolist()):
        entered = trie_words(lex, root)
        assert ids[lo:hi] == sorted(entered)
        for r in range(lo, hi):
            assert rows[r, :rows[r, 31]].tolist() == entered[ids[r]]


# -------------------------------------------------------------------------------------------------------------------
# the folding map
# -------------------------------------------------------------------------------------------------------------------
def test_fold_map_of_a_cased_charset():
    lex = Lexicon(['Hello', 'hello', 'A-1'], TOK)
    fold = lex.fold_map().tolist()
    assert len(fold) == lex.num_classes and fold[lex.eos_id] == lex.eos_id
    for ch, i in TOK._stoi.items():
        if i >= lex.num_classes or i == lex.eos_id:
            continue
        assert fold[i] == TOK._stoi[ch.lower()], ch
    assert fold[TOK._stoi['Q']] == TOK._stoi['q'] and fold[TOK._stoi['q']] == TOK._stoi['q'] and fold[TOK._stoi['7']] == TOK._stoi['7']
    own, folded = lex.rows(False).numpy(), lex.rows(True).numpy()
    assert own[0, :5].tolist() == ids_of(TOK, 'Hello') and folded[0, :5].tolist() == ids_of(TOK, 'hello')
    assert folded[1].tolist() == own[1].tolist() == folded[0].tolist()      # two rows, two ids, one folded spelling
    assert folded[2, :3].tolist() == ids_of(TOK, 'a-1') and (folded[:, 31] == own[:, 31]).all()


def test_fold_map_of_a_single_case_charset():
    lex = Lexicon(['abc'], LOWER)
    assert lex.fold_map().tolist() == list(range(lex.num_classes))
    assert torch.equal(lex.rows(True), lex.rows(False))
    upper = Lexicon(['ABC'], Tokenizer('ABCDEFGH'))
    assert upper.fold_map().tolist() == list(range(upper.num_classes))      # no lower-case class to fold to


def test_encode_readings():
    lex = Lexicon(['abc'], LOWER, fold_case=True)
    tok, lengths = lex.encode_readings(['', 'aBé', 'z' * 32])
    assert tok.shape == (3, 32) and lengths.tolist() == [0, 3, 32]
    assert tok[1, :4].tolist() == [LOWER._stoi['a'], LOWER._stoi['b'], -1, lex.eos_id]
    with pytest.raises(ValueError, match='32'):
        lex.encode_readings(['z' * 33])


# -------------------------------------------------------------------------------------------------------------------
# the restatement
# -------------------------------------------------------------------------------------------------------------------
def _d(a, b):
    ids, lengths = MR.pack([[ord(c) for c in b]])
    return int(MR.distances([ord(c) for c in a], ids, lengths)[0])


def test_reference_distances_by_hand():
    assert _d('', 'abc') == 3 and _d('abc', 'abc') == 0 and _d('a', 'a') == 0
    assert _d('abc', 'abxc') == 1 and _d('abc', 'xabc') == 1 and _d('abc', 'abcx') == 1 and _d('abc', 'xxabcxx') == 4      # insertions
    assert _d('abxc', 'abc') == 1 and _d('abcdef', 'f') == 5 and _d('abc', 'a') == 2                                          # deletions
    assert _d('abc', 'abd') == 1 and _d('abc', 'xyz') == 3 and _d('abc', 'xbz') == 2                                          # substitutions
    assert _d('kitten', 'sitting') == 3 and _d('flaw', 'lawn') == 2 and _d('sunday', 'saturday') == 3
    assert _d('ab', 'ba') == 2                                                                                               # no transposition
    # several words at once, of different lengths
    ids, lengths = MR.pack([[1, 2, 3], [1], [4, 4, 4, 4, 4], [2, 3]])
    assert MR.distances([1, 2, 3], ids, lengths).tolist() == [0, 2, 5, 1]
    assert MR.distances([], ids, lengths).tolist() == [3, 1, 5, 2]


def test_reference_selection():
    words = [[1, 2, 3], [1, 2, 4], [9], [1, 2, 3, 4], [1, 2]]
    wid = [3, 5, 6, 8, 11]
    ids, d = MR.match([[1, 2, 3, 0, 7, 7]], None, words, wid, 3, eos_id=0)
    assert ids == [[3, 5, 8]] and d == [[0, 1, 1]]                            # the reading ends at <eos>; ties: the lower id
    ids, d = MR.match([[1, 2, 3, 5, 7, 7]], [2], words, wid, 7, eos_id=0)
    assert ids == [[11, 3, 5, 6, 8, -1, -1]] and d == [[0, 1, 1, 2, 2, MR.DEAD, MR.DEAD]]
    ids, d = MR.match([[1, 2, 3], [1, 2, 3]], None, words, wid, 2, 0, ranges=[(2, 4), (3, 3)])
    assert ids == [[8, 6], [-1, -1]] and d == [[1, 3], [MR.DEAD, MR.DEAD]]
    ids, d = MR.match([[21, 2, 99]], None, [[1, 2, 3]], [0], 1, 0, fold=[0] + list(range(1, 21)) + list(range(1, 11)))
    assert d == [[1]]                                                          # 21 folds to 1; 99 is no class and matches nothing
    assert MR.DEAD == MATCH_DEAD
    assert MR.candidates([4, 7], [1, 2], False) == [(4, 1, False), (7, 2, False)]
    assert MR.candidates([4, 7], [1, 2], True) == [(-1, 0, True), (4, 1, False), (7, 2, False)]
    assert MR.candidates([4, 7], [0, 2], True) == [(4, 0, False), (7, 2, False), (-1, MR.DEAD, False)]
    assert MR.candidates([-1], [MR.DEAD], True) == [(-1, 0, True), (-1, MR.DEAD, False)]


def test_reference_against_a_recursive_distance():
    import functools
    rng = random.Random(3)

    def lev(a, b):
        @functools.lru_cache(maxsize=None)
        def f(i, j):
            if i == 0 or j == 0:
                return i + j
            return min(f(i - 1, j) + 1, f(i, j - 1) + 1, f(i - 1, j - 1) + (a[i - 1] != b[j - 1]))
        return f(len(a), len(b))
    words = [tuple(rng.randrange(1, 5) for _ in range(rng.randint(1, 9))) for _ in range(60)]
    ids, lengths = MR.pack(words)
    for _ in range(20):
        r = tuple(rng.randrange(1, 5) for _ in range(rng.randint(0, 10)))
        assert MR.distances(r, ids, lengths).tolist() == [lev(r, w) for w in words]


# -------------------------------------------------------------------------------------------------------------------
# refusals that need no device
# -------------------------------------------------------------------------------------------------------------------
def test_python_refusals():
    from parseq_amd.model import check_lexicon_match
    lex = Lexicon(['abc'], TOK)
    check_lexicon_match(16, False, lex, 25, 95)
    check_lexicon_match(15, True, lex, 25, 95)
    for n, keep in ((0, False), (17, False), (16, True), (True, False), (2.0, False)):
        with pytest.raises(ValueError, match='n must be'):
            check_lexicon_match(n, keep, lex, 25, 95)
    with pytest.raises(ValueError, match='classes'):
        check_lexicon_match(4, False, lex, 25, 37)
    with pytest.raises(ValueError, match='characters'):
        check_lexicon_match(4, False, Lexicon(['abc'], TOK, max_label_length=30), 25, 95)
    with pytest.raises(ValueError, match='empty'):
        check_lexicon_match(4, False, Lexicon(['é'], TOK), 25, 95)


def test_read_cli_match_flags():
    pytest.importorskip('PIL.Image')
    import read as read_cli
    parser = read_cli.build_parser()

    def resolve(*argv):
        args, _ = parser.parse_known_args(['pretrained=parseq', '--images', 'a.png', *argv])
        return args, read_cli.resolve_match(parser, args), read_cli.resolve_search(parser, args), read_cli.resolve_refine(parser, args)
    args, match, search, _ = resolve('--lexicon', 'w.txt', '--match')
    assert match == 8 == read_cli.MATCH_N and search[1] == 1
    assert resolve('--lexicon', 'w.txt', '--match', '12', '--nbest', '5')[1:3] == (12, (8, 5))
    assert resolve('--lexicon', 'w.txt', '--match', '--refine-beams', 'score')[1] == 8
    assert resolve('--lexicon', 'w.txt', '--match', '3', '--regions', 'r.txt')[1] == 3
    # without --match, --lexicon is what it was
    assert resolve('--lexicon', 'w.txt')[1:3] == (None, (8, 1)) and resolve('--nbest', '3')[1:3] == (None, (None, 3))
    for argv in (['--match'], ['--match', '4'], ['--lexicon', 'w.txt', '--match', '--beam', '8'], ['--lexicon', 'w.txt', '--match', '--refine-beams', 'edit'],
                 ['--lexicon', 'w.txt', '--match', '0'], ['--lexicon', 'w.txt', '--match', '17'], ['--lexicon', 'w.txt', '--match', '4', '--nbest', '5']):
        with pytest.raises(SystemExit):
            resolve(*argv)
    assert read_cli.match_lines('a.png', [('cat', -1.5, 1), ('cart', -2.25, 2)], False) == ['a.png: cat']
    assert read_cli.match_lines('a.png', [('cat', -1.5, 1), ('cart', -2.25, 12)], True) == ['a.png: cat', '      -1.5000  d=1  cat', '      -2.2500  d=12 cart']
    assert read_cli.match_lines('a.png', [], True) == ['a.png: ']
