"""CPU tests of the host builders of weighted automata (parseq_amd/automaton.py): the weighted trie, the character
n-gram model, the regular subset and the stacking, each against a restatement written here from the definition, and read.py's refusals."""
import math
import random
import re

import numpy as np
import pytest
import torch

from parseq_amd.automaton import Automaton
from parseq_amd.configs import CHARSET_94_FULL
from parseq_amd.lexicon import Lexicon
from parseq_amd.tokenizer import Tokenizer

TOK = Tokenizer(CHARSET_94_FULL)
SMALL = Tokenizer('abc01_-')        # the charset of the pattern tests: letters, digits, a word sign and one that is no word character


def _logsumexp(row):
    row = row[np.isfinite(row)]
    return math.log(np.exp(row - row.max()).sum()) + row.max() if row.size else -math.inf


# ---- from_lexicon ------------------------------------------------------------------------------------------------------
def _lexicon_words(seed=3, n=60):
    rng = random.Random(seed)
    pool = CHARSET_94_FULL[:6] * 5 + CHARSET_94_FULL
    words = [''.join(rng.choice(pool) for _ in range(rng.randint(1, 7))) for _ in range(n)]
    words += [words[4], words[9][:2], 'café', '']          # a repeat, a prefix of a word, two words the trie skips
    counts = [float(rng.randint(0, 500)) for _ in words]
    return words, counts


@pytest.mark.parametrize('smoothing', [1.0, 0.5, 0.0])
def test_from_lexicon_is_the_trie_with_relative_frequencies(smoothing):
    words, counts = _lexicon_words()
    aut = Automaton.from_lexicon(words, counts, TOK, smoothing=smoothing)
    lex = Lexicon(words, TOK)
    assert torch.equal(aut.next, lex.next) and aut.words == words and aut.skipped == lex.skipped == 2
    assert aut.weight.dtype == torch.float32 and aut.weight.shape == aut.next.shape and aut.nbytes == lex.nbytes * 2
    # the mass of a spelling: the counts of every word that spells it, and one smoothing
    mass = {}
    for w, c in zip(words, counts):
        if lex.encode_word(w) is not None:
            mass[w] = mass.get(w, smoothing) + c
    total = sum(mass.values())
    for w, m in mass.items():
        tag, path, _ = aut.walk(TOK._tok2ids(w))
        if m == 0:
            assert tag == -1
            continue
        assert words[tag] == w and tag == words.index(w)
        assert abs(path - math.log(m / total)) <= 1e-12, (w, path, math.log(m / total))
    # every state's outgoing mass is 1 (a state all of whose words have mass 0 is unreachable: its row is all -inf)
    for s in range(aut.num_states):
        lse = _logsumexp(aut.weight64[s])
        assert abs(lse) <= 1e-12 or (smoothing == 0.0 and lse == -math.inf)
    # where the trie has no arc the weight is not finite
    assert not np.isfinite(aut.weight64[aut.next.numpy() < 0]).any()
    assert torch.equal(aut.weight, torch.from_numpy(aut.weight64.astype(np.float32)))


def test_from_lexicon_folds_case_and_refuses_nonsense():
    tok = Tokenizer('abcdefghijklmnopqrstuvwxyz')
    aut = Automaton.from_lexicon(['The', 'the', 'Then'], [3, 5, 1], tok, fold_case=True, smoothing=1.0)
    tag, path, _ = aut.walk(tok._tok2ids('the'))
    assert aut.words[tag] == 'The' and abs(path - math.log(9 / 11)) <= 1e-12
    with pytest.raises(ValueError, match='counts'):
        Automaton.from_lexicon(['a', 'b'], [1], tok)
    with pytest.raises(ValueError, match='finite'):
        Automaton.from_lexicon(['a'], [-1], tok)


# ---- ngram ---------------------------------------------------------------------------------------------------------------
CORPUS = ['abba', 'abc', 'cab', 'a', '', 'bcb', 'abab']      # seven sequences, small enough to do by hand
NG = Tokenizer('abc')
BOS = -1


def _ngram_counts(corpus, order, tok):
    """n(h, c) by the definition: every position of every sequence start .. <eos>, every context length below `order`."""
    n = {}
    for text in corpus:
        ids = tok._tok2ids(text)
        hist = [BOS] + ids
        for i, c in enumerate(ids + [tok.eos_id]):
            for k in range(order):
                if k <= i + 1:
                    h = tuple(hist[i + 1 - k:i + 1])
                    n.setdefault(h, {}).setdefault(c, 0)
                    n[h][c] += 1
    return n


def _witten_bell(n, h, c, C):
    """P(c | h) = (n(h, c) + T(h) P(c | h')) / (n(h) + T(h)), uniform below the empty context: the formula, recursively."""
    lower = 1.0 / C if not h else _witten_bell(n, h[1:], c, C)
    seen = n.get(h, {})
    return (seen.get(c, 0) + len(seen) * lower) / (sum(seen.values()) + len(seen))


@pytest.mark.parametrize('order', [1, 2, 3, 4])
def test_ngram_rows_successors_and_probabilities(order):
    aut = Automaton.ngram(CORPUS, order, NG)
    C, eos = 4, NG.eos_id
    n = _ngram_counts(CORPUS, order, NG)
    states = aut.contexts
    assert states[0] == (BOS,) and states[1] == () and len(set(states)) == len(states) == aut.num_states
    assert set(states) == set(n) | {(BOS,), ()}                  # the empty context, every context seen, the start
    if order == 1:
        assert aut.num_states == 2
    index = {h: s for s, h in enumerate(states)}
    for s, h in enumerate(states):
        assert abs(_logsumexp(aut.weight64[s])) <= 1e-12
        ctx = () if order == 1 else h                             # (a unigram's start predicts as the empty context)
        for c in range(C):
            assert abs(aut.weight64[s, c] - math.log(_witten_bell(n, ctx, c, C))) <= 1e-12, (h, c)
            if c == eos:
                assert aut.next[s, c] == 0
                continue
            hc = (h + (c,))[-(order - 1):] if order > 1 else ()
            want = next(index[hc[k:]] for k in range(len(hc) + 1) if hc[k:] in index)      # brute force: the longest suffix that is a state
            assert aut.next[s, c] == want, (h, c)
    # by hand, order 2: P(b | a) from what follows every 'a' of the corpus and the unigram counts, both read off the strings directly
    if order == 2:
        a, b = NG._tok2ids('ab')
        after_a = [t[i + 1] if i + 1 < len(t) else None for t in CORPUS for i, ch in enumerate(t) if ch == 'a']
        n_ab, n_a, distinct = after_a.count('b'), len(after_a), len(set(after_a))
        uni = [ch for t in CORPUS for ch in t] + [None] * len(CORPUS)
        p_b = (uni.count('b') + len(set(uni)) / C) / (len(uni) + len(set(uni)))
        assert abs(math.exp(aut.weight64[index[(a,)], b]) - (n_ab + distinct * p_b) / (n_a + distinct)) <= 1e-12
    # a whole sequence's weight is the sum of its conditional log-probabilities
    tag, path, _ = aut.walk(NG._tok2ids('abba'))
    ids = NG._tok2ids('abba') + [eos]
    hist = [BOS] + ids
    want = sum(math.log(_witten_bell(n, tuple(hist[max(0, i + 2 - order):i + 1]) if order > 1 else (), c, C)) for i, c in enumerate(ids))
    assert tag == 0 and abs(path - want) <= 1e-12


def test_ngram_sizes_and_refusals():
    with pytest.raises(ValueError, match='order'):
        Automaton.ngram(CORPUS, 5, NG)
    with pytest.raises(ValueError, match='order'):
        Automaton.ngram(CORPUS, 0, NG)
    with pytest.raises(ValueError, match='no text'):
        Automaton.ngram(['é'], 2, NG)
    assert Automaton.ngram(['ab', 'aé'], 2, NG).skipped == 1
    with pytest.raises(ValueError, match=r'\d+ bytes'):
        Automaton.ngram(CORPUS, 3, NG, max_bytes=64)
    # the documented size: every pair of the 94 characters seen -> 1 + 94 + 94 * 94 contexts and the start contexts, 8 bytes an entry
    text = ''.join(a + b for a in CHARSET_94_FULL for b in CHARSET_94_FULL)
    aut = Automaton.ngram([ch + text for ch in CHARSET_94_FULL], 3, TOK)
    assert 8931 <= aut.num_states <= 8931 + 95 and 6.7e6 < aut.nbytes < 6.9e6
    assert np.abs([_logsumexp(r) for r in aut.weight64[::97]]).max() <= 1e-12


# ---- pattern -------------------------------------------------------------------------------------------------------------
PATTERNS = [r'abc', r'a|bc|', r'(ab|c)*1', r'[a-c]+[^a-c0]?', r'\d{3}', r'\w{1,3}-\d*', r'a.c', r'(a(b|c){2}){1,2}_?', r'[\d_]+|[^\w]{2}', r'a\-b?\|?c*',
             r'(0|1)+(-(0|1)+)*', r'[]a]b{0,2}', r'[a\]-]{2}', r'((a|b)(0|1)?)+']


def _accepts(aut, ids):
    return aut.walk(ids)[0] == 0


@pytest.mark.parametrize('pattern', PATTERNS)
def test_pattern_accepts_what_re_fullmatch_accepts(pattern):
    """2000 strings over the small charset, half drawn uniformly and half by random walks of the DFA (cut at a random point or carried to
    an accepting state, then sometimes spoiled by one edit), so that both outcomes occur; '|' is no character of the charset, so the
    escaped one of the tenth pattern can never match, here or in `re`."""
    if r'\|' in pattern:
        with pytest.raises(ValueError, match='position 5'):
            Automaton.pattern(pattern, SMALL)
        pattern = pattern.replace(r'\|?', '')
    aut = Automaton.pattern(pattern, SMALL)
    assert not aut.weight64.any() and aut.words is None
    rx = re.compile(pattern)
    rng = random.Random(len(pattern))
    chars = SMALL._itos[1:len(SMALL) - 2]
    table = aut.next.numpy()
    strings = [''.join(rng.choice(chars) for _ in range(rng.randint(0, 7))) for _ in range(1000)]
    for _ in range(1000):
        s, out = 0, []
        for _ in range(rng.randint(0, 9)):
            kids = [c for c in range(1, table.shape[1]) if table[s, c] >= 0]
            if not kids or (table[s, 0] >= 0 and rng.random() < 0.3):
                break
            c = rng.choice(kids)
            out.append(c)
            s = table[s, c]
        text = SMALL._ids2tok(out)
        if text and rng.random() < 0.2:
            k = rng.randrange(len(text))
            text = text[:k] + rng.choice(chars) + text[k + 1:]
        strings.append(text)
    outcomes = set()
    for text in strings:
        want = rx.fullmatch(text) is not None
        assert _accepts(aut, SMALL._tok2ids(text)) == want, (pattern, text)
        outcomes.add(want)
    assert outcomes == {True, False}
    # no dead state: every state reaches an accepting one
    reach = {s for s in range(aut.num_states) if table[s, 0] >= 0}
    while True:
        more = {s for s in range(aut.num_states) if s not in reach and any(t in reach for t in table[s, 1:] if t >= 0)}
        if not more:
            break
        reach |= more
    assert reach == set(range(aut.num_states))


@pytest.mark.parametrize('pattern,position', [('^ab', 0), ('ab$', 2), ('a*?', 2), ('a+?', 2), ('a??', 2), ('a*+', 2), ('a{2}{3}', 4), ('(?:ab)', 0), ('(?P<x>a)', 0),
                                              ('(a)\\1', 3), ('a\\b', 1), ('\\s', 0), ('\\D', 0), ('[\\s]', 1), ('a{2,}', 1), ('a{,2}', 1), ('a{x}', 1),
                                              ('a{3,2}', 1), ('*a', 0), ('a|*', 2), ('(ab', 0), ('ab)', 2), ('[ab', 0), ('a]', 1), ('a\\', 1), ('[c-a]', 4),
                                              ('[[:alpha:]]', 1), ('x', 0), ('[\\d-a]', 3)])
def test_pattern_refuses_what_is_outside_the_subset(pattern, position):
    with pytest.raises(ValueError, match=f'position {position} '):
        Automaton.pattern(pattern, SMALL)


def test_pattern_fixed_length_and_empty_language():
    aut = Automaton.pattern('[0-9]{3}', TOK)
    assert aut.num_states == 4
    for text, want in (('123', True), ('12', False), ('1234', False), ('12a', False), ('', False)):
        assert _accepts(aut, TOK._tok2ids(text)) == want
    none = Automaton.pattern('a[^a-c01_-]', SMALL)          # the class is empty over this charset: nothing matches, the start state stays
    assert none.num_states == 1 and (none.next < 0).all()


# ---- stack -----------------------------------------------------------------------------------------------------------------
def test_stack_walks_as_the_parts_do():
    rng = random.Random(5)
    parts = [Automaton.from_lexicon(['ab', 'abc', 'b'], [5, 1, 2], SMALL), Automaton.from_lexicon(['c', 'ca'], [1, 9], SMALL),
             Automaton.from_lexicon(['0_', 'a'], [3, 3], SMALL)]
    both, roots = Automaton.stack(parts)
    assert roots.dtype == torch.int32 and roots.tolist() == [0, parts[0].num_states, parts[0].num_states + parts[1].num_states]
    assert both.words == ['ab', 'abc', 'b', 'c', 'ca', '0_', 'a'] and both.num_states == sum(p.num_states for p in parts)
    chars = SMALL._itos[1:len(SMALL) - 2]
    firsts = [0, 3, 5]
    for k, part in enumerate(parts):
        for text in [''.join(rng.choice(chars) for _ in range(rng.randint(0, 3))) for _ in range(300)] + part.words:
            ids = SMALL._tok2ids(text)
            tag, path, prefix = part.walk(ids)
            got = both.walk(ids, int(roots[k]))
            assert got == ((tag + firsts[k]) if tag >= 0 else -1, path, prefix), (k, text)
    pats = [Automaton.pattern('a+', SMALL), Automaton.pattern('[01]{2}', SMALL), Automaton.ngram(['ab', 'ba'], 2, SMALL)]
    mixed, roots = Automaton.stack(pats)
    assert mixed.words is None
    for k, part in enumerate(pats):
        for text in [''.join(rng.choice(chars) for _ in range(rng.randint(0, 4))) for _ in range(300)]:
            assert mixed.walk(SMALL._tok2ids(text), int(roots[k])) == part.walk(SMALL._tok2ids(text))
    with pytest.raises(ValueError, match='all or none'):
        Automaton.stack([parts[0], pats[0]])
    with pytest.raises(ValueError, match='same classes'):
        Automaton.stack([parts[0], Automaton.pattern('a', NG)])


def test_constructor_checks_the_tables():
    with pytest.raises(ValueError, match='states >= 1'):
        Automaton(np.zeros((2, 5), dtype=np.int32), np.zeros((2, 4)))
    aut = Automaton(torch.zeros(1, 5, dtype=torch.int32), torch.zeros(1, 5))
    assert aut.num_states == 1 and aut.num_classes == 5 and aut.nbytes == 40 and aut.table('cpu')[0] is aut.next and aut.to('cpu') is aut


# ---- read.py ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('flags,message', [
    (['--priors'], '--priors needs --lexicon'),
    (['--lexicon', 'w.txt', '--lm', 'c.txt'], 'one table'),
    (['--lexicon', 'w.txt', '--pattern', 'a+'], 'one table'),
    (['--lm', 'c.txt', '--pattern', 'a+'], 'one of them'),
    (['--lexicon', 'w.txt', '--priors', '--lm', 'c.txt'], 'one of them'),
    (['--lm-order', '2'], '--lm-order needs --lm'),
    (['--lm', 'c.txt', '--lm-order', '5'], r'\[1, 4\]'),
    (['--lm-weight', '0.5'], 'need --priors, --lm or --pattern'),
    (['--char-bonus', '0.5', '--nbest', '3'], 'need --priors, --lm or --pattern'),
    (['--lm', 'c.txt', '--nbest', '3', '--refine-beams', 'score'], 'refinement under a weighted automaton'),
    (['--pattern', 'a+', '--nbest', '3', '--refine-beams', 'edit'], 'refinement under a weighted automaton'),
    (['--lexicon', 'w.txt', '--priors', '--match'], 'refinement under a weighted automaton'),
    (['--pattern', 'a+', '--boxes'], '--boxes'),
    (['--lm', 'c.txt', '--lm-weight', 'inf'], 'finite'),
    (['--pattern', 'a+', '--nbest', '9', '--beam', '4'], '--beam must be at least --nbest'),
])
def test_read_cli_refuses_contradictions(flags, message, capsys):
    pytest.importorskip('PIL.Image')
    import read as read_cli
    with pytest.raises(SystemExit) as exit_info:
        read_cli.main(['pretrained=parseq', '--images', 'a.png', *flags])
    assert exit_info.value.code == 2 and re.search(message, capsys.readouterr().err)


def test_read_cli_word_counts(tmp_path):
    pytest.importorskip('PIL.Image')
    import read as read_cli
    f = tmp_path / 'counts.txt'
    f.write_text('the 120\n\nthen\t7.5\n  a   0\n')
    assert read_cli.load_word_counts(str(f)) == (['the', 'then', 'a'], [120.0, 7.5, 0.0])
    for bad in ('the\n', 'the x\n', 'the 1 2\n', 'the -1\n', 'the nan\n', 'the inf\n'):
        f.write_text('ok 1\n' + bad)
        with pytest.raises(ValueError, match='line 2'):
            read_cli.load_word_counts(str(f))
