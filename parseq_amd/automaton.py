"""Deterministic weighted automata over the head's classes, the tables of `beam_search(automaton=)`.

An automaton is two dense tables over the C classes (`<eos>` and the charset, the tokenizer's ids 0 .. C - 1): `next` int32 [S, C] with
exactly the meaning of a lexicon's trie table — a negative entry is "not allowed", a character column holds the
successor state, the `<eos>` column a non-negative tag where the state accepts (a word id for a lexicon, 0 otherwise) — and `weight` fp32
[S, C], the natural-log weight of taking class c from state s (the `<eos>` column: the final weight).  Cycles and shared states are
allowed; a non-finite weight makes its arc not allowed.  State 0 is where a search without `roots` starts.  Everything here is host
float64 and numpy; the weights are rounded to fp32 once, at the end (`weight64` keeps them as they were before).

  Automaton.from_lexicon   a word list with counts: section 19's trie, every path summing to the log of the word's smoothed relative frequency
  Automaton.ngram          a character n-gram model (order 1 .. 4), interpolated Witten-Bell, every row resolved at build time
  Automaton.pattern        a regular expression (a stated subset) as a DFA over the charset, all weights 0
  Automaton.stack          several automata in one table, one root each (per-crop grammars)

`S * C * 8` bytes: a trigram over the 94-character set has at most 1 + 94 + 94 * 94 = 8931 contexts plus the start contexts, about 8.9 k
states and about 6.8 MB.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .lexicon import CharsetEncoder, Lexicon

MAX_TABLE_BYTES = 256 << 20      # a builder refuses a table (next and weight together) above this
NGRAM_MAX_ORDER = 4
_BOS = -1                        # the start-of-sequence symbol inside an n-gram context (never a class)


def _check_size(states: int, classes: int, what: str, max_bytes: int) -> None:
    need = states * classes * 8
    if need > max_bytes:
        raise ValueError(f'{what}: {states} states x {classes} classes need a table of {need} bytes, above the limit of {max_bytes} bytes')


class Automaton:
    """`Automaton(next, weight, words=None)`: the two tables ([S, C], anything `numpy.asarray` takes) and, for a lexicon, the strings the
    accept tags index.  `eos_id` is the `<eos>` column (the tokenizer's 0)."""

    def __init__(self, next, weight, words: Optional[Sequence[str]] = None, eos_id: int = 0) -> None:
        nxt = np.ascontiguousarray(np.asarray(next.cpu() if isinstance(next, Tensor) else next), dtype=np.int32)
        w64 = np.ascontiguousarray(np.asarray(weight.cpu() if isinstance(weight, Tensor) else weight), dtype=np.float64)
        if nxt.ndim != 2 or nxt.shape[0] < 1 or w64.shape != nxt.shape:
            raise ValueError(f'Automaton: next and weight must both be [states >= 1, classes], got {nxt.shape} and {w64.shape}')
        if not 0 <= int(eos_id) < nxt.shape[1]:
            raise ValueError(f'Automaton: eos_id {eos_id} outside [0, {nxt.shape[1]})')
        self.next: Tensor = torch.from_numpy(nxt)
        self.weight64: np.ndarray = w64
        with np.errstate(over='ignore'):
            self.weight: Tensor = torch.from_numpy(w64.astype(np.float32))
        self.words: Optional[List[str]] = None if words is None else list(words)
        self.eos_id = int(eos_id)
        self.skipped = 0
        self._device_tables: Dict[torch.device, Tuple[Tensor, Tensor]] = {}

    # ---- use -----------------------------------------------------------------------------------------------------------
    @property
    def num_states(self) -> int:
        return self.next.shape[0]

    @property
    def num_classes(self) -> int:
        return self.next.shape[1]

    @property
    def nbytes(self) -> int:
        return self.next.numel() * 8

    def to(self, device) -> 'Automaton':
        """Uploads the tables to `device` once; later calls (and `table(device)`) reuse the copies."""
        self.table(device)
        return self

    def table(self, device) -> Tuple[Tensor, Tensor]:
        """(next, weight) on `device`."""
        device = torch.device(device)
        if device.type == 'cpu':
            return self.next, self.weight
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if device not in self._device_tables:
            self._device_tables[device] = (self.next.to(device), self.weight.to(device))
        return self._device_tables[device]

    def walk(self, ids: Sequence[int], root: int = 0) -> Tuple[int, float, float]:
        """Follows class ids (no `<eos>`) from `root`: (tag, path weight with the final weight, path weight without it) in float64 — tag -1
        if an arc is not allowed or the state reached does not accept."""
        nxt, w = self.next.numpy(), self.weight64
        s, total = int(root), 0.0
        if not 0 <= s < nxt.shape[0]:
            return -1, float('-inf'), float('-inf')
        for c in ids:
            t = int(nxt[s, c])
            if c == self.eos_id or t < 0 or t >= nxt.shape[0] or not np.isfinite(w[s, c]):
                return -1, float('-inf'), float('-inf')
            total += float(w[s, c])
            s = t
        tag = int(nxt[s, self.eos_id])
        if tag < 0 or not np.isfinite(w[s, self.eos_id]):
            return -1, float('-inf'), total
        return tag, total + float(w[s, self.eos_id]), total

    # ---- a word list with counts ---------------------------------------------------------------------------------------
    @classmethod
    def from_lexicon(cls, words: Sequence[str], counts: Sequence[float], tokenizer, fold_case: bool = False, smoothing: float = 1.0) -> 'Automaton':
        """Section 19's trie of `words` (the same numbering: `next` equals `Lexicon(words, tokenizer, fold_case).next`, the tags are word ids)
        with the counts as a prior.  A word's mass is its count plus `smoothing`; the count of a word that repeats an earlier one goes to the
        first.  An arc's weight is the log of the mass below its child over the mass below its state, the `<eos>` weight the log of the mass of
        the word ending there over the same, so a word's path sums to the log of its share of the whole mass.  A word of mass 0 gets a weight
        of -inf: it is not allowed."""
        words = list(words)
        counts = np.asarray(list(counts), dtype=np.float64)
        if counts.shape != (len(words),):
            raise ValueError(f'from_lexicon: {len(words)} words but {counts.size} counts')
        if not (np.isfinite(counts).all() and (counts >= 0).all()) or not (np.isfinite(smoothing) and smoothing >= 0):
            raise ValueError('from_lexicon: the counts and the smoothing must be finite and not negative')
        lex = Lexicon(words, tokenizer, fold_case)
        nxt = lex.next.numpy()
        S, C = nxt.shape
        eos = lex.eos_id
        below, ends = np.zeros(S), np.zeros(S)

        def add(ids, mass):
            n = 0
            below[0] += mass
            for c in ids:
                n = int(nxt[n, c])
                below[n] += mass
            ends[n] += mass
        for _, ids in lex.entries:
            add(ids, float(smoothing))
        for word, count in zip(words, counts):
            ids = lex.encode_word(word)
            if ids is not None:
                add(ids, float(count))
        weight = np.full((S, C), -np.inf)
        rows, cols = np.nonzero(nxt >= 0)
        final = cols == eos
        with np.errstate(divide='ignore', invalid='ignore'):
            weight[rows[~final], cols[~final]] = np.log(below[nxt[rows[~final], cols[~final]]] / below[rows[~final]])
            weight[rows[final], eos] = np.log(ends[rows[final]] / below[rows[final]])
        weight[np.isnan(weight)] = -np.inf      # (0 / 0 below a state all of whose words have no mass)
        self = cls(nxt, weight, words, eos)
        self.skipped = lex.skipped
        return self

    # ---- a character n-gram model ----------------------------------------------------------------------------------------
    @classmethod
    def ngram(cls, texts: Sequence[str], order: int, tokenizer, fold_case: bool = False, max_bytes: int = MAX_TABLE_BYTES) -> 'Automaton':
        """A character n-gram model of `texts`, each a sequence from the start to `<eos>` (`<eos>` is a class of the model like any other;
        every state accepts, tag 0).  The states are the contexts: state 0 the start context, state 1 the empty one, then every context
        of fewer than `order` symbols seen in `texts`, shorter first.  The successor of (h, c) is the longest suffix of hc that is a state.
        Every row is resolved at build time by interpolated Witten-Bell smoothing,
            P(c | h) = (n(h, c) + T(h) P(c | h')) / (n(h) + T(h)),
        T(h) the number of distinct successors of h, h' = h without its oldest symbol, uniform over the C classes below the empty context;
        so no back-off happens during the search and every row sums to 1.  A text with a character outside the charset is left out and
        counted in `.skipped`.  A table of more than `max_bytes` bytes is refused."""
        if not isinstance(order, int) or isinstance(order, bool) or not 1 <= order <= NGRAM_MAX_ORDER:
            raise ValueError(f'ngram: order must be an integer in [1, {NGRAM_MAX_ORDER}], got {order!r}')
        enc = CharsetEncoder(tokenizer, fold_case)
        C, eos = enc.num_classes, enc.eos_id
        seqs, skipped = [], 0
        for text in texts:
            ids = enc.encode(text)
            if ids is None:
                skipped += 1
            else:
                seqs.append(ids)
        if not seqs:
            raise ValueError('ngram: no text to count (every text has a character outside the charset, or there is none)')
        # n(h, c) for every context h of 0 .. order - 1 symbols, the start symbol included
        counts: Dict[Tuple[int, ...], np.ndarray] = {(): np.zeros(C), (_BOS,): np.zeros(C)}
        for ids in seqs:
            hist = [_BOS] + ids
            for i, c in enumerate(ids + [eos]):
                for k in range(min(order - 1, i + 1) + 1):
                    h = tuple(hist[i + 1 - k:i + 1])
                    if h not in counts:
                        counts[h] = np.zeros(C)
                    counts[h][c] += 1
        start = (_BOS,)
        states = [start, ()] + sorted((h for h in counts if h not in (start, ())), key=lambda h: (len(h), h))
        _check_size(len(states), C, f'ngram of order {order}', max_bytes)
        index = {h: s for s, h in enumerate(states)}
        prob: Dict[Tuple[int, ...], np.ndarray] = {}
        longest: Dict[Tuple[int, ...], np.ndarray] = {}      # per context g of at most order - 2 symbols: the longest suffix of gc that is a state
        nxt = np.empty((len(states), C), dtype=np.int32)
        weight = np.empty((len(states), C))
        for h in sorted(states, key=len):
            n = counts[h]
            if order == 1 and h == start:      # a unigram has no context: the start predicts as the empty context does
                prob[h] = prob[()]
                continue
            lower = prob[h[1:]] if h else np.full(C, 1.0 / C)
            distinct = float(np.count_nonzero(n))
            prob[h] = (n + distinct * lower) / (n.sum() + distinct)
        for h in sorted(states, key=len):
            if len(h) <= order - 2:
                row = longest[h[1:]].copy() if h else np.full(C, index[()], dtype=np.int32)
                for c in range(C):
                    if c != eos and h + (c,) in index:
                        row[c] = index[h + (c,)]
                longest[h] = row
        for s, h in enumerate(states):
            nxt[s] = longest[h] if len(h) <= order - 2 else (longest[h[1:]] if order >= 2 else index[()])
            nxt[s, eos] = 0
            weight[s] = np.log(prob[h])
        self = cls(nxt, weight, None, eos)
        self.skipped = skipped
        self.contexts = states      # the context of every state: class ids, -1 the start symbol
        return self

    # ---- a regular expression ----------------------------------------------------------------------------------------------
    @classmethod
    def pattern(cls, regex: str, tokenizer, max_bytes: int = MAX_TABLE_BYTES) -> 'Automaton':
        """The DFA of `regex` over the tokenizer's charset as an automaton: all weights 0, accept tag 0, a full match (no anchors needed or
        allowed).  The subset: literals, `\\` escapes of signs, `.` (any character of the charset), `[...]` with ranges and a leading `^`,
        `\\d`, `\\w`, groups `( )`, `|`, and the quantifiers `?`, `*`, `+`, `{m}`, `{m,n}`.  Anything else — anchors, lazy or possessive
        quantifiers, `(?...)` groups, back-references, other classes such as `\\s` or `\\b`, `{m,}`, a literal outside the charset — raises
        ValueError naming the position.  Inside `[...]` it is different: a class is a set of characters met with the charset, so a member
        the charset lacks — a lone character as much as part of a range — matches nothing and is no error (`[^,]` is every character of a
        charset without a comma).  Thompson's construction, then the subset construction; states that cannot reach an accepting
        one are removed, so a search never enters a prefix that cannot complete."""
        enc = CharsetEncoder(tokenizer)
        C, eos = enc.num_classes, enc.eos_id
        ast = _RegexParser(regex, enc.stoi).parse()
        nfa = _Nfa()
        first, last = nfa.build(ast)
        # subset construction
        start = nfa.closure({first})
        ids, order, trans = {start: 0}, [start], []
        for cur in order:
            row: Dict[int, set] = {}
            for s in cur:
                for classes, t in nfa.arcs[s]:
                    for c in classes:
                        row.setdefault(c, set()).add(t)
            out = {}
            for c, targets in row.items():
                nxt_set = nfa.closure(targets)
                if nxt_set not in ids:
                    ids[nxt_set] = len(order)
                    order.append(nxt_set)
                    _check_size(len(order), C, 'pattern', max_bytes)
                out[c] = ids[nxt_set]
            trans.append(out)
        accept = [last in cur for cur in order]
        # states that reach an accepting one, numbered in discovery order (the start stays state 0 even if the language is empty)
        live = set(s for s, a in enumerate(accept) if a)
        changed = True
        while changed:
            changed = False
            for s, out in enumerate(trans):
                if s not in live and any(t in live for t in out.values()):
                    live.add(s)
                    changed = True
        keep = [s for s in range(len(order)) if s in live or s == 0]
        number = {s: k for k, s in enumerate(keep)}
        nxt = np.full((len(keep), C), -1, dtype=np.int32)
        for s in keep:
            for c, t in trans[s].items():
                if t in live:
                    nxt[number[s], c] = number[t]
            if accept[s]:
                nxt[number[s], eos] = 0
        return cls(nxt, np.zeros(nxt.shape), None, eos)

    # ---- several automata in one table -------------------------------------------------------------------------------------
    @classmethod
    def stack(cls, automata: Sequence['Automaton']) -> Tuple['Automaton', Tensor]:
        """(automaton, roots int32 [len(automata)]): the tables one below the other, automaton k's state 0 at roots[k], as `Lexicon.forest`
        does for tries.  If the automata have `words` (all or none), the lists are concatenated and the tags moved with them."""
        automata = list(automata)
        if not automata:
            raise ValueError('stack: no automaton')
        C, eos = automata[0].num_classes, automata[0].eos_id
        with_words = [a.words is not None for a in automata]
        if any(a.num_classes != C or a.eos_id != eos for a in automata) or (any(with_words) and not all(with_words)):
            raise ValueError('stack: the automata must have the same classes and <eos>, and either all or none of them words')
        tables, weights, roots, words, base, first = [], [], [], [], 0, 0
        for a in automata:
            t = a.next.numpy().copy()
            chars = np.ones(C, dtype=bool)
            chars[eos] = False
            t[:, chars] = np.where(t[:, chars] >= 0, t[:, chars] + base, t[:, chars])
            if a.words is not None:
                t[:, eos] = np.where(t[:, eos] >= 0, t[:, eos] + first, t[:, eos])
                words += a.words
                first += len(a.words)
            tables.append(t)
            weights.append(a.weight64)
            roots.append(base)
            base += a.num_states
        self = cls(np.concatenate(tables, 0), np.concatenate(weights, 0), words if all(with_words) else None, eos)
        return self, torch.tensor(roots, dtype=torch.int32)


# ---- the regular subset of Automaton.pattern ---------------------------------------------------------------------------------
# The syntax tree: ('set', frozenset of class ids), ('cat', [nodes]), ('alt', [nodes]), ('rep', node, m, n).
_REPEAT_MAX = 256
_WORD = 'abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_'
_DIGIT = '0123456789'


class _RegexParser:
    def __init__(self, regex: str, stoi: Dict[str, int]) -> None:
        self.s, self.i, self.stoi = regex, 0, stoi

    def fail(self, what: str, at: Optional[int] = None):
        at = self.i if at is None else at
        raise ValueError(f'pattern: {what} at position {at} of {self.s!r}')

    def peek(self) -> str:
        return self.s[self.i] if self.i < len(self.s) else ''

    def chars(self, text: str) -> frozenset:
        return frozenset(self.stoi[ch] for ch in text if ch in self.stoi)

    def parse(self):
        node = self.alt()
        if self.i < len(self.s):
            self.fail("an unmatched ')'")
        return node

    def alt(self):
        branches = [self.cat()]
        while self.peek() == '|':
            self.i += 1
            branches.append(self.cat())
        return branches[0] if len(branches) == 1 else ('alt', branches)

    def cat(self):
        items = []
        while self.peek() not in ('', '|', ')'):
            items.append(self.repeat())
        return ('cat', items)

    def repeat(self):
        node = self.atom()
        ch = self.peek()
        if ch in ('?', '*', '+'):
            self.i += 1
            node = ('rep', node, 0 if ch != '+' else 1, 1 if ch == '?' else None)
        elif ch == '{':
            close = self.s.find('}', self.i)
            body = self.s[self.i + 1:close] if close > 0 else ''
            parts = body.split(',')
            if close < 0 or len(parts) > 2 or not all(p.isdigit() and p.isascii() for p in parts):
                self.fail('a repetition that is neither {m} nor {m,n}')
            m, n = int(parts[0]), int(parts[-1])
            if n < m or n > _REPEAT_MAX:
                self.fail(f'a repetition with n < m or n > {_REPEAT_MAX}')
            self.i = close + 1
            node = ('rep', node, m, n)
        else:
            return node
        if self.peek() in ('?', '*', '+', '{'):
            self.fail('a quantifier after a quantifier (lazy, possessive and stacked quantifiers are outside the subset)')
        return node

    def escape(self) -> frozenset:
        """The set of the escape at self.i (which is a backslash); advances past it."""
        at = self.i
        ch = self.s[self.i + 1] if self.i + 1 < len(self.s) else ''
        self.i += 2
        if ch == 'd':
            return self.chars(_DIGIT)
        if ch == 'w':
            return self.chars(_WORD)
        if ch == '' or ch.isalnum():
            self.fail(f'an escape outside the subset (\\{ch})' if ch else 'a lone backslash', at)
        return self.literal(ch, at)

    def literal(self, ch: str, at: int) -> frozenset:
        if ch not in self.stoi:
            self.fail(f'the character {ch!r}, which the charset does not have,', at)
        return frozenset([self.stoi[ch]])

    def atom(self):
        ch, at = self.peek(), self.i
        if ch == '(':
            if self.s.startswith('(?', self.i):
                self.fail('a (?...) group')
            self.i += 1
            node = self.alt()
            if self.peek() != ')':
                self.fail("a '(' without its ')'", at)
            self.i += 1
            return node
        if ch == '[':
            return ('set', self.char_class())
        if ch == '.':
            self.i += 1
            return ('set', frozenset(self.stoi.values()))
        if ch == '\\':
            return ('set', self.escape())
        if ch in ('^', '$'):
            self.fail('an anchor (the match is always a full match)')
        if ch in ('?', '*', '+', '{'):
            self.fail('a quantifier with nothing to repeat')
        if ch in (']', '}'):
            self.fail(f'a {ch!r} that closes nothing (escape it)')
        self.i += 1
        return ('set', self.literal(ch, at))

    def char_class(self) -> frozenset:
        at = self.i
        self.i += 1
        negate = self.peek() == '^'
        if negate:
            self.i += 1
        members: set = set()
        first = True
        while True:
            ch = self.peek()
            if ch == '':
                self.fail("a '[' without its ']'", at)
            if ch == ']' and not first:
                self.i += 1
                break
            first = False
            if ch == '[':
                self.fail('a [ inside a class (escape it; nested and POSIX classes are outside the subset)')
            if ch == '\\':
                esc = self.s[self.i + 1:self.i + 2]
                if esc in ('d', 'w'):
                    members |= self.escape()
                    if self.peek() == '-' and self.s[self.i + 1:self.i + 2] not in (']', ''):
                        self.fail('a range that starts at a class escape')
                    continue
                if esc == '' or esc.isalnum():
                    self.fail(f'an escape outside the subset (\\{esc})' if esc else 'a lone backslash')
                lo = esc
                self.i += 2
            else:
                lo = ch
                self.i += 1
            if self.peek() == '-' and self.s[self.i + 1:self.i + 2] not in (']', ''):
                self.i += 1
                hi = self.peek()
                if hi == '\\':
                    hi = self.s[self.i + 1:self.i + 2]
                    if hi == '' or hi.isalnum():
                        self.fail('a range that ends at a class escape')
                    self.i += 1
                elif hi == '[':
                    self.fail('a [ inside a class (escape it)')
                self.i += 1
                if ord(hi) < ord(lo):
                    self.fail(f'a reversed range {lo}-{hi}')
                members |= {k for c2, k in self.stoi.items() if ord(lo) <= ord(c2) <= ord(hi)}
            elif lo in self.stoi:
                members.add(self.stoi[lo])
        if negate:
            members = set(self.stoi.values()) - members
        return frozenset(members)


class _Nfa:
    """Thompson's construction: arcs[s] the (class set, target) arcs of state s, eps[s] its empty moves."""

    def __init__(self) -> None:
        self.arcs: List[List[Tuple[frozenset, int]]] = []
        self.eps: List[List[int]] = []

    def state(self) -> int:
        self.arcs.append([])
        self.eps.append([])
        return len(self.arcs) - 1

    def build(self, node) -> Tuple[int, int]:
        """(entry, exit) of the fragment of `node`."""
        kind = node[0]
        a, b = self.state(), self.state()
        if kind == 'set':
            if node[1]:
                self.arcs[a].append((node[1], b))
        elif kind == 'cat':
            cur = a
            for item in node[1]:
                x, y = self.build(item)
                self.eps[cur].append(x)
                cur = y
            self.eps[cur].append(b)
        elif kind == 'alt':
            for item in node[1]:
                x, y = self.build(item)
                self.eps[a].append(x)
                self.eps[y].append(b)
        else:
            _, inner, m, n = node
            cur = a
            for _ in range(m):
                x, y = self.build(inner)
                self.eps[cur].append(x)
                cur = y
            if n is None:      # a star after the m copies
                x, y = self.build(inner)
                hub = self.state()
                self.eps[cur].append(hub)
                self.eps[hub] += [x, b]
                self.eps[y].append(hub)
            else:
                for _ in range(n - m):      # n - m optional copies, each skippable to the exit
                    x, y = self.build(inner)
                    self.eps[cur] += [x, b]
                    cur = y
                self.eps[cur].append(b)
        return a, b

    def closure(self, states) -> frozenset:
        seen, stack = set(states), list(states)
        while stack:
            for t in self.eps[stack.pop()]:
                if t not in seen:
                    seen.add(t)
                    stack.append(t)
        return frozenset(seen)
