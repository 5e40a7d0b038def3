"""A word list as the trie table of the lexicon-constrained beam search.

The table is dense: `next` int32 [nodes, C] over the head's C classes (`<eos>` and the charset, the tokenizer's ids 0 .. C - 1).
`next[n, c] >= 0` is the child of node `n` along class `c`; `next[n, eos_id] >= 0` says a word ends at `n` and is its word id, the index
into `Lexicon.words`; every other entry is -1.  Nodes are numbered breadth first, children in ascending class order, so the same words in
the same order always give the same table.  Several tries may share one table (`Lexicon.forest`): per-image word lists in one call, each
image starting at its own root.  `nodes * C * 4` bytes: about 95 MB for a 250 k-node trie at C = 95.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor


class Lexicon:
    """`Lexicon(words, tokenizer, fold_case=False)`.  `words` is kept as given: a finished hypothesis' word id indexes it, so a caller gets
    the list's own spelling back.  Left out of the trie and counted in `.skipped`: empty words, words with a character outside the
    tokenizer's charset and words of more than `max_label_length` characters (they could never finish).  A word that is already in the
    trie keeps the first id.  `fold_case=True` folds the words to the charset's only case when it has one (`Hello` is entered as `hello`
    under a lower-case charset and read back as `Hello`)."""

    def __init__(self, words: Sequence[str], tokenizer, fold_case: bool = False, max_label_length: int = 25) -> None:
        self._setup(tokenizer, fold_case, max_label_length)
        self.words: List[str] = list(words)
        self.next, roots = self._build([self.words])
        assert roots == [0]

    @classmethod
    def forest(cls, word_lists: Sequence[Sequence[str]], tokenizer, fold_case: bool = False,
               max_label_length: int = 25) -> Tuple['Lexicon', Tensor]:
        """(lexicon, roots int32 [len(word_lists)]): one trie per list in one table, list b's root at roots[b].  `lexicon.words` is the
        concatenation of the lists; the tries share no node."""
        self = cls.__new__(cls)
        self._setup(tokenizer, fold_case, max_label_length)
        lists = [list(ws) for ws in word_lists]
        self.words = [w for ws in lists for w in ws]
        self.next, roots = self._build(lists)
        return self, torch.tensor(roots, dtype=torch.int32)

    # ---- construction --------------------------------------------------------------------------------------------------
    def _setup(self, tokenizer, fold_case, max_label_length):
        self.eos_id = int(tokenizer.eos_id)
        self.num_classes = len(tokenizer) - 2
        self.max_label_length = int(max_label_length)
        self.skipped = 0
        self._stoi: Dict[str, int] = {ch: i for i, ch in enumerate(tokenizer._itos[:self.num_classes]) if i != self.eos_id}
        charset = ''.join(self._stoi)
        self._fold = (str.lower if charset == charset.lower() else str.upper if charset == charset.upper() else None) if fold_case else None
        self._device_tables: Dict[torch.device, Tensor] = {}

    def _encode(self, word: str) -> Optional[List[int]]:
        if self._fold is not None:
            word = self._fold(word)
        if not 0 < len(word) <= self.max_label_length:
            return None
        try:
            return [self._stoi[ch] for ch in word]
        except KeyError:
            return None

    def _build(self, lists: List[List[str]]) -> Tuple[Tensor, List[int]]:
        rows: List[np.ndarray] = []
        roots, first_id = [], 0
        for words in lists:
            # the trie in insertion order: per node a {class: node} dictionary and the word that ends there
            children: List[Dict[int, int]] = [{}]
            ends: List[int] = [-1]
            for k, word in enumerate(words):
                ids = self._encode(word)
                if ids is None:
                    self.skipped += 1
                    continue
                n = 0
                for c in ids:
                    nxt = children[n].get(c)
                    if nxt is None:
                        nxt = len(children)
                        children[n][c] = nxt
                        children.append({})
                        ends.append(-1)
                    n = nxt
                if ends[n] < 0:
                    ends[n] = first_id + k
            # renumbered breadth first, children in ascending class order
            base = sum(r.shape[0] for r in rows)
            order, number = [0], {0: 0}
            for n in order:
                for c in sorted(children[n]):
                    number[children[n][c]] = len(order)
                    order.append(children[n][c])
            table = np.full((len(order), self.num_classes), -1, dtype=np.int32)
            for new, n in enumerate(order):
                for c, child in children[n].items():
                    table[new, c] = base + number[child]
                table[new, self.eos_id] = ends[n]
            roots.append(base)
            rows.append(table)
            first_id += len(words)
        return torch.from_numpy(np.concatenate(rows, 0) if rows else np.full((1, self.num_classes), -1, dtype=np.int32)), roots

    # ---- use -----------------------------------------------------------------------------------------------------------
    @property
    def num_nodes(self) -> int:
        return self.next.shape[0]

    @property
    def nbytes(self) -> int:
        return self.next.numel() * 4

    def __len__(self) -> int:
        return len(self.words)

    def to(self, device) -> 'Lexicon':
        """Uploads the table to `device` once; later calls (and `table(device)`) reuse the copy."""
        self.table(device)
        return self

    def table(self, device) -> Tensor:
        device = torch.device(device)
        if device.type == 'cpu':
            return self.next
        if device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        if device not in self._device_tables:
            self._device_tables[device] = self.next.to(device)
        return self._device_tables[device]
