"""A word list as the trie table of the lexicon-constrained beam search.

The table is dense: `next` int32 [nodes, C] over the head's C classes (`<eos>` and the charset, the tokenizer's ids 0 .. C - 1).
`next[n, c] >= 0` is the child of node `n` along class `c`; `next[n, eos_id] >= 0` says a word ends at `n` and is its word id, the index
into `Lexicon.words`; every other entry is -1.  Nodes are numbered breadth first, children in ascending class order, so the same words in
the same order always give the same table.  Several tries may share one table (`Lexicon.forest`): per-image word lists in one call, each
image starting at its own root.  `nodes * C * 4` bytes: about 95 MB for a 250 k-node trie at C = 95.

The same words also have a packed form for lexicon matching, built on first use: one 32-byte row per entered word in
ascending word id — bytes 0 .. 30 the class ids, byte 31 the length — with the word id of every row beside it and, for a forest, every
list's [begin, end) range of rows.  32 bytes a word whatever the list shares: about 3 MB for 90 k words.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor


class CharsetEncoder:
    """Strings as the head's class ids (`<eos>` and the charset: the tokenizer's ids 0 .. C - 1), for the host builders of search tables
    (`Lexicon`, `parseq_amd.automaton.Automaton`).  `fold_case=True` folds to the charset's only case when it has one."""

    def __init__(self, tokenizer, fold_case: bool = False) -> None:
        self.eos_id = int(tokenizer.eos_id)
        self.num_classes = len(tokenizer) - 2
        self.stoi: Dict[str, int] = {ch: i for i, ch in enumerate(tokenizer._itos[:self.num_classes]) if i != self.eos_id}
        charset = ''.join(self.stoi)
        self.fold = (str.lower if charset == charset.lower() else str.upper if charset == charset.upper() else None) if fold_case else None

    def encode(self, text: str) -> Optional[List[int]]:
        """The class ids of `text` (folded), None if it has a character outside the charset."""
        if self.fold is not None:
            text = self.fold(text)
        try:
            return [self.stoi[ch] for ch in text]
        except KeyError:
            return None


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
        self.encoder = CharsetEncoder(tokenizer, fold_case)
        self.eos_id, self.num_classes = self.encoder.eos_id, self.encoder.num_classes
        self.max_label_length = int(max_label_length)
        self.skipped = 0
        self._stoi, self._fold = self.encoder.stoi, self.encoder.fold
        self._device_tables: Dict[torch.device, Tensor] = {}
        self._entries: List[Tuple[int, List[int]]] = []      # (word id, class ids) of every word entered into a trie, in ascending id
        self._list_rows: List[Tuple[int, int]] = []          # per list its [begin, end) range of `_entries`
        self._packed: Dict[bool, np.ndarray] = {}
        self._device_packed: Dict[Tuple[torch.device, bool], Dict[str, Optional[Tensor]]] = {}

    def encode_word(self, word: str) -> Optional[List[int]]:
        """The class ids a word is entered as, None for a word the trie leaves out."""
        if not 0 < len(self._fold(word) if self._fold is not None else word) <= self.max_label_length:
            return None
        return self.encoder.encode(word)

    @property
    def entries(self) -> List[Tuple[int, List[int]]]:
        """(word id, class ids) of every word entered into a trie, in ascending id (skipped words and repeats have none)."""
        return self._entries

    def _build(self, lists: List[List[str]]) -> Tuple[Tensor, List[int]]:
        rows: List[np.ndarray] = []
        roots, first_id = [], 0
        for words in lists:
            # the trie in insertion order: per node a {class: node} dictionary and the word that ends there
            children: List[Dict[int, int]] = [{}]
            ends: List[int] = [-1]
            begin = len(self._entries)
            for k, word in enumerate(words):
                ids = self.encode_word(word)
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
                    self._entries.append((first_id + k, ids))
            self._list_rows.append((begin, len(self._entries)))
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

    # ---- the packed form --------------------------------------------------------------------------
    ROW_BYTES = 32             # PARSEQ_LEXICON_ROW_BYTES
    MAX_READING = 32           # characters of a reading the matching kernel compares

    @property
    def num_rows(self) -> int:
        """Words in the packed table: the entered ones (skipped words and repeats of a word within its list have no row)."""
        return len(self._entries)

    @property
    def row_ids(self) -> Tensor:
        """int32 [num_rows]: the word id (index into `words`) of every row, ascending."""
        return torch.tensor([k for k, _ in self._entries], dtype=torch.int32)

    @property
    def list_ranges(self) -> Tensor:
        """int32 [lists, 2]: every list's [begin, end) range of rows (one list for a plain `Lexicon`)."""
        return torch.tensor(self._list_rows, dtype=torch.int32).reshape(-1, 2)

    def fold_map(self) -> Tensor:
        """int32 [C]: the class a class is matched as under `ignore_case` — a letter's lower-case class where the charset has one, itself
        otherwise (`<eos>`, digits, signs, and every class of a single-case charset)."""
        fold = list(range(self.num_classes))
        for ch, i in self._stoi.items():
            fold[i] = self._stoi.get(ch.lower(), i) if len(ch.lower()) == 1 else i
        return torch.tensor(fold, dtype=torch.int32)

    def rows(self, ignore_case: bool = False) -> Tensor:
        """uint8 [num_rows, 32] on the host: the words' class ids (through `fold_map` with `ignore_case`) and, in byte 31, their lengths."""
        if self.num_classes > 256 or self.max_label_length > self.ROW_BYTES - 1:
            raise ValueError(f'the packed word table holds class ids below 256 and words of at most 31 characters; this lexicon has {self.num_classes} '
                             f'classes and max_label_length {self.max_label_length}')
        if ignore_case not in self._packed:
            table = np.zeros((len(self._entries), self.ROW_BYTES), dtype=np.uint8)
            fold = self.fold_map().numpy() if ignore_case else None
            for r, (_, ids) in enumerate(self._entries):
                table[r, :len(ids)] = ids if fold is None else fold[ids]
                table[r, self.ROW_BYTES - 1] = len(ids)
            self._packed[ignore_case] = table
        return torch.from_numpy(self._packed[ignore_case])

    @property
    def rows_nbytes(self) -> int:
        return self.num_rows * self.ROW_BYTES

    def match_table(self, device, ignore_case: bool = False) -> Dict[str, Optional[Tensor]]:
        """The packed form on `device`, uploaded once (as `table(device)` is): `table` the rows that are matched, `own` the words' own rows
        (the same tensor without `ignore_case`), `row_ids`, `ranges` [lists, 2] and `fold` (None without `ignore_case`)."""
        device = torch.device(device)
        if device.type != 'cpu' and device.index is None:
            device = torch.device(device.type, torch.cuda.current_device())
        key = (device, bool(ignore_case))
        if key not in self._device_packed:
            own = self._device_packed[(device, False)]['own'] if (device, False) in self._device_packed else self.rows(False).to(device)
            self._device_packed[key] = {'table': self.rows(True).to(device) if ignore_case else own, 'own': own, 'row_ids': self.row_ids.to(device),
                                        'ranges': self.list_ranges.to(device), 'fold': self.fold_map().to(device) if ignore_case else None}
        return self._device_packed[key]

    def encode_readings(self, readings: Sequence[str]) -> Tuple[Tensor, Tensor]:
        """(int32 [B, 32] class ids, int32 [B] lengths) of strings as the matching kernel reads them: a character outside the charset is -1 (it
        equals no character of any word), the case is folded as the words' was (`fold_case`).  More than 32 characters: ValueError."""
        tok = np.full((len(readings), self.MAX_READING), self.eos_id, dtype=np.int32)
        lengths = np.zeros(len(readings), dtype=np.int32)
        for b, text in enumerate(readings):
            if self._fold is not None:
                text = self._fold(text)
            if len(text) > self.MAX_READING:
                raise ValueError(f'a reading of {len(text)} characters: the matching kernel compares at most {self.MAX_READING}')
            tok[b, :len(text)] = [self._stoi.get(ch, -1) for ch in text]
            lengths[b] = len(text)
        return torch.from_numpy(tok), torch.from_numpy(lengths)

    def nearest(self, readings, n: int, lists=None, ignore_case: bool = False, device='cuda', crops_per_block: int = 0) -> Tuple[Tensor, Tensor]:
        """The `n` words nearest to every reading in Levenshtein distance, no model involved: (word ids int32 [B, n],
        distances int32 [B, n]) on `device`, ordered by (distance, word id); a slot beyond the list holds -1 and `MATCH_DEAD`.  `readings`:
        strings, or an int tensor [B, L <= 32] of class ids in which a reading ends before its first `<eos>`.  `lists` (a forest's list index
        per reading) matches every reading against its own list.  One launch pair on the device, nothing read back."""
        from . import _native
        if isinstance(readings, Tensor):
            if readings.dim() != 2 or not 1 <= readings.shape[1] <= self.MAX_READING:
                raise ValueError(f'nearest: readings must be [B, L] with 1 <= L <= {self.MAX_READING}, got {tuple(readings.shape)}')
            tok, lengths = readings.to(device, torch.int32).contiguous(), None
        else:
            tok, lengths = (t.to(device) for t in self.encode_readings(list(readings)))
        B = tok.shape[0]
        if not 1 <= int(n) <= MATCH_MAX_N:
            raise ValueError(f'nearest: n must be in [1, {MATCH_MAX_N}], got {n}')
        if self.num_rows == 0:
            raise ValueError('nearest: no word of the lexicon was entered (the packed table is empty)')
        t = self.match_table(tok.device, ignore_case)
        ranges = self.crop_ranges(lists, B, tok.device)
        ids = torch.empty(B, n, dtype=torch.int32, device=tok.device)
        dist = torch.empty(B, n, dtype=torch.int32, device=tok.device)
        if B == 0:
            return ids, dist
        lib = _native.lib()
        need = lib.parseq_op_lexicon_match_workspace_bytes(B, self.num_rows, int(n))
        if need == 0:
            raise ValueError(f'nearest: {B} readings x {self.num_rows} words x n = {n} is outside what one call matches')
        ws = torch.empty(need, dtype=torch.uint8, device=tok.device)
        with _native.guard(tok):
            _native.check(lib.parseq_op_lexicon_match(_native.ptr(tok), tok.shape[1], _native.ptr(lengths), B, _native.ptr(t['table']), self.num_rows,
                                                      _native.ptr(t['row_ids']), _native.ptr(ranges), _native.ptr(t['fold']), self.num_classes, self.eos_id,
                                                      int(n), int(crops_per_block), _native.ptr(ids), _native.ptr(dist), _native.ptr(ws), need,
                                                      _native.stream_ptr(tok)))
        return ids, dist

    def crop_ranges(self, lists, batch: int, device) -> Optional[Tensor]:
        """int32 [batch, 2] on `device`: the rows of list `lists[b]` for crop b; None for `lists=None` (every crop against every row)."""
        if lists is None:
            return None
        lists = torch.as_tensor(lists, dtype=torch.int64).cpu()
        if lists.dim() != 1 or lists.shape[0] != batch:
            raise ValueError(f'lists must be [batch] = [{batch}], got {tuple(lists.shape)}')
        if batch and (int(lists.min()) < 0 or int(lists.max()) >= len(self._list_rows)):
            raise ValueError(f'lists: a list index outside [0, {len(self._list_rows)})')
        return self.list_ranges[lists].to(device).contiguous()


MATCH_MAX_N = 16                # PARSEQ_BEAM_MAX_WIDTH
MATCH_DEAD = 0x7FFFFFFF         # PARSEQ_LEXICON_MATCH_DEAD: the distance of a slot beyond the list
