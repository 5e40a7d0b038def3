"""Evaluation with the metrics on the device: what the reference's `test.py:115-131` and `validation_step` /
`_aggregate_results` (`strhub/models/base.py:112-177`) compute, without a device-to-host copy per batch.

`eval_step` (parseq_amd/system.py) mirrors `BaseSystem._eval_step`: forward, copy ids and lengths to the host, then per
sample the test-charset adapter, a Python Levenshtein distance and float sums.  `Evaluator.update` keeps all of that on the
device: `parseq_eval_metrics` (csrc/eval_metrics.h) picks the characters exactly as `parseq_postprocess` does, maps them
through a table form of `CharsetAdapter`, computes the edit distance against the ground truth (uploaded as code points)
and adds the batch to a 40-byte accumulator.  `result()` makes the one small copy.

The table form of the adapter: `CharsetAdapter` lower- or upper-cases the whole prediction, then drops what is not in the test
charset.  Character by character that is a map `train token id -> one code point, or dropped`, which `adapter_table` builds
with Python's own `str.lower()` / `str.upper()` and the adapter's regex.  Two things a table cannot express, both decided
once, when the `Evaluator` is built:
  * a character that folds to more than one code point ('ß'.upper() == 'SS', 'İ'.lower() == 'i̇');
  * 'Σ' under lower-casing: Python lowers it to 'ς' at the end of a word and to 'σ' elsewhere, so the result depends on context.
For such a model `adapter_table` returns None and the `Evaluator` runs `eval_step` per batch and sums on the host (`host_path`
is True): same totals, the parent path's speed.

`ErrorAnalysis` says HOW the readings are wrong: `parseq_eval_errors` (csrc/eval_errors.h) takes the ids and lengths
the metrics kernel just wrote and the labels already uploaded, and keeps per-sample edit scripts and integer tables (operation totals,
accuracy by label length, errors by position, a confusion matrix) on the device; `ErrorReport` is the one copy.

Limits: a label of at most `MAX_GT` = 256 code points (the reference's dataset drops labels longer than `max_label_length`,
25 by default, before they get here: strhub/data/dataset.py:111-113); predictions of at most 32 positions (DEC_MAXL).
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch
from torch import Tensor

from .system import BatchResult, edit_distance, eval_step

MAX_GT = 256                 # PARSEQ_EVAL_MAX_GT


def adapter_table(tokenizer, charset_adapter) -> Optional[np.ndarray]:
    """int32 [len(tokenizer) - 2]: for every class the head predicts, the code point `charset_adapter` turns that character into, or
    -1 if it drops it (the <eos> entry is -1 and never read).  None if the adapter is not a per-character map for this charset."""
    classes = len(tokenizer) - 2                       # the head predicts neither <bos> nor <pad>
    table = np.full(classes, -1, dtype=np.int32)
    for token_id in range(classes):
        if token_id == tokenizer.eos_id:
            continue
        ch = tokenizer._itos[token_id]
        if ch == 'Σ' and charset_adapter.lowercase_only:
            return None                                # final-sigma rule: str.lower() looks at the neighbours
        folded = ch.lower() if charset_adapter.lowercase_only else ch.upper() if charset_adapter.uppercase_only else ch
        out = charset_adapter(ch)
        if len(folded) > 1 or len(out) > 1:            # decided on the fold itself, whatever the test charset then keeps of it
            return None
        if out:
            table[token_id] = ord(out)
    return table


def encode_ground_truth(labels: Sequence[str]) -> np.ndarray:
    """Labels as code points for the device, ONE int32 array so that one upload carries it: [B] lengths, then [B, G] code points
    row by row, padded with 0, G = max(longest label, 1).  `decode_ground_truth` inverts it.  Raises ValueError past MAX_GT."""
    n = len(labels)
    lens = np.fromiter((len(y) for y in labels), dtype=np.int64, count=n)
    width = max(int(lens.max()) if n else 0, 1)
    if width > MAX_GT:
        raise ValueError(f'a label of {width} characters: the metrics kernel takes at most {MAX_GT} code points per label')
    flat = np.fromiter((ord(c) for y in labels for c in y), dtype=np.int32, count=int(lens.sum()))
    out = np.zeros(n + n * width, dtype=np.int32)
    out[:n] = lens
    rows = np.repeat(np.arange(n), lens)
    cols = np.arange(flat.size) - np.repeat(np.cumsum(lens) - lens, lens)
    out[n + rows * width + cols] = flat
    return out


def decode_ground_truth(encoded: np.ndarray, n: int) -> List[str]:
    width = (encoded.size - n) // n if n else 0
    body = encoded[n:].reshape(n, width)
    return [''.join(map(chr, body[i, :encoded[i]])) for i in range(n)]


def _all_reduce_words(ints, floats, process_group):
    """(`ints`, `floats`) summed over the ranks of `process_group` (None = the default group), as lists: one int64 and one float64
    all-reduce of host tensors (works on gloo); an empty side is skipped."""
    import torch.distributed as dist
    out = []
    for words, dtype in ((ints, torch.int64), (floats, torch.float64)):
        words = torch.as_tensor(words, dtype=dtype)
        if words.numel():
            dist.all_reduce(words, group=process_group)
        out.append(words.tolist())
    return out


def _batch_result(n, correct, label_length, ned, confidence, loss_sum, numel, with_loss: bool) -> BatchResult:
    """The greedy totals as a `BatchResult`; with the loss, `loss` is sum(loss * numel) / sum(numel) (base.py:146-164) as a float64 host scalar."""
    if not with_loss:
        return BatchResult(n, correct, ned, confidence, label_length, None, None)
    return BatchResult(n, correct, ned, confidence, label_length, torch.tensor(loss_sum / numel if numel else float('nan'), dtype=torch.float64), numel)


def reduce_result(result: BatchResult, process_group=None) -> BatchResult:
    """Totals summed over the ranks of `process_group` (None = the default group) — what `sync_dist=True` does to the logged values in
    base.py:171-177, applied to the totals so that the quotients are those of the whole job.  Host tensors: works on gloo."""
    loss_sum = float(result.loss) * result.loss_numel if result.loss_numel else 0.0
    (n, correct, label_length, numel), (ned, confidence, loss_sum) = _all_reduce_words(
        [result.num_samples, result.correct, result.label_length, result.loss_numel or 0], [result.ned, result.confidence, loss_sum], process_group)
    return _batch_result(n, correct, label_length, ned, confidence, loss_sum, numel, result.loss_numel is not None)


class _DeviceEvaluator:
    """What `Evaluator`, `BeamEvaluator` and `ErrorAnalysis` share: the system must be on the GPU (there is no CPU path), its adapter as
    a table on the device (`host_path` when it has none: see the module docstring), and the upload of a batch's labels."""

    def __init__(self, system) -> None:
        self.system = system
        self.device = torch.device(system.device)
        if self.device.type != 'cuda':
            raise RuntimeError(f'{type(self).__name__} runs on the GPU (no CPU fallback); move the model to the device first')
        table = adapter_table(system.tokenizer, system.charset_adapter)
        self.host_path = table is None
        self._table = None if self.host_path else torch.from_numpy(table).to(self.device)

    def _upload_labels(self, labels, n: int):
        """`labels` (strings, or the device tensor an earlier upload made of them) as `encode_ground_truth` lays them out, on the device:
        (the whole tensor, its [n] lengths, its code points, G).  One pinned, asynchronous copy."""
        encoded = labels if isinstance(labels, Tensor) else torch.from_numpy(encode_ground_truth(labels)).pin_memory()
        encoded = encoded.to(device=self.device, dtype=torch.int32, non_blocking=True).contiguous()
        return encoded, encoded[:n], encoded[n:], (encoded.numel() - n) // n if n else 0


class Evaluator(_DeviceEvaluator):
    """Running totals of an evaluation over any system with `.forward`, `.tokenizer` and `.charset_adapter` (PARSeq, ViTSTR).

        ev = Evaluator(model)                  # validation=True adds the loss, as validation_step does
        for images, labels in loader:
            ev.update(images, labels)          # enqueues; no device-to-host copy, no synchronisation
        totals = ev.result()                   # BatchResult of sums: the one copy

    The system must be on the GPU when the Evaluator is built (there is no CPU path: RuntimeError otherwise).  `host_path` tells
    whether this model's charsets forced the per-batch host loop (see the module docstring).  `errors`: an `ErrorAnalysis` of the same
    system; every `update` then hands it the ids and lengths the metrics kernel wrote and the uploaded labels, `reset` resets it too.
    `audit`: a `LabelAudit` of the same system; every `update` then scores label and reading of the batch.  It needs
    the device path (ValueError on a model whose charsets select `host_path`)."""

    def __init__(self, system, validation: bool = False, errors: Optional['ErrorAnalysis'] = None, audit: Optional['LabelAudit'] = None) -> None:
        super().__init__(system)
        self.validation, self.errors, self.audit = validation, errors, audit
        if audit is not None and self.host_path:
            raise ValueError('Evaluator(audit=) needs the device path; this model\'s charsets select the host path')
        self._last_rows = None
        self.reset()

    def reset(self) -> None:
        self._host = [0, 0, 0, 0.0, 0.0, 0.0, 0]          # host path: samples, correct, label_length, ned, confidence, loss * numel, numel
        self._last_rows = None
        if self.errors is not None:
            self.errors.reset()
        if self.audit is not None:
            self.audit.reset()
        if not self.host_path:
            self._accum = torch.zeros(5, dtype=torch.int64, device=self.device)          # 3 x int64, then 2 x float64 bit patterns
            self._loss_sum = torch.zeros(1, dtype=torch.float64, device=self.device)
            self._numel = torch.zeros(1, dtype=torch.int64, device=self.device)

    @torch.inference_mode()
    def update(self, images: Tensor, labels: Sequence[str]) -> None:
        if self.host_path:
            self._update_host(images, labels)
            return
        from . import _native
        from .system import forward_logits_loss
        n = len(labels)
        encoded, gt_len, gt, width = self._upload_labels(labels, n)
        if self.validation:
            logits, loss, numel = forward_logits_loss(self.system, images, labels)
            self._loss_sum += loss.double() * numel
            self._numel += numel
        else:
            logits = self.system.forward(images)
        logits = logits.float().contiguous()
        if logits.shape[0] != n:
            raise ValueError(f'{logits.shape[0]} images but {n} labels')
        length, classes = logits.shape[1], logits.shape[2]
        dev = self.device
        ids = torch.empty((n, length), dtype=torch.int32, device=dev)
        lengths = torch.empty((n,), dtype=torch.int32, device=dev)
        conf = torch.empty((n,), dtype=torch.float32, device=dev)
        rows = torch.empty((n, 4), dtype=torch.int32, device=dev)
        ws = torch.empty((n,), dtype=torch.float64, device=dev)
        with _native.guard(dev):
            _native.check(_native.lib().parseq_eval_metrics(
                _native.ptr(logits), n, length, classes, self.system.tokenizer.eos_id, _native.ptr(self._table), _native.ptr(gt),
                _native.ptr(gt_len), width, _native.ptr(ids), _native.ptr(lengths), _native.ptr(conf), _native.ptr(rows), _native.ptr(ws),
                _native.ptr(self._accum), _native.stream_ptr(dev)))
        self._last_rows = rows
        if self.errors is not None:
            self.errors.update_ids(ids, lengths, encoded)
        if self.audit is not None:
            self.audit.update_ids(images, labels, ids, lengths, rows[:, 3])

    def _update_host(self, images: Tensor, labels: Sequence[str]) -> None:
        sink = None if self.errors is None else lambda ids, lengths: self.errors.update_ids(ids, lengths, labels)
        r = eval_step(self.system, (images, labels), self.validation, sink)['output']
        h = self._host
        h[0] += r.num_samples; h[1] += r.correct; h[2] += r.label_length; h[3] += r.ned; h[4] += r.confidence
        if self.validation:
            numel = int(r.loss_numel)
            h[5] += float(r.loss) * numel; h[6] += numel

    def result(self) -> BatchResult:
        """Totals so far.  With validation=True `loss` is sum(loss * numel) / sum(numel) (base.py:146-164) as a float64 host scalar."""
        if self.host_path:
            n, correct, label_length, ned, confidence, loss_sum, numel = self._host
        else:
            packed = torch.cat([self._accum, self._loss_sum.view(torch.int64), self._numel]).cpu()
            n, correct, label_length = packed[:3].tolist()
            ned, confidence, loss_sum = packed[3:6].view(torch.float64).tolist()
            numel = int(packed[6])
        return _batch_result(n, correct, label_length, ned, confidence, loss_sum, numel, self.validation)

    def per_sample(self) -> np.ndarray:
        """The last batch's rows, int32 [B, 4]: length of the adapted prediction, length of the label, edit distance, exact match."""
        if self.host_path:
            raise RuntimeError('per_sample() needs the device path; this model\'s charsets select the host path')
        if self._last_rows is None:
            raise RuntimeError('per_sample() before the first update()')
        return self._last_rows.cpu().numpy()

    def reduce(self, process_group=None) -> BatchResult:
        """`result()` summed over the ranks of `process_group`."""
        return reduce_result(self.result(), process_group)


# -------------------------------------------------------------------------------------------------------------------
# N-best evaluation
# -------------------------------------------------------------------------------------------------------------------
MAX_BEAMS = 17               # PARSEQ_EVAL_MAX_BEAMS: the 16 candidates of a lexicon match plus the reading
NO_HIT = -1                  # image row, word 4: no live hypothesis equals the label
_BEAM_INTS = 8 + MAX_BEAMS   # int64 words of the accumulator; three float64 follow


@dataclass
class BeamEvalResult:
    """Sums over the images of an N-best evaluation (the accumulator of `parseq_eval_beams`) and the quotients derived from them.
    The top-1 of an image is its first live hypothesis; ranks are live ranks, counted from 0 (`first_hit[k]`: images whose first
    exact hypothesis stands at rank k; `miss`: images without one).  The derived values are fractions, not percentages."""
    num_samples: int = 0
    correct: int = 0                     # images whose top-1 equals the label
    label_length_sum: int = 0            # characters of the top-1s
    top1_distance: int = 0               # edit distances of the top-1s
    oracle_correct: int = 0              # images with the label anywhere in the list
    oracle_distance: int = 0             # smallest edit distance over each image's list
    live: int = 0                        # live hypotheses
    miss: int = 0
    first_hit: Tuple[int, ...] = (0,) * MAX_BEAMS
    ned_sum: float = 0.0                 # normalised edit distances of the top-1s
    confidence_sum: float = 0.0          # exp(log-probability) of the top-1s
    oracle_ned_sum: float = 0.0          # smallest normalised edit distance over each image's list

    def _mean(self, total) -> float:
        return total / self.num_samples if self.num_samples else 0.0

    @property
    def accuracy(self) -> float:
        return self._mean(self.correct)

    @property
    def ned(self) -> float:
        """Mean normalised edit distance of the top-1 (the table prints 1 - this)."""
        return self._mean(self.ned_sum)

    @property
    def confidence(self) -> float:
        return self._mean(self.confidence_sum)

    @property
    def label_length(self) -> float:
        return self._mean(self.label_length_sum)

    def hit_at(self, k: int) -> float:
        """Share of the images whose label is among their first `k` live hypotheses."""
        return self._mean(sum(self.first_hit[:max(int(k), 0)]))

    @property
    def oracle_accuracy(self) -> float:
        return self._mean(self.oracle_correct)

    @property
    def oracle_ned(self) -> float:
        return self._mean(self.oracle_ned_sum)

    @property
    def mrr(self) -> float:
        """Mean reciprocal rank of the label (0 for an image without it)."""
        return self._mean(sum(c / (k + 1) for k, c in enumerate(self.first_hit)))

    def _words(self):
        ints = [self.num_samples, self.correct, self.label_length_sum, self.top1_distance, self.oracle_correct, self.oracle_distance, self.live, self.miss]
        return ints + list(self.first_hit), [self.ned_sum, self.confidence_sum, self.oracle_ned_sum]

    @classmethod
    def _from_words(cls, ints, floats) -> 'BeamEvalResult':
        ints = [int(v) for v in ints]
        return cls(*ints[:8], tuple(ints[8:8 + MAX_BEAMS]), *(float(v) for v in floats))


def host_beam_metrics(hypotheses, labels):
    """The definitions of `parseq_eval_beams` on strings: `hypotheses[b]` is image b's slots in order, None for a dead slot, else
    (adapted string, confidence score).  Returns (hypothesis rows [[m, n, distance, exact]], image rows, BeamEvalResult)."""
    import math
    hyp_rows, image_rows = [], []
    ints, first_hit, floats = [0] * 8, [0] * MAX_BEAMS, [0.0, 0.0, 0.0]
    for slots, gt in zip(hypotheses, labels):
        n = len(gt)
        top, hit, live, odist, oned, top_ned, conf = -1, NO_HIT, 0, n, n / max(n, 1), n / max(n, 1), 0.0
        m, dist, exact = 0, n, 0
        for w, slot in enumerate(slots):
            if slot is None:
                hyp_rows.append([-1, -1, -1, 0])
                continue
            s, score = slot
            d = edit_distance(s, gt)
            e = d / max(len(s), n, 1)
            hyp_rows.append([len(s), n, d, int(d == 0)])
            if live == 0:
                top, odist, oned, top_ned, conf = w, d, e, e, math.exp(score)
                m, dist, exact = len(s), d, int(d == 0)
            else:
                odist, oned = min(odist, d), min(oned, e)
            if hit == NO_HIT and d == 0:
                hit = live
            live += 1
        image_rows.append([m, n, dist, exact, hit, odist, live, top])
        for i, v in enumerate((1, exact, m, dist, int(hit != NO_HIT), odist, live, int(hit == NO_HIT))):
            ints[i] += v
        if hit != NO_HIT:
            first_hit[hit] += 1
        floats[0] += top_ned; floats[1] += conf; floats[2] += oned
    return hyp_rows, image_rows, BeamEvalResult._from_words(ints + first_hit, floats)


def reduce_beam_result(result: BeamEvalResult, process_group=None) -> BeamEvalResult:
    """The sums of `result` added over the ranks of `process_group` (None = the default group), as `reduce_result` does for the greedy
    totals: the quotients are then those of the whole job.  Host tensors: works on gloo."""
    return BeamEvalResult._from_words(*_all_reduce_words(*result._words(), process_group))


class BeamEvaluator(_DeviceEvaluator):
    """Running totals of an evaluation of N-best decoding: `Evaluator` for `beam_search` / `lexicon_match` and everything they compose with.

        ev = BeamEvaluator(model, beam_width=5, lexicon=lexicon)      # the search's own keywords
        for images, labels in loader:
            ev.update(images, labels)          # the search, then parseq_eval_beams: enqueues only
        r = ev.result()                        # BeamEvalResult: the one copy

    `match=N` evaluates `lexicon_match(images, lexicon, N, rescore=, keep_reading=, ignore_case=)` instead of a beam search.
    `update_result(result, labels)` takes any BeamResult / LexiconBeamResult / LexiconMatchResult made elsewhere.  What is compared with
    the label is the hypothesis' TOKENS through the test-charset adapter, also under a lexicon (not `lexicon.words[...]`' spelling).  The
    confidence of an image is exp(score) of its first live hypothesis — `model_scores` where the result has them (a weighted automaton's
    `scores` are fused values, no log-probabilities), `scores` otherwise.  The search's refusals pass through unchanged.  `host_path`:
    as `Evaluator`'s, per batch through `decode_beams`."""

    def __init__(self, system, beam_width: int = 5, lexicon=None, roots=None, automaton=None, alpha: float = 1.0, beta: float = 0.0,
                 refine: Optional[str] = None, refine_iters: int = 1, match: Optional[int] = None, rescore: bool = True, keep_reading: bool = False,
                 ignore_case: bool = False) -> None:
        super().__init__(system)
        if match is not None and lexicon is None:
            raise ValueError('BeamEvaluator: match= needs a lexicon')
        self.beam_width, self.match = beam_width, match
        self._search = dict(lexicon=lexicon, roots=roots, automaton=automaton, alpha=alpha, beta=beta, refine=refine, refine_iters=refine_iters)
        self._match = dict(rescore=rescore, keep_reading=keep_reading, ignore_case=ignore_case)
        self.reset()

    def reset(self) -> None:
        self._host = BeamEvalResult()
        self._last = None
        if not self.host_path:
            self._accum = torch.zeros(_BEAM_INTS + 3, dtype=torch.int64, device=self.device)      # 25 x int64, then 3 x float64 bit patterns

    @torch.inference_mode()
    def update(self, images: Tensor, labels: Sequence[str]) -> None:
        if images.shape[0] != len(labels):
            raise ValueError(f'{images.shape[0]} images but {len(labels)} labels')
        if self.match is not None:
            result = self.system.lexicon_match(images, self._search['lexicon'], self.match, **self._match)
        else:
            result = self.system.beam_search(images, self.beam_width, **self._search)
        self.update_result(result, labels)

    @torch.inference_mode()
    def update_result(self, result, labels: Sequence[str]) -> None:
        n = len(labels)
        if result.tokens.dim() != 3 or result.tokens.shape[0] != n:
            raise ValueError(f'a result of shape {tuple(result.tokens.shape)} but {n} labels')
        if self.host_path:
            self._update_host(result, labels)
            return
        from . import _native
        dev = self.device
        _, gt_len, gt, gt_width = self._upload_labels(labels, n)
        _, width, steps = result.tokens.shape
        tokens = result.tokens.to(torch.int32).contiguous()
        scores = result.scores.to(torch.float32).contiguous()
        lengths = result.lengths.to(torch.int32).contiguous()
        conf = scores if result.model_scores is None else result.model_scores.to(torch.float32).contiguous()
        hyp_rows = torch.empty((n * width, 4), dtype=torch.int32, device=dev)
        image_rows = torch.empty((n, 8), dtype=torch.int32, device=dev)
        ws = torch.empty((n * (width + 3),), dtype=torch.float64, device=dev)
        with _native.guard(dev):
            _native.check(_native.lib().parseq_eval_beams(
                _native.ptr(tokens), _native.ptr(scores), _native.ptr(lengths), _native.ptr(conf), n, width, steps, self._table.numel(),
                _native.ptr(self._table), _native.ptr(gt), _native.ptr(gt_len), gt_width, _native.ptr(hyp_rows), _native.ptr(image_rows),
                _native.ptr(ws), _native.ptr(self._accum), _native.stream_ptr(dev)))
        self._last = (hyp_rows, image_rows, width)

    def _update_host(self, result, labels: Sequence[str]) -> None:
        tokenizer, adapter = self.system.tokenizer, self.system.charset_adapter
        beams = tokenizer.decode_beams(result)                   # the tokens' characters, live slots only, in order
        packed = torch.stack([result.scores.float(), (result.scores if result.model_scores is None else result.model_scores).float()]).cpu()
        live, conf = (packed[0] != float('-inf')).tolist(), packed[1].tolist()
        hypotheses = []
        for alts, live_row, conf_row in zip(beams, live, conf):
            strings = iter(alts)
            hypotheses.append([(adapter(next(strings)[0]), c) if on else None for on, c in zip(live_row, conf_row)])
        hyp_rows, image_rows, r = host_beam_metrics(hypotheses, labels)
        ints, floats = self._host._words()
        more_ints, more_floats = r._words()
        self._host = BeamEvalResult._from_words([a + b for a, b in zip(ints, more_ints)], [a + b for a, b in zip(floats, more_floats)])
        self._last = (np.asarray(hyp_rows, dtype=np.int32).reshape(-1, 4), np.asarray(image_rows, dtype=np.int32).reshape(-1, 8), result.tokens.shape[1])

    def result(self) -> BeamEvalResult:
        """Totals so far: one copy of 224 bytes."""
        if self.host_path:
            return self._host
        packed = self._accum.cpu()
        return BeamEvalResult._from_words(packed[:_BEAM_INTS].tolist(), packed[_BEAM_INTS:].view(torch.float64).tolist())

    def _rows(self, which: int, what: str):
        if self._last is None:
            raise RuntimeError(f'{what}() before the first update()')
        rows = self._last[which]
        return rows if isinstance(rows, np.ndarray) else rows.cpu().numpy()

    def per_sample(self) -> np.ndarray:
        """The last batch's image rows, int32 [B, 8]: length of the top-1 (the first live hypothesis), length of the label, their edit distance,
        exact match, live rank of the first exact hypothesis (-1: none), smallest edit distance in the list, live hypotheses, the top-1's slot
        (-1: every slot dead; the image then reads as the empty string)."""
        return self._rows(1, 'per_sample')

    def per_hypothesis(self) -> np.ndarray:
        """The last batch's hypothesis rows, int32 [B, W, 4]: length of the adapted hypothesis, length of the label, edit distance, exact match;
        a dead slot's row is [-1, -1, -1, 0]."""
        return self._rows(0, 'per_hypothesis').reshape(-1, self._last[2], 4)

    def reduce(self, process_group=None) -> BeamEvalResult:
        """`result()` summed over the ranks of `process_group` (None = the default group).  Host tensors: works on gloo."""
        return reduce_beam_result(self.result(), process_group)


# -------------------------------------------------------------------------------------------------------------------
# Error analysis
# -------------------------------------------------------------------------------------------------------------------
MAX_SYMBOLS = 512            # PARSEQ_EVAL_MAX_SYMBOLS
SCRIPT_WIDTH = MAX_GT + 32   # PARSEQ_EVAL_SCRIPT_WIDTH
LEN_BINS = 33                # rows of by_length / by_position: 0 .. 31, then "32 and more"
MATCH, SUBSTITUTION, INSERTION, DELETION = range(4)      # the codes of an edit script
_HEAD, _BY_LENGTH, _BY_POSITION, _CONFUSION = 0, 8, 8 + LEN_BINS * 4, 8 + 2 * LEN_BINS * 4      # int64 words of the accumulator
OTHER, NONE = '<other>', '<none>'                        # what `ErrorReport` calls symbol T and symbol T + 1


def symbol_table(adapter_table) -> np.ndarray:
    """int32, strictly ascending: the distinct code points a prediction can consist of under `adapter_table`."""
    table = np.asarray(adapter_table)
    return np.unique(table[table >= 0]).astype(np.int32)


def host_edit_script(pred: str, gt: str) -> List[int]:
    """The canonical edit script of DESIGN.md section 28 in forward order: 0 match, 1 substitution, 2 insertion (a character of `pred` that
    answers to none of `gt`), 3 deletion (a character of `gt` nothing was predicted for).  Plain Python over the full table."""
    m, n = len(pred), len(gt)
    table = [list(range(n + 1))]
    for i in range(1, m + 1):
        above, row = table[-1], [i]
        for j in range(1, n + 1):
            row.append(min(above[j - 1] + (pred[i - 1] != gt[j - 1]), above[j] + 1, row[j - 1] + 1))
        table.append(row)
    script, i, j = [], m, n
    while i or j:
        if i and j and table[i - 1][j - 1] + (pred[i - 1] != gt[j - 1]) == table[i][j]:
            script.append(SUBSTITUTION if pred[i - 1] != gt[j - 1] else MATCH)
            i, j = i - 1, j - 1
        elif i and table[i - 1][j] + 1 == table[i][j]:
            script.append(INSERTION)
            i -= 1
        else:
            script.append(DELETION)
            j -= 1
    return script[::-1]


def _accumulate_script(words: np.ndarray, index: dict, script: Sequence[int], pred: str, gt: str) -> None:
    """One sample into the flat int64 accumulator `words` (the layout of `parseq_eval_errors`); `index`: character -> symbol index."""
    t = len(index)
    confusion = words[_CONFUSION:].reshape(t + 2, t + 2)
    by_position = words[_BY_POSITION:_CONFUSION].reshape(LEN_BINS, 4)
    i = j = 0
    for code in script:
        at = by_position[min(j, LEN_BINS - 1)]
        row = t + 1 if code == INSERTION else index.get(gt[j], t)
        col = t + 1 if code == DELETION else index.get(pred[i], t)
        confusion[row, col] += 1
        words[_HEAD + 1 + code] += 1
        if code != INSERTION:
            at[0] += 1
        if code:
            at[{SUBSTITUTION: 1, DELETION: 2, INSERTION: 3}[code]] += 1
        i += code != DELETION
        j += code != INSERTION
    distance = sum(1 for code in script if code)
    words[_HEAD] += 1
    words[_HEAD + 5] += distance == 0
    words[_BY_LENGTH:_BY_POSITION].reshape(LEN_BINS, 4)[min(len(gt), LEN_BINS - 1)] += (1, distance == 0, distance, len(gt))


def host_error_tables(preds: Sequence[str], labels: Sequence[str], symbols: Sequence[str]) -> 'ErrorReport':
    """The tables of `parseq_eval_errors` for adapted predictions and labels given as strings: `host_edit_script` per pair."""
    index = {ch: i for i, ch in enumerate(symbols)}
    words = np.zeros(_CONFUSION + (len(index) + 2) ** 2, dtype=np.int64)
    for pred, gt in zip(preds, labels):
        _accumulate_script(words, index, host_edit_script(pred, gt), pred, gt)
    return ErrorReport._from_words(symbols, words)


@dataclass
class ErrorReport:
    """The tables of an error analysis as numpy int64 arrays, and the symbols they are indexed by as characters.
    `head` = [samples, matches, substitutions, insertions, deletions, exact, 0, 0]; `by_length[min(n, 32)]` = [samples, exact, distance,
    label characters] of the labels of n characters; `by_position[min(j, 32)]` = [label characters at position j, substitutions, deletions,
    insertions] (an insertion's position is the number of label characters before it); `confusion[label][predicted]` over the T symbols,
    then `OTHER` (a label character outside them) and `NONE` (the missing side of an insertion or deletion)."""
    symbols: List[str]
    head: np.ndarray
    by_length: np.ndarray
    by_position: np.ndarray
    confusion: np.ndarray

    @classmethod
    def _from_words(cls, symbols: Sequence[str], words) -> 'ErrorReport':
        words, t = np.asarray(words, dtype=np.int64), len(symbols)
        return cls(list(symbols), words[:_BY_LENGTH].copy(), words[_BY_LENGTH:_BY_POSITION].reshape(LEN_BINS, 4).copy(),
                   words[_BY_POSITION:_CONFUSION].reshape(LEN_BINS, 4).copy(), words[_CONFUSION:].reshape(t + 2, t + 2).copy())

    def _words(self) -> np.ndarray:
        return np.concatenate([self.head.ravel(), self.by_length.ravel(), self.by_position.ravel(), self.confusion.ravel()]).astype(np.int64)

    samples = property(lambda self: int(self.head[0]))
    matches = property(lambda self: int(self.head[1]))
    substitutions = property(lambda self: int(self.head[2]))
    insertions = property(lambda self: int(self.head[3]))
    deletions = property(lambda self: int(self.head[4]))
    exact = property(lambda self: int(self.head[5]))

    def __add__(self, other: 'ErrorReport') -> 'ErrorReport':
        if self.symbols != other.symbols:
            raise ValueError('reports over different symbol sets do not add')
        return ErrorReport._from_words(self.symbols, self._words() + other._words())

    def __eq__(self, other) -> bool:
        return isinstance(other, ErrorReport) and self.symbols == other.symbols and np.array_equal(self._words(), other._words())

    def name(self, index: int) -> str:
        t = len(self.symbols)
        return self.symbols[index] if index < t else OTHER if index == t else NONE

    def _top(self, cells: np.ndarray, k: int):
        """(flat index, count) of the `k` largest positive cells, ties in index order."""
        flat = cells.ravel()
        order = np.argsort(-flat, kind='stable')[:max(int(k), 0)]
        return [(int(i), int(flat[i])) for i in order if flat[i] > 0]

    def top_confusions(self, k: int) -> List[Tuple[str, str, int]]:
        """(label character, predicted character, count) of the `k` most frequent substitutions; ties by (label, predicted) index."""
        t = len(self.symbols)
        cells = self.confusion[:t + 1, :t + 1].copy()
        cells[np.arange(t), np.arange(t)] = 0
        return [(self.name(i // (t + 1)), self.name(i % (t + 1)), c) for i, c in self._top(cells, k)]

    def top_deleted(self, k: int) -> List[Tuple[str, int]]:
        """(label character, count) of the `k` label characters most often left unread."""
        t = len(self.symbols)
        return [(self.name(i), c) for i, c in self._top(self.confusion[:t + 1, t + 1], k)]

    def top_inserted(self, k: int) -> List[Tuple[str, int]]:
        """(predicted character, count) of the `k` characters most often read where the label has none."""
        t = len(self.symbols)
        return [(self.name(i), c) for i, c in self._top(self.confusion[t + 1, :t + 1], k)]

    def accuracy_by_length(self) -> List[Tuple[int, int, float]]:
        """(label length, samples, share read exactly) for every length that occurs; the last row, 32, holds every longer label."""
        return [(n, int(r[0]), int(r[1]) / int(r[0])) for n, r in enumerate(self.by_length) if r[0]]

    def error_rate_by_position(self) -> List[Tuple[int, int, float, int]]:
        """(position, label characters there, share of them substituted or deleted, insertions in front of that position) for every
        position that occurs; the last row, 32, holds every later one."""
        return [(j, int(r[0]), (int(r[1]) + int(r[2])) / int(r[0]) if r[0] else 0.0, int(r[3])) for j, r in enumerate(self.by_position) if r[0] or r[3]]

    def to_dict(self) -> dict:
        return dict(symbols=list(self.symbols), head=self.head.tolist(), by_length=self.by_length.tolist(), by_position=self.by_position.tolist(),
                    confusion=self.confusion.tolist())

    @classmethod
    def from_dict(cls, d: dict) -> 'ErrorReport':
        return cls(list(d['symbols']), *(np.asarray(d[key], dtype=np.int64) for key in ('head', 'by_length', 'by_position', 'confusion')))

    def to_json(self) -> str:
        import json
        return json.dumps(self.to_dict(), ensure_ascii=False)

    @classmethod
    def from_json(cls, text: str) -> 'ErrorReport':
        import json
        return cls.from_dict(json.loads(text))


def reduce_report(report: ErrorReport, process_group=None) -> ErrorReport:
    """The tables of `report` added over the ranks of `process_group` (None = the default group), as `reduce_result` does for the totals.
    One int64 all-reduce of a host tensor: works on gloo.  The ranks must analyse the same symbol set."""
    return ErrorReport._from_words(report.symbols, _all_reduce_words(report._words(), [], process_group)[0])


def _host_symbols(tokenizer, charset_adapter) -> List[str]:
    """The characters a prediction can consist of when the adapter is no per-character map (the host path): whatever it makes of each
    train character alone and doubled (a doubled 'Σ' lower-cases to both of its forms)."""
    classes = len(tokenizer) - 2
    chars = set()
    for token_id in range(classes):
        if token_id != tokenizer.eos_id:
            ch = tokenizer._itos[token_id]
            chars.update(charset_adapter(ch), charset_adapter(ch + ch))
    return sorted(chars)


class ErrorAnalysis(_DeviceEvaluator):
    """Running edit scripts and error tables of an evaluation, beside `Evaluator`'s totals:

        errors = ErrorAnalysis(model)
        ev = Evaluator(model, errors=errors)
        for images, labels in loader:
            ev.update(images, labels)          # the metrics, then parseq_eval_errors on the ids they wrote: enqueues only
        report = errors.result()               # ErrorReport: the one copy

    `update_ids(ids, lengths, labels)` takes the device tensors of any greedy decode (`parseq_postprocess`) directly.  A model whose
    charsets select `host_path` (see the module docstring) is analysed by `host_edit_script` per sample: the same tables."""

    def __init__(self, system) -> None:
        super().__init__(system)
        self.symbols = _host_symbols(system.tokenizer, system.charset_adapter) if self.host_path else [chr(c) for c in symbol_table(self._table.cpu().numpy())]
        if not 1 <= len(self.symbols) <= MAX_SYMBOLS:
            raise ValueError(f'{len(self.symbols)} symbols: the error analysis takes 1 to {MAX_SYMBOLS}')
        self._words = _CONFUSION + (len(self.symbols) + 2) ** 2
        if self.host_path:
            self._index = {ch: i for i, ch in enumerate(self.symbols)}
        else:
            self._symbols = torch.tensor([ord(ch) for ch in self.symbols], dtype=torch.int32).to(self.device)
        self.reset()

    def reset(self) -> None:
        self._last = None
        if self.host_path:
            self._host = np.zeros(self._words, dtype=np.int64)
        else:
            self._accum = torch.zeros(self._words, dtype=torch.int64, device=self.device)

    @torch.inference_mode()
    def update_ids(self, ids: Tensor, lengths: Tensor, labels) -> None:
        """`ids` int32 [B, L] and `lengths` int32 [B] on the device, as `parseq_postprocess` / `parseq_eval_metrics` write them; `labels`:
        the strings, or the device tensor `encode_ground_truth` made of them (what `Evaluator` has uploaded already)."""
        n, length = ids.shape
        if lengths.shape[0] != n:
            raise ValueError(f'{n} rows of ids but {lengths.shape[0]} lengths')
        if isinstance(labels, Tensor):
            if n == 0 or labels.numel() % n or labels.numel() < 2 * n:
                raise ValueError(f'an encoded label tensor of {labels.numel()} words for {n} samples')
        elif len(labels) != n:
            raise ValueError(f'{n} rows of ids but {len(labels)} labels')
        if self.host_path:
            self._update_host(ids, lengths, labels)
            return
        from . import _native
        dev = self.device
        _, gt_len, gt, width = self._upload_labels(labels, n)
        ids, lengths = ids.to(device=dev, dtype=torch.int32).contiguous(), lengths.to(device=dev, dtype=torch.int32).contiguous()
        scripts = torch.empty((n, SCRIPT_WIDTH), dtype=torch.int8, device=dev)
        script_len = torch.empty((n,), dtype=torch.int32, device=dev)
        rows = torch.empty((n, 4), dtype=torch.int32, device=dev)
        with _native.guard(dev):
            _native.check(_native.lib().parseq_eval_errors(
                _native.ptr(ids), _native.ptr(lengths), n, length, self._table.numel(), _native.ptr(self._table), _native.ptr(self._symbols),
                len(self.symbols), _native.ptr(gt), _native.ptr(gt_len), width, _native.ptr(scripts), _native.ptr(script_len), _native.ptr(rows),
                _native.ptr(self._accum), _native.stream_ptr(dev)))
        self._last = (scripts, script_len, rows)

    def _update_host(self, ids: Tensor, lengths: Tensor, labels) -> None:
        tokenizer, adapter = self.system.tokenizer, self.system.charset_adapter
        if isinstance(labels, Tensor):
            labels = decode_ground_truth(labels.cpu().numpy(), ids.shape[0])
        classes = len(tokenizer) - 2
        n, length = ids.shape
        scripts = np.full((n, SCRIPT_WIDTH), -1, dtype=np.int8)
        script_len, rows = np.zeros(n, dtype=np.int32), np.zeros((n, 4), dtype=np.int32)
        for b, (row, k, gt) in enumerate(zip(ids.cpu().numpy(), lengths.cpu().tolist(), labels)):
            kept = [int(i) for i in row[:min(max(k, 0), length)] if 0 <= i < classes and i != tokenizer.eos_id]
            pred = adapter(tokenizer._ids2tok(kept))
            script = host_edit_script(pred, gt)
            _accumulate_script(self._host, self._index, script, pred, gt)
            distance = sum(1 for code in script if code)
            scripts[b, :len(script)] = script
            script_len[b], rows[b] = len(script), (len(pred), len(gt), distance, distance == 0)
        self._last = (scripts, script_len, rows)

    def result(self) -> ErrorReport:
        """The tables so far: one copy of 8 * (272 + (T + 2) ** 2) bytes."""
        return ErrorReport._from_words(self.symbols, self._host if self.host_path else self._accum.cpu().numpy())

    def per_sample(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        """The last batch's (scripts int8 [B, 288] in forward order, padded with -1; script lengths int32 [B]; rows int32 [B, 4] = length of the
        adapted prediction, length of the label, edit distance, exact match)."""
        if self._last is None:
            raise RuntimeError('per_sample() before the first update_ids()')
        return tuple(t if isinstance(t, np.ndarray) else t.cpu().numpy() for t in self._last)

    def reduce(self, process_group=None) -> ErrorReport:
        """`result()` summed over the ranks of `process_group`."""
        return reduce_report(self.result(), process_group)


# -------------------------------------------------------------------------------------------------------------------
# label audit
# -------------------------------------------------------------------------------------------------------------------
@dataclass
class AuditReport:
    """What a `LabelAudit` has seen, on the host.  Per sample, in the order of the updates: the label, the raw reading (the training
    charset's characters, before the test-charset adapter), whether the adapted reading differs from the label, and — where it does and
    both strings can be scored — the two log-probabilities; `suspicion` = score(reading) - score(label), NaN elsewhere.  `unscorable`:
    mismatching samples whose label the training charset cannot spell (or whose reading has no <eos>)."""
    labels: List[str]
    readings: List[str]
    mismatch: np.ndarray           # bool [S]
    label_scores: np.ndarray       # float32 [S]
    reading_scores: np.ndarray     # float32 [S]
    suspicion: np.ndarray          # float32 [S], NaN where nothing was compared
    unscorable: int

    def top(self, k: int) -> List[dict]:
        """The `k` most suspicious samples: suspicion descending, then the sample index."""
        idx = [i for i in range(len(self.labels)) if not np.isnan(self.suspicion[i])]
        idx.sort(key=lambda i: (-float(self.suspicion[i]), i))
        return [dict(index=i, label=self.labels[i], reading=self.readings[i], label_score=float(self.label_scores[i]),
                     reading_score=float(self.reading_scores[i]), suspicion=float(self.suspicion[i])) for i in idx[:max(int(k), 0)]]


class LabelAudit:
    """Which labels does the model disagree with most?  Beside an `Evaluator`:

        audit = LabelAudit(model)                      # orders / combine / normalize as `PARSeq.score` takes them
        ev = Evaluator(model, audit=audit)
        for images, labels in loader:
            ev.update(images, labels)                  # the metrics, then ONE `score` call with N = 2 (label, raw reading): enqueues only
        report = audit.result()                        # AuditReport: the one copy
        report.top(20)

    The score call covers the whole batch — which samples mismatch is known on the device only, and asking would be a host
    synchronisation — and the suspicion of a sample whose adapted reading equals its label is masked to NaN there.  The candidates are
    L = max_label_length + 1 wide whatever the batch holds, so one mask upload serves every update."""

    def __init__(self, system, orders='forward', combine: str = 'mix', normalize: bool = False, seed: Optional[int] = None) -> None:
        from . import score as _score
        self.system = system
        self._flags = _score.score_flags(combine, normalize)
        self._T = system.model.max_label_length
        self.perms = _score.parse_orders(orders, self._T, system, seed)
        self._masks = None
        self.reset()

    def reset(self) -> None:
        self._labels: List[str] = []
        self._parts = []           # per update: (label score, reading score, mismatch & scorable, mismatch, reading ids, reading lengths)

    def label_rows(self, labels: Sequence[str]) -> Tuple[np.ndarray, np.ndarray]:
        """(int32 [B, L] candidate rows of the labels — an absent row for one the training charset cannot spell —, bool [B] scorable)."""
        tok = self.system.tokenizer
        L = self._T + 1
        rows = np.full((len(labels), L), tok.pad_id, dtype=np.int32)
        ok = np.zeros(len(labels), dtype=bool)
        specials = (tok.BOS, tok.EOS, tok.PAD)
        for b, y in enumerate(labels):
            if len(y) <= self._T and all(ch in tok._stoi and ch not in specials for ch in y):
                rows[b, :len(y)] = [tok._stoi[ch] for ch in y]
                rows[b, len(y)] = tok.eos_id
                ok[b] = True
        return rows, ok

    def reading_rows(self, ids: Tensor, lengths: Tensor) -> Tensor:
        """The greedy readings (`ids` int32 [B, P], `lengths` int32 [B]: the index of the first <eos>, P without one) as candidate rows
        int32 [B, L], with torch operations on whatever device holds them.  A reading without <eos> gives a row without one: invalid."""
        tok = self.system.tokenizer
        B, P = ids.shape
        L = self._T + 1
        pos = torch.arange(L, device=ids.device).unsqueeze(0)
        n = lengths.to(torch.int64).clamp(0, P).unsqueeze(1)
        body = torch.full((B, L), tok.pad_id, dtype=torch.int32, device=ids.device)
        body[:, :min(P, L)] = ids[:, :L].to(torch.int32)
        eos = torch.full_like(body, tok.eos_id)
        pad = torch.full_like(body, tok.pad_id)
        return torch.where(pos < n, body, torch.where(pos == n, eos, pad))

    def add_scores(self, labels: Sequence[str], scores: Tensor, valid: Tensor, mismatch: Tensor, reading_ids: Tensor,
                   reading_lengths: Tensor) -> None:
        """The bookkeeping of one batch, no copy: `scores` fp32 [B, 2] and `valid` [B, 2] of the (label, reading) candidates, `mismatch` [B]
        (the adapted reading differs from the label), on any one device."""
        self._labels += list(labels)
        both = (valid[:, 0] != 0) & (valid[:, 1] != 0)
        mismatch = mismatch.to(torch.bool)
        self._parts.append((scores[:, 0].float(), scores[:, 1].float(), mismatch & both, mismatch, reading_ids.to(torch.int32), reading_lengths.to(torch.int32)))

    @torch.inference_mode()
    def update_ids(self, images: Tensor, labels: Sequence[str], ids: Tensor, lengths: Tensor, exact: Tensor) -> None:
        """`ids`, `lengths`: what the metrics kernel (or `parseq_postprocess`) wrote for `images`; `exact` [B]: non-zero where the adapted
        reading equals the label.  One `score` call on (label, raw reading) per sample."""
        from . import score as _score
        dev = images.device
        if self._masks is None or self._masks.device != dev:
            self._masks = _score.query_masks(self.perms).to(dev)
        rows, _ = self.label_rows(labels)
        cand = torch.stack([torch.from_numpy(rows).pin_memory().to(dev, non_blocking=True), self.reading_rows(ids, lengths)], dim=1).contiguous()
        scores, _, _, _, _, valid = self.system.model.score(self.system.tokenizer, images, cand, self._masks, self._flags, char_logprobs=False)
        self.add_scores(labels, scores, valid, exact == 0, ids, lengths)

    def result(self) -> AuditReport:
        """Everything so far: one copy."""
        tok = self.system.tokenizer
        if not self._parts:
            return AuditReport([], [], np.zeros(0, bool), np.zeros(0, np.float32), np.zeros(0, np.float32), np.zeros(0, np.float32), 0)
        width = max(p[4].shape[1] for p in self._parts)
        packed = torch.cat([torch.cat([p[0].view(-1, 1).contiguous().view(torch.int32), p[1].view(-1, 1).contiguous().view(torch.int32),
                                       p[2].view(-1, 1).to(torch.int32), p[3].view(-1, 1).to(torch.int32), p[5].view(-1, 1),
                                       torch.nn.functional.pad(p[4], (0, width - p[4].shape[1]), value=tok.pad_id)], dim=1) for p in self._parts]).cpu()
        label_scores = packed[:, 0].contiguous().view(torch.float32).numpy()
        reading_scores = packed[:, 1].contiguous().view(torch.float32).numpy()
        compared, mismatch = packed[:, 2].numpy().astype(bool), packed[:, 3].numpy().astype(bool)
        lengths, ids = packed[:, 4].tolist(), packed[:, 5:].numpy()
        classes = len(tok) - 2
        readings = [tok._ids2tok([int(i) for i in row[:min(max(k, 0), width)] if 0 <= i < classes and i != tok.eos_id]) for row, k in zip(ids, lengths)]
        with np.errstate(invalid='ignore'):
            suspicion = np.where(compared, reading_scores - label_scores, np.float32('nan')).astype(np.float32)
        return AuditReport(list(self._labels), readings, mismatch, label_scores, reading_scores, suspicion, int((mismatch & ~compared).sum()))

    def top(self, k: int) -> List[dict]:
        return self.result().top(k)
