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

Limits: a label of at most `MAX_GT` = 256 code points (the reference's dataset drops labels longer than `max_label_length`,
25 by default, before they get here: strhub/data/dataset.py:111-113); predictions of at most 32 positions (DEC_MAXL).
"""
from __future__ import annotations

from typing import List, Optional, Sequence

import numpy as np
import torch
from torch import Tensor

from .system import BatchResult, eval_step

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


def reduce_result(result: BatchResult, process_group=None) -> BatchResult:
    """Totals summed over the ranks of `process_group` (None = the default group) — what `sync_dist=True` does to the logged values in
    base.py:171-177, applied to the totals so that the quotients are those of the whole job.  Host tensors: works on gloo."""
    import torch.distributed as dist
    ints = torch.tensor([result.num_samples, result.correct, result.label_length, result.loss_numel or 0], dtype=torch.int64)
    loss_sum = float(result.loss) * result.loss_numel if result.loss_numel else 0.0
    floats = torch.tensor([result.ned, result.confidence, loss_sum], dtype=torch.float64)
    dist.all_reduce(ints, group=process_group)
    dist.all_reduce(floats, group=process_group)
    n, correct, label_length, numel = ints.tolist()
    ned, confidence, loss_sum = floats.tolist()
    if result.loss_numel is None:
        return BatchResult(n, correct, ned, confidence, label_length, None, None)
    return BatchResult(n, correct, ned, confidence, label_length, torch.tensor(loss_sum / numel if numel else float('nan'), dtype=torch.float64), numel)


class Evaluator:
    """Running totals of an evaluation over any system with `.forward`, `.tokenizer` and `.charset_adapter` (PARSeq, ViTSTR).

        ev = Evaluator(model)                  # validation=True adds the loss, as validation_step does
        for images, labels in loader:
            ev.update(images, labels)          # enqueues; no device-to-host copy, no synchronisation
        totals = ev.result()                   # BatchResult of sums: the one copy

    The system must be on the GPU when the Evaluator is built (there is no CPU path: RuntimeError otherwise).  `host_path` tells
    whether this model's charsets forced the per-batch host loop (see the module docstring)."""

    def __init__(self, system, validation: bool = False) -> None:
        self.system, self.validation = system, validation
        self.device = torch.device(system.device)
        if self.device.type != 'cuda':
            raise RuntimeError('Evaluator runs on the GPU (no CPU fallback); move the model to the device first')
        table = adapter_table(system.tokenizer, system.charset_adapter)
        self.host_path = table is None
        self._table = None if self.host_path else torch.from_numpy(table).to(self.device)
        self._last_rows = None
        self.reset()

    def reset(self) -> None:
        self._host = [0, 0, 0, 0.0, 0.0, 0.0, 0]          # host path: samples, correct, label_length, ned, confidence, loss * numel, numel
        self._last_rows = None
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
        encoded = torch.from_numpy(encode_ground_truth(labels)).pin_memory().to(self.device, non_blocking=True)
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
        width = (encoded.numel() - n) // n
        with _native.guard(dev):
            _native.check(_native.lib().parseq_eval_metrics(
                _native.ptr(logits), n, length, classes, self.system.tokenizer.eos_id, _native.ptr(self._table), _native.ptr(encoded[n:]),
                _native.ptr(encoded), width, _native.ptr(ids), _native.ptr(lengths), _native.ptr(conf), _native.ptr(rows), _native.ptr(ws),
                _native.ptr(self._accum), _native.stream_ptr(dev)))
        self._last_rows = rows

    def _update_host(self, images: Tensor, labels: Sequence[str]) -> None:
        r = eval_step(self.system, (images, labels), self.validation)['output']
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
        if not self.validation:
            return BatchResult(n, correct, ned, confidence, label_length, None, None)
        return BatchResult(n, correct, ned, confidence, label_length, torch.tensor(loss_sum / numel if numel else float('nan'), dtype=torch.float64), numel)

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
