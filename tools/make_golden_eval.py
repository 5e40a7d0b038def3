#!/usr/bin/env python3
"""Mint golden vectors for the evaluation metrics (`parseq_eval_metrics`, parseq_amd/evaluate.py).   *** TEST INFRASTRUCTURE ***

The expected totals come from the reference's own `BaseSystem._eval_step` (strhub/models/base.py:112-143), loaded under the
stubs of oracle/make_golden_train.py (imported unchanged) with `forward` pointed at stored logits.  nltk is not installed where
this runs, so the stubbed `nltk.edit_distance` is replaced by the textbook two-row dynamic programme below (unit costs, no
transpositions: nltk's defaults); the json says so.  Runs in the build container only (needs the reference checkout).

Cases (charset_train / charset_test): 94 / 36 (lower-casing and dropped punctuation), 94 / 94, 36 / 36, and the 200-character
charset of tests/golden/parseq_c200.json against its lower-case form.  Each row's logits are peaked at a mutated copy of its
label — equal, case-flipped, punctuation inserted, substitution, insertion, deletion, empty prediction, no <eos> at all — over
noise.  Logits are stored as int8 `q` with logits = q * 0.25 exactly (a quarter of the bytes of fp32; the reference is fed
the fp32 values).  No row has both an empty adapted prediction and an empty label: the reference divides by zero there (asserted).

Confidence.  Two fp32 soft-max implementations (torch's on the CPU here, the post-processing kernel on the device) differ by rounding,
about 1e-7 relative per probability — a hundred times the 1e-9 the totals are held to.  So the logits are built to make every
winning probability exactly representable however it is computed: the peak is 31.75, every other class is at most -0.5 (their
exponentials sum to under 1e-11, far below half an ulp of 1), except that a position may repeat the peak VALUE at 1 or 3 classes of
HIGHER index (first maximum wins in torch.max and in the kernel), which makes its probability exactly 1/2 or 1/4.  A row's confidence
is then an exact power of two that depends on the cut keeping the <eos> probability and ignoring every position after it.

Usage:  python tools/make_golden_eval.py --ref <reference checkout> [--out tests/golden]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle.make_golden_train import install_stubs  # noqa: E402
from oracle.synth import CHARSET_36, CHARSET_200  # noqa: E402
from parseq_amd.configs import CHARSET_94_FULL  # noqa: E402

SCALE = 0.25
MAX_LABEL_LENGTH = 12                     # 13 positions per row
# name -> (charset_train, charset_test, rows)
CASES = {
    'c94_c36': (CHARSET_94_FULL, CHARSET_36, 24),
    'c94_c94': (CHARSET_94_FULL, CHARSET_94_FULL, 24),
    'c36_c36': (CHARSET_36, CHARSET_36, 24),
    'c200_c174': (CHARSET_200, CHARSET_36 + CHARSET_200[62:], 16),
}
KINDS = ('equal', 'case', 'punct', 'substitute', 'insert', 'delete', 'empty', 'no_eos')


def two_row_edit_distance(a, b):
    """Levenshtein distance by the textbook dynamic programme, two rows of the table at a time."""
    prev = list(range(len(b) + 1))
    for i in range(1, len(a) + 1):
        cur = [i] + [0] * len(b)
        for j in range(1, len(b) + 1):
            cur[j] = min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (0 if a[i - 1] == b[j - 1] else 1))
        prev = cur
    return prev[len(b)]


def mutate(label, kind, train, rng, positions):
    """A prediction (characters of the train charset, or None for "no <eos>": then every position holds a character)."""
    chars = list(label)
    others = [c for c in train if c not in label]
    at = int(rng.integers(len(chars)))
    if kind == 'case':
        chars = [c.upper() if c.upper() in train and len(c.upper()) == 1 else c for c in chars]
    elif kind == 'punct':
        marks = [c for c in train if not c.isalnum()] or others
        chars.insert(at, marks[int(rng.integers(len(marks)))])
    elif kind == 'substitute':
        chars[at] = others[int(rng.integers(len(others)))]
    elif kind == 'insert':
        chars.insert(at, others[int(rng.integers(len(others)))])
    elif kind == 'delete':
        del chars[at]
    elif kind == 'empty':
        chars = []
    elif kind == 'no_eos':
        while len(chars) < positions:
            chars.append(train[int(rng.integers(len(train)))])
    return ''.join(c for c in chars if c in train)[:positions if kind == 'no_eos' else positions - 1], kind != 'no_eos'


def make_case(name, train, test, rows, ref_tokenizer, adapter):
    rng = np.random.default_rng(sum(map(ord, name)))
    positions = MAX_LABEL_LENGTH + 1
    classes = len(ref_tokenizer) - 2
    usable = [c for c in test if adapter(c) == c and c in train]
    q = rng.integers(-128, -1, size=(rows, positions, classes), dtype=np.int64)          # -32 .. -0.5
    labels, kinds = [], []
    for r in range(rows):
        kind = KINDS[r % len(KINDS)]
        n = int(rng.integers(2, MAX_LABEL_LENGTH - 1))
        label = ''.join(usable[int(rng.integers(len(usable)))] for _ in range(n))
        pred, with_eos = mutate(label, kind, train, rng, positions)
        ids = ref_tokenizer._tok2ids(pred) + ([ref_tokenizer.eos_id] if with_eos else [])
        for pos in range(positions):
            # past the <eos> the peaks go on: the cut has to ignore them
            peak = ids[pos] if pos < len(ids) else int(rng.integers(classes))
            q[r, pos, peak] = 127
            repeats = (0, 0, 1, 3)[int(rng.integers(4))]                                   # probability 1, 1/2 or 1/4, exactly
            if peak + repeats < classes:
                higher = rng.choice(np.arange(peak + 1, classes), size=repeats, replace=False)
                q[r, pos, higher] = 127
        labels.append(label)
        kinds.append(kind)
    return torch.from_numpy(q.astype(np.int8)), labels, kinds


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--ref', required=True, help='checkout of the reference repository')
    ap.add_argument('--out', default=os.path.join(ROOT, 'tests', 'golden'))
    args = ap.parse_args()
    from safetensors.torch import save_file
    install_stubs()
    sys.modules['nltk'].edit_distance = two_row_edit_distance
    sys.path.insert(0, args.ref)
    from strhub.models import base as ref_base
    ref_base.edit_distance = two_row_edit_distance          # `from nltk import edit_distance` was bound at import

    class StoredLogits(ref_base.CrossEntropySystem):
        """The reference's evaluation step around logits that are already there."""

        def forward(self, images, max_length=None):
            return images                                   # the "images" of a batch ARE its logits

        def training_step(self, batch, batch_idx):
            raise NotImplementedError

    tensors, meta = {}, {'edit_distance': 'nltk is not installed: textbook two-row dynamic programme of tools/make_golden_eval.py (unit costs, no transpositions)',
                         'logits': f'int8 q, logits = q * {SCALE} exactly', 'max_label_length': MAX_LABEL_LENGTH, 'torch': torch.__version__, 'cases': {}}
    for name, (train, test, rows) in CASES.items():
        system = StoredLogits(train, test, 1, 1e-3, 0.0, 0.0)
        q, labels, kinds = make_case(name, train, test, rows, system.tokenizer, system.charset_adapter)
        logits = q.to(torch.float32) * SCALE
        preds, probs = system.tokenizer.decode(logits.softmax(-1))
        adapted = [system.charset_adapter(p) for p in preds]
        assert all(a or g for a, g in zip(adapted, labels)), (name, 'an empty adapted prediction against an empty label: the reference divides by zero')
        assert all(system.charset_adapter(g) == g for g in labels), (name, 'labels must already be in the test charset, as the dataset leaves them')
        with torch.inference_mode():
            res = system._eval_step((logits, labels), False)['output']
        distances = [two_row_edit_distance(a, g) for a, g in zip(adapted, labels)]
        confs = [float(p.prod().item()) for p in probs]
        assert all(c > 0 and np.log2(c) == int(np.log2(c)) for c in confs) and len(set(confs)) > 3, (name, confs)      # exact powers of two
        assert {'equal', 'substitute', 'insert', 'delete', 'empty', 'no_eos'} <= set(kinds) and 0 in distances and max(distances) > 1
        tensors[f'{name}.q'] = q.contiguous()
        meta['cases'][name] = {
            'charset_train': train, 'charset_test': test, 'labels': labels, 'kinds': kinds, 'preds': preds,
            'row_confidence': confs, 'row_distance': distances,
            'result': {'num_samples': res.num_samples, 'correct': res.correct, 'ned': float(res.ned), 'confidence': float(res.confidence),
                       'label_length': res.label_length}}
        print(name, meta['cases'][name]['result'], 'distances', distances)
    save_file(tensors, os.path.join(args.out, 'eval_metrics.safetensors'))
    with open(os.path.join(args.out, 'eval_metrics.json'), 'w') as f:
        json.dump(meta, f, indent=1, ensure_ascii=False)


if __name__ == '__main__':
    main()
