"""Training and validation data: labelled folders and the loader that turns them into uint8 batches on the device.

A dataset is a directory with a `gt.txt`: one sample per line, the image path (relative to the directory) and the label separated by
the first run of whitespace — the input format of the reference's `tools/create_lmdb_dataset.py:40-45`, the form `test.py` reads too.
The reference trains from LMDB archives made from such files (`strhub/data/dataset.py`); LMDB is out of scope here.

Labels go through the reference dataset's filter (`strhub/data/dataset.py:95-127`, `preprocess_label`): whitespace removed, NFKD-normalised
to ASCII, dropped if longer than `max_label_length`, mapped into the charset (`charset_train` for training and validation sets —
`strhub/data/module.py:84-109` — `charset_test` for `test.py`), dropped if nothing is left.

`Loader` is `SceneTextDataModule.train_dataloader` / `val_dataloader` (`strhub/data/module.py:111-131`) plus the training transform
(`:69-82`): a shuffle per epoch drawn from (seed, epoch), no `drop_last`, PIL decode in a thread pool of `workers` threads, ONE upload of
the batch's ragged crops, then `RandAugment.sample` + `augment_resize_batch` (augment=True) or `resize_batch` on the device.  A batch is
uint8 [N, 3, H, W] plus its labels — what `TrainStep` and `Evaluator` take as they are.  The host half (decode, the policy's draws) of
the next batch runs in a background thread while the caller works on the current one, and the device half runs on a side stream of the
loader's own, so asking for the next batch right after enqueueing a training step waits for neither.
"""
from __future__ import annotations

import copy
import os
import queue
import threading
import unicodedata
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Iterator, List, Optional, Sequence, Tuple

import numpy as np

from .tokenizer import CharsetAdapter


def parse_gt_line(line: str) -> Optional[Tuple[str, str]]:
    """'path label' -> (path, label); the label may contain blanks.  None for a line without both parts."""
    parts = line.strip().split(maxsplit=1)
    return (parts[0], parts[1]) if len(parts) == 2 else None


def preprocess_label(label: str, adapter: CharsetAdapter, max_label_length: int) -> Optional[str]:
    """The label as the reference's dataset hands it to the model, or None if the dataset drops the sample."""
    label = ''.join(label.split())
    label = unicodedata.normalize('NFKD', label).encode('ascii', 'ignore').decode()
    if len(label) > max_label_length:            # before the adapter: the raw label may be too long for the model
        return None
    return adapter(label) or None


def read_gt(folder: str, charset: str, max_label_length: int) -> List[Tuple[str, str]]:
    """[(image file, label)] of the samples of `folder/gt.txt` that survive the label filter."""
    adapter = CharsetAdapter(charset)
    samples = []
    with open(os.path.join(folder, 'gt.txt'), encoding='utf-8') as fh:
        for line in fh:
            parsed = parse_gt_line(line)
            if parsed is None:
                continue
            label = preprocess_label(parsed[1], adapter, max_label_length)
            if label is not None:
                samples.append((os.path.join(folder, parsed[0]), label))
    return samples


class LabelledFolder:
    """The samples of one labelled folder: `labels[i]` and `load(i)` -> uint8 [H, W, 3] (decoded by PIL, converted to RGB as
    strhub/data/dataset.py:137-139 does)."""

    def __init__(self, folder: str, charset: str, max_label_length: int):
        self.folder = folder
        self.samples = read_gt(folder, charset, max_label_length)
        self.labels = [label for _, label in self.samples]

    def __len__(self) -> int:
        return len(self.samples)

    def load(self, i: int) -> np.ndarray:
        from PIL import Image
        with Image.open(self.samples[i][0]) as im:
            return np.asarray(im.convert('RGB'))


class InMemoryDataset:
    """Already decoded crops (uint8 [H_i, W_i, 3] arrays) and their labels, unfiltered: what a benchmark or a test renders itself."""

    def __init__(self, crops: Sequence[np.ndarray], labels: Sequence[str]):
        if len(crops) != len(labels):
            raise ValueError(f'{len(crops)} crops for {len(labels)} labels')
        self.crops, self.labels = list(crops), list(labels)

    def __len__(self) -> int:
        return len(self.crops)

    def load(self, i: int) -> np.ndarray:
        return self.crops[i]


def epoch_order(n: int, seed: int, epoch: int, shuffle: bool = True) -> np.ndarray:
    """The order in which epoch `epoch` visits n samples: a permutation drawn from numpy's generator seeded with (seed, epoch) — the same
    for the same pair wherever a run is resumed, different from epoch to epoch."""
    if not shuffle:
        return np.arange(n)
    return np.random.default_rng([int(seed), int(epoch)]).permutation(n)


def batch_slices(n: int, batch_size: int) -> List[Tuple[int, int]]:
    """[(begin, end)] of the batches of n samples: the last one may be short (no drop_last, strhub/data/module.py:117-121)."""
    if batch_size < 1:
        raise ValueError(f'batch_size={batch_size}')
    return [(at, min(at + batch_size, n)) for at in range(0, n, batch_size)]


@dataclass
class Batch:
    images: object                   # uint8 [N, 3, H, W] on the device
    labels: List[str]
    index: int                       # the batch's number within its epoch
    indices: np.ndarray              # the samples it holds
    policy_state: Optional[dict]     # the augmentation policy's generator state AFTER this batch's draws (None without augmentation)


@dataclass
class _HostBatch:
    crops: List[np.ndarray]
    chains: Optional[list]
    labels: List[str]
    index: int
    indices: np.ndarray
    policy_state: Optional[dict]


class Loader:
    """Batches of a dataset (`LabelledFolder`, `InMemoryDataset`) as uint8 [N, 3, H, W] on `device` (see the module docstring).

        loader = Loader(dataset, 384, (32, 128), 'cuda', augment=True, seed=0)
        for batch in loader.epoch(3):          # the shuffle of epoch 3; start=k skips the first k batches (the policy draws nothing for them)
            step(batch.images, batch.labels)

    `workers` sizes the decode pool (an argument, never the machine's core count).  `policy`: a `parseq_amd.augment.RandAugment`; the
    default is the reference's (magnitude 5, three layers) seeded with `seed`."""

    def __init__(self, dataset, batch_size: int, img_size=(32, 128), device='cuda', shuffle: bool = True, augment: bool = False, seed: int = 0,
                 workers: int = 8, policy=None):
        if workers < 1:
            raise ValueError(f'workers={workers}')
        self.dataset, self.batch_size, self.img_size, self.device = dataset, int(batch_size), tuple(img_size), device
        self.shuffle, self.augment, self.seed, self.workers = shuffle, augment, int(seed), int(workers)
        if augment and policy is None:
            from .augment import RandAugment
            policy = RandAugment(seed=seed)
        self.policy = policy if augment else None
        self._side = None
        if len(dataset) == 0:
            raise ValueError('an empty dataset')

    def __len__(self) -> int:
        """Batches per epoch."""
        return (len(self.dataset) + self.batch_size - 1) // self.batch_size

    def order(self, epoch: int) -> np.ndarray:
        return epoch_order(len(self.dataset), self.seed, epoch, self.shuffle)

    # ---- host half (background thread) --------------------------------------------------------------------------------------------
    def _host_batches(self, epoch: int, start: int, pool: ThreadPoolExecutor) -> Iterator[_HostBatch]:
        order = self.order(epoch)
        for k, (b, e) in enumerate(batch_slices(len(order), self.batch_size)):
            if k < start:
                continue
            idx = order[b:e]
            crops = list(pool.map(self.dataset.load, idx.tolist()))
            chains = state = None
            if self.policy is not None:
                chains = self.policy.sample([c.shape[:2] for c in crops])
                state = copy.deepcopy(self.policy.rng.bit_generator.state)
            yield _HostBatch(crops, chains, [self.dataset.labels[i] for i in idx.tolist()], k, idx, state)

    # ---- device half (caller's thread, the loader's side stream) --------------------------------------------------------------------
    def to_device(self, crops: Sequence[np.ndarray], chains=None):
        """Ragged uint8 [H_i, W_i, 3] host crops -> uint8 [N, 3, H, W] on the device: the crops packed into one buffer and uploaded at once
        (each on a 16-byte boundary), then augmented (`chains`) and resized, or resized only."""
        import torch
        from .augment import augment_resize_batch
        from .preprocess import resize_batch
        offsets, total = [], 0
        for c in crops:
            if c.dtype != np.uint8 or c.ndim != 3 or c.shape[2] != 3:
                raise ValueError(f'a crop of {c.dtype} {c.shape}: expected uint8 [H, W, 3]')
            offsets.append(total)
            total += (c.size + 15) // 16 * 16
        packed = np.empty(total, dtype=np.uint8)
        for c, at in zip(crops, offsets):
            packed[at:at + c.size] = c.reshape(-1)
        dev = torch.device(self.device)
        main = torch.cuda.current_stream(dev)
        if self._side is None:
            self._side = torch.cuda.Stream(device=dev)
        with torch.cuda.stream(self._side):
            flat = torch.from_numpy(packed).to(dev)
            views = [flat[at:at + c.size].view(c.shape) for c, at in zip(crops, offsets)]
            out = augment_resize_batch(views, chains, self.img_size) if chains is not None else resize_batch(views, self.img_size)
            # (both end with a synchronisation of the current stream — the side stream: the batch is complete here)
        main.wait_stream(self._side)
        out.record_stream(main)
        return out

    def epoch(self, epoch: int, start: int = 0) -> Iterator[Batch]:
        """The batches of one epoch, from batch `start` on.  The host half of batch k + 1 is made while the caller holds batch k."""
        q: queue.Queue = queue.Queue(maxsize=1)
        stop = threading.Event()

        def produce():
            try:
                with ThreadPoolExecutor(max_workers=self.workers) as pool:
                    for hb in self._host_batches(epoch, start, pool):
                        while not stop.is_set():
                            try:
                                q.put(hb, timeout=0.1)
                                break
                            except queue.Full:
                                continue
                        if stop.is_set():
                            return
                item = None
            except BaseException as exc:      # handed to the consumer
                item = exc
            while not stop.is_set():
                try:
                    q.put(item, timeout=0.1)
                    return
                except queue.Full:
                    continue

        thread = threading.Thread(target=produce, name='parseq-loader', daemon=True)
        thread.start()
        try:
            while True:
                hb = q.get()
                if hb is None:
                    return
                if isinstance(hb, BaseException):
                    raise hb
                yield Batch(self.to_device(hb.crops, hb.chains), hb.labels, hb.index, hb.indices, hb.policy_state)
        finally:
            stop.set()
            thread.join()
