"""
Labelled chunk data of a training run: chunks.npy, references.npy, reference_lengths.npy (and an optional indices.npy) of a directory,
what ``basecaller --save-ctc`` writes (the reference's bonito/data.py: load_numpy_datasets, load_numpy, load_data).

There is no DataLoader: a ``Batches`` object yields plain index slices of the arrays as host tensors. The training order of epoch e is
the permutation ``np.random.default_rng([seed, e])`` draws, so a resumed run sees the batches the uninterrupted run saw.
"""
import os

import numpy as np
import torch

__all__ = ["load_numpy_datasets", "load_numpy", "load_data", "Batches"]


def load_numpy_datasets(limit=None, directory=None):
    """chunks, references, reference_lengths of a directory (reference bonito/data.py:122-144)."""
    chunks = np.load(os.path.join(directory, "chunks.npy"), mmap_mode="r")
    targets = np.load(os.path.join(directory, "references.npy"), mmap_mode="r")
    lengths = np.load(os.path.join(directory, "reference_lengths.npy"), mmap_mode="r")
    indices = os.path.join(directory, "indices.npy")
    if os.path.exists(indices):
        idx = np.load(indices, mmap_mode="r")
        idx = idx[idx < lengths.shape[0]]
        if limit:
            idx = idx[:limit]
        return chunks[idx, :], targets[idx, :], lengths[idx]
    if limit:
        chunks, targets, lengths = chunks[:limit], targets[:limit], lengths[:limit]
    return np.array(chunks), np.array(targets), np.array(lengths)


def load_numpy(limit, directory, valid_chunks=None):
    """-> (train, valid), each (chunks, references, lengths). The validation set is the validation/ sub-directory when there is one
    (its first `valid_chunks`), otherwise the tail of the training set: the last `valid_chunks`, or the last 3 % when none is given."""
    directory = str(directory)
    train = load_numpy_datasets(limit=limit, directory=directory)
    if os.path.exists(os.path.join(directory, "validation")):
        return tuple(train), tuple(load_numpy_datasets(limit=valid_chunks, directory=os.path.join(directory, "validation")))
    print("[validation set not found: splitting training set]")
    n = len(train[0])
    split = int(np.floor(n * 0.97)) if valid_chunks is None else max(0, n - valid_chunks)
    return tuple(x[:split] for x in train), tuple(x[split:] for x in train)


class Batches:
    """Batches of (chunks float32 [B, 1, L], targets int64 [B, Lmax], lengths int64 [B]) host tensors over one data set; the last batch
    may be short. With `shuffle`, the order of an epoch is the permutation of default_rng([seed, epoch]); ``set_epoch`` chooses it."""

    def __init__(self, data, batch_size, shuffle=False, seed=0):
        self.chunks, self.targets, self.lengths = data
        self.batch_size, self.shuffle, self.seed, self.epoch = int(batch_size), bool(shuffle), int(seed), 0
        if self.batch_size < 1:
            raise ValueError("Batches: batch_size must be positive, got %d" % self.batch_size)

    def set_epoch(self, epoch):
        self.epoch = int(epoch)

    def order(self):
        n = len(self.lengths)
        return np.random.default_rng([self.seed, self.epoch]).permutation(n) if self.shuffle else np.arange(n)

    def __len__(self):
        return -(-len(self.lengths) // self.batch_size)

    def __iter__(self):
        order = self.order()
        for lo in range(0, len(order), self.batch_size):
            idx = order[lo:lo + self.batch_size]
            yield (torch.from_numpy(np.asarray(self.chunks[idx], dtype=np.float32)).unsqueeze(1),
                   torch.from_numpy(np.asarray(self.targets[idx]).astype(np.int64)),
                   torch.from_numpy(np.asarray(self.lengths[idx]).astype(np.int64)))


def load_data(directory, chunks, valid_chunks, batch_size, seed):
    """-> (train Batches, valid Batches) of a directory with chunks.npy. A directory that brings its own dataset.py loader is refused:
    running a data set's script is not supported here."""
    directory = str(directory)
    if os.path.exists(os.path.join(directory, "chunks.npy")):
        print("[loading data] - chunks from %s" % directory)
        train, valid = load_numpy(chunks, directory, valid_chunks=valid_chunks)
        return Batches(train, batch_size, shuffle=True, seed=seed), Batches(valid, batch_size)
    if os.path.exists(os.path.join(directory, "dataset.py")):
        raise IOError("Failed to load input data from %s: a dataset.py loader is not supported, only chunks.npy / references.npy / "
                      "reference_lengths.npy" % directory)
    raise IOError("Failed to load input data from %s: no chunks.npy found" % directory)
