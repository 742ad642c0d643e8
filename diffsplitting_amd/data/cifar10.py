"""``data/cifar10.py`` of the reference: the CIFAR-10 "python version" batch files (pickles of
``{b'data': (n, 3072) uint8, b'labels': [n ints], ...}``) -> per-class image stacks for ``SplitDataset('cifar10', ...)``.

Same functions, signatures and return types as the reference (:6-40).  Two departures:

* ``training_files`` returns the directory's entries in SORTED name order.  The reference takes ``os.listdir`` order,
  which is arbitrary; the set of images per class is the same, the order only decides which image of class 0 meets which
  image of class 1 when a directory holds several files.
* a directory entry that is not a CIFAR batch (not a pickle, no ``b'data'`` / ``b'labels'``, a row length other than
  3072, labels and rows of different counts) raises ``DsxError`` naming the file, and so does a class without a single
  image in the directory; the reference fails somewhere inside numpy.

The files are unpickled with ``pickle.load``, which runs whatever a pickle tells it to: a batch file is trusted exactly
like a checkpoint handed to ``torch.load``.  Read only files you would run.
"""
import os
import pickle

import numpy as np

from .._lib import DsxError

ROW = 3 * 32 * 32


def unpickle(file):                                                  # :6-9
    with open(file, "rb") as fo:
        return pickle.load(fo, encoding="bytes")


def training_files(datadir):                                         # :11-13, sorted
    return sorted(os.listdir(datadir))


def testing_files():                                                 # :15-16
    return ["test_batch"]


def load_cifar10_data(fpath):
    """:18-23 -> (imgs (n, 3, 32, 32) uint8, labels)."""
    try:
        data = unpickle(fpath)
    except Exception as e:                                           # unpickling garbage raises nearly anything
        if isinstance(e, OSError) and not isinstance(e, IsADirectoryError):
            raise                                                    # unreadable, not malformed
        raise DsxError(f"{fpath}: not a CIFAR-10 batch file (not a pickle: {type(e).__name__}: {e})") from e
    if not isinstance(data, dict) or b"data" not in data or b"labels" not in data:
        raise DsxError(f"{fpath}: not a CIFAR-10 batch file (a pickled dict with b'data' and b'labels' expected)")
    imgs, labels = np.asarray(data[b"data"]), data[b"labels"]
    if imgs.dtype != np.uint8 or imgs.ndim != 2 or imgs.shape[1] != ROW:
        raise DsxError(f"{fpath}: b'data' must be (n, {ROW}) uint8 rows, got {imgs.dtype} {imgs.shape}")
    if len(labels) != imgs.shape[0]:
        raise DsxError(f"{fpath}: {len(labels)} labels for {imgs.shape[0]} images")
    return imgs.reshape(-1, 3, 32, 32), labels


def load_train_val_data(datadir, label_idx_list):
    """:25-40 -> {i: (n_i, 3, 32, 32) uint8}: the images of label ``label_idx_list[i]`` of every file of ``datadir``,
    file after file in sorted name order."""
    if not isinstance(datadir, (str, os.PathLike)) or not os.path.isdir(datadir):
        raise DsxError(f"cifar10: {datadir!r} is not a directory of CIFAR-10 batch files")
    fnames = training_files(datadir)
    if not fnames:
        raise DsxError(f"cifar10: {datadir} holds no file")
    data = {i: [] for i in range(len(label_idx_list))}
    for f in fnames:
        imgs, labels = load_cifar10_data(os.path.join(datadir, f))
        labels = np.array(labels)
        for i, label in enumerate(label_idx_list):
            data[i].append(imgs[np.where(labels == label)[0]])
    for i, label in enumerate(label_idx_list):
        data[i] = np.concatenate(data[i], axis=0)
        if len(data[i]) == 0:
            raise DsxError(f"cifar10: no image of label {label} in {datadir}")
    return data
