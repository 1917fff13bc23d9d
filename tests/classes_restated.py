"""numpy restatement of csrc/mc_classes.h (the length-class rule) and of what the device prologue of a class run (csrc/k_classes.h)
must leave: perm, the class starts and the trimmed reads of every class back to back in 16-byte aligned blocks."""
import numpy as np


def class_of(lengths, class_len):
    """index of the largest class_len[k] <= len, K where there is none"""
    cl = np.asarray(class_len, np.int64)
    k = np.searchsorted(cl, np.asarray(lengths, np.int64), side="right") - 1
    return np.where(k < 0, len(cl), k).astype(np.int64)


def row_len(rows):
    """index of the first 0 byte of every row, or the stride"""
    rows = np.asarray(rows, np.uint8)
    zero = rows == 0
    return np.where(zero.any(axis=1), zero.argmax(axis=1), rows.shape[1]).astype(np.int64)


def make_rows(seqs, stride):
    """reads (bytes) -> padded rows: the first min(len, stride) bases, then 0 bytes"""
    rows = np.zeros((len(seqs), stride), np.uint8)
    for i, s in enumerate(seqs):
        s = s[:stride]
        rows[i, :len(s)] = np.frombuffer(s, np.uint8)
    return rows


def prologue(rows, class_len):
    """-> perm (stable by class, rows without a class last), start[K + 2], word0[K + 1], sorted bytes (16 * word0[K])"""
    K = len(class_len)
    cls = class_of(row_len(rows), class_len)
    perm = np.argsort(cls, kind="stable").astype(np.uint32)
    counts = np.bincount(cls, minlength=K + 1)
    start = np.zeros(K + 2, np.int64)
    start[1:] = np.cumsum(counts)
    word0 = np.zeros(K + 1, np.int64)
    for k in range(K):
        word0[k + 1] = word0[k] + (counts[k] * class_len[k] + 15) // 16
    out = np.zeros(int(word0[K]) * 16, np.uint8)
    for k in range(K):
        idx = perm[start[k]:start[k + 1]]
        blk = rows[idx, :class_len[k]].reshape(-1)
        out[word0[k] * 16: word0[k] * 16 + len(blk)] = blk
    return perm, start.astype(np.uint32), word0, out
