"""The definition of vocabulary cells (include/hesaff_amd.h, hesaff_set_vocabulary_cells) in numpy, on top of tests/vocabulary_ref.py's
assignment: the lowest nearest coarse row, then the lowest nearest row of that cell.  Integers only: nothing here rounds."""
import struct

import numpy as np

from tests import vocabulary_ref as V
from tests import vocabulary_training_ref as T


def first_ok(first, c, k):
    first = [int(v) for v in first]
    return len(first) == c + 1 and 1 <= c <= k and first[0] == 0 and first[c] == k and all(a < b for a, b in zip(first, first[1:]))


def assign_cells(desc, vocab, coarse, first):
    """-> int32 [n, 2] = (word, dist2): V.assign against the coarse rows gives the cell, V.assign against the cell's rows the word"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 128)
    vocab = np.asarray(vocab, np.uint8).reshape(-1, 128)
    coarse = np.asarray(coarse, np.uint8).reshape(-1, 128)
    assert first_ok(first, len(coarse), len(vocab))
    cell = V.assign(desc, coarse)[:, 0]
    out = np.zeros((len(desc), 2), np.int32)
    for c in np.unique(cell):
        lo, hi = int(first[c]), int(first[c + 1])
        keys = np.nonzero(cell == c)[0]
        a = V.assign(desc[keys], vocab[lo:hi])
        out[keys, 0] = a[:, 0] + lo
        out[keys, 1] = a[:, 1]
    return out


def build_cells(words, coarse):
    """-> (words in cell order, order with order[new] = old row, the coarse rows that received a row, first): a stable argsort by the
    nearest coarse row, empty cells dropped"""
    words = np.asarray(words, np.uint8).reshape(-1, 128)
    coarse = np.asarray(coarse, np.uint8).reshape(-1, 128)
    cell = V.assign(words, coarse)[:, 0]
    order = np.argsort(cell, kind="stable").astype(np.int32)
    counts = np.bincount(cell, minlength=len(coarse))
    kept = np.nonzero(counts)[0]
    first = np.concatenate([[0], np.cumsum(counts[kept])]).astype(np.uint32)
    return np.ascontiguousarray(words[order]), order, np.ascontiguousarray(coarse[kept]), first


def train_cells(desc, words, coarse, first, iterations):
    """T.train with the cell-restricted assignment: -> (words uint8 [k, 128], distortion int64 [done], empty int32 [done])"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 128)
    vocab = np.array(words, np.uint8).reshape(-1, 128)
    k = len(vocab)
    distortion, empty = [], []
    for _ in range(iterations):
        a = assign_cells(desc, vocab, coarse, first)
        sums, counts = T.accumulate(desc, a[:, 0], k)
        distortion.append(int(a[:, 1].astype(np.int64).sum()))
        empty.append(int((counts == 0).sum()))
        new = T.update(vocab, sums, counts)
        same = np.array_equal(new, vocab)
        vocab = new
        if same:
            break
    return vocab, np.array(distortion, np.int64), np.array(empty, np.int32)


def train_cell_vocabulary(desc, k, cells, iterations, coarse_iterations):
    """the composite -> (words, coarse, first, distortion, empty)"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 128)
    assert len(desc) >= k >= cells >= 1
    g = T.train(desc, cells, coarse_iterations)[0]
    v0, _, g, first = build_cells(T.sample(desc, k), g)
    words, distortion, empty = train_cells(desc, v0, g, first, iterations)
    return words, g, first, distortion, empty


def cells_file(coarse, first):
    coarse = np.ascontiguousarray(coarse, np.uint8).reshape(-1, 128)
    first = np.asarray(first, "<u4")
    return b"HESAFFC1" + struct.pack("<IIII", 128, len(coarse), int(first[-1]), 0) + coarse.tobytes() + first.tobytes()
