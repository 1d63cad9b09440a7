"""The definition of vocabulary probes (include/hesaff_amd.h, hesaff_set_vocabulary_probes) in numpy, on top of tests/vocabulary_ref.py's
assignment: the P' = min(P, C) first cells in the order (dist2 to the coarse row, cell), then the lexicographic minimum (dist2, row) over
the rows of those cells.  Integers only: nothing here rounds."""
import numpy as np

from tests import vocabulary_cells_ref as R
from tests import vocabulary_ref as V


def coarse_dist2(desc, coarse):
    """-> int64 [n, C]: the squared distances of every key to every coarse row"""
    d = np.asarray(desc, np.uint8).reshape(-1, 128).astype(np.int64)
    g = np.asarray(coarse, np.uint8).reshape(-1, 128).astype(np.int64)
    out = np.zeros((len(d), len(g)), np.int64)
    for i0 in range(0, len(d), 64):
        out[i0:i0 + 64] = ((d[i0:i0 + 64, None, :] - g[None, :, :]) ** 2).sum(axis=2)
    return out


def probe_cells(desc, coarse, P):
    """-> (cells int32 [n, P'], dist2 int32 [n, P']) in probe order: a stable argsort, so equal distances go in ascending cell"""
    dist2 = coarse_dist2(desc, coarse)
    used = min(int(P), dist2.shape[1])
    order = np.argsort(dist2, axis=1, kind="stable")[:, :used]
    return order.astype(np.int32), np.take_along_axis(dist2, order, axis=1).astype(np.int32)


def assign_probes(desc, vocab, coarse, first, P):
    """-> int32 [n, 2] = (word, dist2): V.assign inside every probed cell, then the least (dist2, row) of a key's P' results"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 128)
    vocab = np.asarray(vocab, np.uint8).reshape(-1, 128)
    coarse = np.asarray(coarse, np.uint8).reshape(-1, 128)
    assert R.first_ok(first, len(coarse), len(vocab))
    cells, _ = probe_cells(desc, coarse, P)
    n, used = cells.shape
    row = np.zeros((n, used), np.int64)
    dist2 = np.zeros((n, used), np.int64)
    for p in range(used):
        for c in np.unique(cells[:, p]):
            lo, hi = int(first[c]), int(first[c + 1])
            keys = np.nonzero(cells[:, p] == c)[0]
            a = V.assign(desc[keys], vocab[lo:hi])
            row[keys, p] = a[:, 0] + lo
            dist2[keys, p] = a[:, 1]
    out = np.zeros((n, 2), np.int32)
    if n:
        best = np.lexsort((row, dist2), axis=1)[:, 0]   # (the last key is the primary one: dist2, then the row)
        out[:, 0] = row[np.arange(n), best]
        out[:, 1] = dist2[np.arange(n), best]
    return out


def winning_rank(desc, vocab, coarse, first, P):
    """-> int [n]: the probe rank of the cell that holds each key's word under P probes"""
    cells, _ = probe_cells(desc, coarse, P)
    word = assign_probes(desc, vocab, coarse, first, P)[:, 0]
    cell_of_word = np.searchsorted(np.asarray(first, np.int64), word, side="right") - 1
    return np.argmax(cells == cell_of_word[:, None], axis=1)
