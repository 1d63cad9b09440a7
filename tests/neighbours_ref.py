"""The definition of vocabulary neighbours (include/hesaff_amd.h, hesaff_set_vocabulary_neighbours) in numpy: the R lexicographically
least pairs (dist2(k), k) per key, ascending.  Integers only; the stable sort gives the lower row on ties."""
import numpy as np

NONE = (-1, 2 ** 31 - 1)   # a rank the vocabulary is too small for


def neighbours(desc, vocab, R, block=32):
    """desc uint8 [n, 128], vocab uint8 [K, 128] -> int32 [n, R, 2] = (word, dist2) per rank; ranks r >= K are NONE"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 128)
    w = np.asarray(vocab, np.uint8).reshape(-1, 128).astype(np.int64)
    out = np.empty((len(desc), R, 2), np.int32)
    out[:] = NONE
    m = min(R, len(w))
    for i0 in range(0, len(desc), block):
        d2 = ((desc[i0:i0 + block].astype(np.int64)[:, None, :] - w[None, :, :]) ** 2).sum(axis=2)
        order = np.argsort(d2, axis=1, kind="stable")[:, :R]
        out[i0:i0 + block, :m, 0] = order
        out[i0:i0 + block, :m, 1] = np.take_along_axis(d2, order, axis=1)
    return out


def neighbours_loops(desc, vocab, R):
    """the same by a plain double loop and Python's sort of (dist2, k) tuples"""
    out = []
    for d in desc:
        pairs = sorted((sum((int(a) - int(b)) ** 2 for a, b in zip(d, w)), k) for k, w in enumerate(vocab))
        out.append([[k, d2] for d2, k in pairs[:R]] + [list(NONE)] * max(0, R - len(pairs)))
    return np.array(out, np.int32).reshape(len(desc), R, 2)
