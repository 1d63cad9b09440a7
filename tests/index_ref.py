"""The image index of include/hesaff_amd.h (hesaff_index_build / hesaff_index_query) in numpy: the definition, not an implementation.
Integers are Python's or uint64; the score is three binary64 operations."""
import numpy as np


def ilog2_q8(n, df):
    q = (n << 31) // df
    e = q.bit_length() - 1 - 31
    m, r = q >> e, e
    for _ in range(8):
        m, r = (m * m) >> 31, 2 * r
        if m >= 1 << 32:
            r, m = r + 1, m >> 1
    return r


def build(images, k):
    """images: a list of int arrays of words in 0 .. k - 1 -> (tf: per image (words, counts), df uint32 [k], idf uint32 [k], norm2 uint64 [N])"""
    n = len(images)
    tf = [np.unique(np.asarray(w, np.int64), return_counts=True) for w in images]
    df = np.zeros(k, np.uint32)
    for w, _ in tf:
        df[w] += 1
    idf = np.zeros(k, np.uint32)
    used = np.nonzero(df)[0]
    idf[used] = [ilog2_q8(n, int(d)) for d in df[used]]
    norm2 = np.array([((c.astype(np.uint64) * idf[w].astype(np.uint64)) ** 2).sum(dtype=np.uint64) for w, c in tf], np.uint64)
    return tf, df, idf, norm2


def query(index, words, top):
    """-> (images int32 [min(top, N)], scores float64, dot uint64 [N], score float64 [N], nq2 int)"""
    tf, df, idf, norm2 = index
    qw, qc = np.unique(np.asarray(words, np.int64), return_counts=True)
    tfq = np.zeros(len(df), np.uint64)
    tfq[qw] = qc.astype(np.uint64)
    f = idf.astype(np.uint64)
    nq2 = ((tfq * f) ** 2).sum(dtype=np.uint64)
    dot = np.array([(tfq[w] * c.astype(np.uint64) * f[w] * f[w]).sum(dtype=np.uint64) for w, c in tf], np.uint64)
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.where(dot > 0, dot.astype(np.float64) / np.sqrt(np.float64(nq2) * norm2.astype(np.float64)), 0.0)
    order = np.lexsort((np.arange(len(tf)), -score))[:top]
    return order.astype(np.int32), score[order], dot, score, int(nq2)
