"""Hamming embedding of include/hesaff_amd.h (hesaff_set_embedding, hesaff_train_embedding, hesaff_index_query_embedded) in numpy:
the definition, not an implementation.  Integers are Python's, int64 or uint64; the score is the plain query's three binary64
operations (tests/index_ref.py)."""
import numpy as np

from tests import index_ref

BITS = 64
MASK64 = (1 << 64) - 1


def projection(seed):
    """hesaff_embedding_projection, one entry at a time in Python integers: int8 [64, 128]"""
    s = seed & MASK64
    out = np.zeros(BITS * 128, np.int8)
    for e in range(BITS * 128):
        s = (s + 0x9E3779B97F4A7C15) & MASK64
        x = s
        x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
        x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & MASK64
        x ^= x >> 31
        v = (x >> 56) - 128
        out[e] = -127 if v == -128 else v
    return out.reshape(BITS, 128)


def project(P, desc):
    """z int64 [n, 64]: z[k][i] = sum_j P[i][j] * d_k[j], the descriptor bytes unsigned"""
    return np.asarray(desc, np.uint8).astype(np.int64) @ np.asarray(P, np.int8).astype(np.int64).T


def signatures(P, tau, desc, words):
    """uint64 [n]: bit i of key k is z[k][i] > tau[word_k][i], strictly"""
    z = project(P, desc)
    bits = z > np.asarray(tau, np.int64)[np.asarray(words, np.int64)]
    return (bits.astype(np.uint64) << np.arange(BITS, dtype=np.uint64)).sum(axis=1, dtype=np.uint64)


def thresholds(P, desc, words, k):
    """(tau int32 [k, 64], counts uint32 [k]): per word and bit the lower median - element (m - 1) // 2 of the word's values sorted
    ascending - and 0 for a word without keys"""
    z = project(P, desc)
    words = np.asarray(words, np.int64)
    tau = np.zeros((k, BITS), np.int32)
    counts = np.bincount(words, minlength=k).astype(np.uint32)
    for w in np.nonzero(counts)[0]:
        zs = np.sort(z[words == w], axis=0)
        tau[w] = zs[(len(zs) - 1) // 2]
    return tau, counts


def popcount(x):
    x = np.asarray(x, np.uint64)
    return np.array([bin(int(v)).count("1") for v in x.reshape(-1)], np.int64).reshape(x.shape)


def query(index, images, image_sigs, words, sigs, hamming, top):
    """index: index_ref.build(images, k); images / image_sigs: per image its words and its signatures; the query's words and
    signatures -> (images int32 [min(top, N)], scores float64, dot uint64 [N], score float64 [N], nq2 int)"""
    tf, df, idf, norm2 = index
    words = np.asarray(words, np.int64)
    sigs = np.asarray(sigs, np.uint64)
    f = idf.astype(np.uint64)
    qw, qc = np.unique(words, return_counts=True)
    nq2 = int(((qc.astype(np.uint64) * f[qw]) ** 2).sum(dtype=np.uint64))
    dot = np.zeros(len(images), np.uint64)
    for i, (iw, ig) in enumerate(zip(images, image_sigs)):
        iw = np.asarray(iw, np.int64)
        ig = np.asarray(ig, np.uint64)
        total = 0
        for w, g in zip(words, sigs):
            same = iw == w
            if same.any():
                total += int((popcount(ig[same] ^ g) <= hamming).sum()) * int(f[w]) ** 2
        dot[i] = total
    with np.errstate(divide="ignore", invalid="ignore"):
        score = np.where(dot > 0, dot.astype(np.float64) / np.sqrt(np.float64(nq2) * norm2.astype(np.float64)), 0.0)
    order = np.lexsort((np.arange(len(images)), -score))[:top]
    return order.astype(np.int32), score[order], dot, score, nq2


def build(images, k):
    return index_ref.build(images, k)
