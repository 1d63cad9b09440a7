"""The definition of visual-word assignment (include/hesaff_amd.h, hesaff_set_vocabulary) in numpy, the data families the tests run
it on, and builders for the two file formats.  Integers only: nothing here rounds."""
import struct

import numpy as np

WORDS_ROW = np.dtype([("x", "<f4"), ("y", "<f4"), ("a", "<f4"), ("b", "<f4"), ("c", "<f4"), ("word", "<u4")])


def assign(desc, vocab, block=64):
    """desc uint8 [n, 128], vocab uint8 [K, 128] -> int32 [n, 2] = (word, dist2): int64 differences, argmin (the first minimum)."""
    desc = np.asarray(desc, np.uint8).reshape(-1, 128)
    vocab = np.asarray(vocab, np.uint8).reshape(-1, 128)
    out = np.zeros((len(desc), 2), np.int32)
    w = vocab.astype(np.int64)
    for i0 in range(0, len(desc), block):
        d = desc[i0:i0 + block].astype(np.int64)
        dist2 = ((d[:, None, :] - w[None, :, :]) ** 2).sum(axis=2)
        word = np.argmin(dist2, axis=1)
        out[i0:i0 + block, 0] = word
        out[i0:i0 + block, 1] = dist2[np.arange(len(d)), word]
    return out


def assign_xor(desc, vocab):
    """the identity the device uses: d' = d ^ 0x80, w' = w ^ 0x80 as signed bytes, dist2 = |d'|^2 + |w'|^2 - 2 d'.w', all in int32;
    the first minimum of |w'_k|^2 - 2 d'.w'_k over k is the word"""
    d = (np.asarray(desc, np.uint8).reshape(-1, 128) ^ 0x80).view(np.int8).astype(np.int32)
    w = (np.asarray(vocab, np.uint8).reshape(-1, 128) ^ 0x80).view(np.int8).astype(np.int32)
    dot = d @ w.T
    assert np.abs(dot).max(initial=0) <= 1 << 21
    score = (w * w).sum(axis=1, dtype=np.int32)[None, :] - 2 * dot
    word = np.argmin(score, axis=1)
    out = np.zeros((len(d), 2), np.int32)
    out[:, 0] = word
    out[:, 1] = score[np.arange(len(d)), word] + (d * d).sum(axis=1, dtype=np.int32)
    return out


FAMILIES = ("uniform", "extremes", "high", "low")


def family(name, rows, seed):
    """seeded uint8 [rows, 128]: uniform bytes, bytes in {0, 255}, in {254, 255}, in {0, 1}"""
    rng = np.random.RandomState(seed)
    if name == "uniform":
        return rng.randint(0, 256, (rows, 128)).astype(np.uint8)
    bits = rng.randint(0, 2, (rows, 128)).astype(np.uint8)
    if name == "extremes":
        return (bits * 255).astype(np.uint8)
    if name == "high":
        return (254 + bits).astype(np.uint8)
    if name == "low":
        return bits
    raise ValueError(name)


def vocabulary_file(vocab):
    vocab = np.ascontiguousarray(vocab, np.uint8).reshape(-1, 128)
    return b"HESAFFV1" + struct.pack("<II", 128, len(vocab)) + vocab.tobytes()


def words_file(xyabc, words, vocabulary_size):
    """xyabc: float32 [n, 5] (the five floats of the .hesaff.bin rows), words: the int32 [n, 2] rows or their first column"""
    xyabc = np.asarray(xyabc, np.float32).reshape(-1, 5)
    words = np.asarray(words)
    word = words[:, 0] if words.ndim == 2 else words
    rows = np.zeros(len(xyabc), WORDS_ROW)
    for j, f in enumerate(("x", "y", "a", "b", "c")):
        rows[f] = xyabc[:, j]
    rows["word"] = word.astype(np.uint32)
    return b"HESAFFW1" + struct.pack("<II", vocabulary_size, len(rows)) + rows.tobytes()
