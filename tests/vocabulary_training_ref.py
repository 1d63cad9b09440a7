"""The definition of vocabulary training (include/hesaff_amd.h, hesaff_train_vocabulary) in numpy: Lloyd iterations over
tests/vocabulary_ref.py's assignment with the mean rounded half up, empty words keeping their rows.  Integers only."""
import numpy as np

from tests import vocabulary_ref as V


def sample(desc, k):
    """the initial vocabulary of a call without one: row r = desc[r * n // k]"""
    n = len(desc)
    assert n >= k
    return np.ascontiguousarray(desc[[r * n // k for r in range(k)]])


def accumulate(desc, words, k):
    """-> (sums uint32 [k, 128], counts uint32 [k])"""
    sums = np.zeros((k, 128), np.int64)
    np.add.at(sums, words, np.asarray(desc, np.uint8).astype(np.int64))
    return sums.astype(np.uint32), np.bincount(words, minlength=k).astype(np.uint32)


def update(vocab, sums, counts):
    """(2 sum + count) // (2 count) where count > 0, the old row elsewhere"""
    s, c = sums.astype(np.int64), counts.astype(np.int64)[:, None]
    mean = (2 * s + c) // np.maximum(2 * c, 1)
    return np.where(c > 0, mean, vocab.astype(np.int64)).astype(np.uint8)


def train(desc, k, iterations, init=None):
    """-> (words uint8 [k, 128], distortion int64 [done], empty int32 [done])"""
    desc = np.asarray(desc, np.uint8).reshape(-1, 128)
    vocab = sample(desc, k) if init is None else np.array(init, np.uint8).reshape(k, 128)
    distortion, empty = [], []
    for _ in range(iterations):
        a = V.assign(desc, vocab)
        sums, counts = accumulate(desc, a[:, 0], k)
        distortion.append(int(a[:, 1].astype(np.int64).sum()))
        empty.append(int((counts == 0).sum()))
        new = update(vocab, sums, counts)
        same = np.array_equal(new, vocab)
        vocab = new
        if same:
            break
    return vocab, np.array(distortion, np.int64), np.array(empty, np.int32)


def clustered(n=4099, centres=33, noise=12, seed=5):
    """n keys around `centres` rows with bytes in 20 .. 235, uniform noise of +-noise: K = 33 from the sampled rows runs 8 iterations
    to a fixed point with 2 words empty"""
    rng = np.random.RandomState(seed)
    c = rng.randint(20, 236, (centres, 128))
    which = rng.randint(0, centres, n)
    return (c[which] + rng.randint(-noise, noise + 1, (n, 128))).astype(np.uint8)
