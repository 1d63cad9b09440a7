"""GPU suite of the frame the four word kernels share (kernels_words.h: key load, tile stream, running best and its reduction):
k_assign_words, k_assign_neighbours, k_assign_words_cells and k_probe_cells must agree with the reference and with each other at the
frame's edges - one key, one key in the second column tile, the second wave, the second block; one row, one tile, one row in the
last tile, three tiles.  Keys and rows are drawn from a handful of distinct rows, so equal distances occur across accumulator elements,
across the two lane halves and across tiles, and the lowest row has to win everywhere.  Integers throughout: every comparison is exact."""
import numpy as np
import pytest

import hesaff_amd
from tests import neighbours_ref as N
from tests import vocabulary_probes_ref as P
from tests import vocabulary_ref as V

COUNTS = (1, 33, 65, 257)
SIZES = (1, 32, 33, 65)
POOL = V.family("uniform", 8, seed=901)   # rows draw from the first six, keys from all eight
DESC = POOL[np.random.RandomState(902).randint(0, 8, 257)]


def rows_of(K):
    """K rows of the pool; the first min(K, 4) are distinct, so that each of that many coarse rows keeps a cell"""
    rows = POOL[np.random.RandomState(910 + K).randint(0, 6, K)].copy()
    rows[:min(K, 4)] = POOL[:min(K, 4)]
    return rows


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(want), -1).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d keys differ, first %s: got %s, want %s" % (what, len(bad), len(want), list(bad[:6]), got[bad[:2]].tolist(),
                                                                                 want[bad[:2]].tolist())


@pytest.fixture(scope="module")
def fctx():
    with hesaff_amd.HesaffContext(device=0) as c:
        yield c


@pytest.mark.gpu
@pytest.mark.parametrize("K", SIZES)
def test_the_four_kernels_agree_at_the_edges_of_the_frame(fctx, K):
    c, vocab = fctx, rows_of(K)
    ranks = N.neighbours(DESC, vocab, 8)   # the reference: int64 brute force ordered by (dist2, k)
    flat = ranks[:, 0]
    assert (flat == V.assign(DESC, vocab)).all() and (ranks[:, min(8, K):] == N.NONE).all() and (ranks[:, :min(8, K), 0] >= 0).all()
    assert K == 1 or (ranks[:, 0, 1] == ranks[:, 1, 1]).sum() >= 100, "no ties: the lowest row would not be tested"
    try:
        # k_assign_words, then k_assign_neighbours at R = 8
        c.set_vocabulary(vocab)
        for n in COUNTS:
            _same(c.assign_words(DESC[:n]), flat[:n], "flat, K = %d, n = %d" % (K, n))
        c.set_vocabulary_neighbours(8)
        for n in COUNTS:
            got = c.assign_neighbours(DESC[:n])
            _same(got, ranks[:n], "neighbours, K = %d, n = %d" % (K, n))
            _same(np.ascontiguousarray(got[:, 0]), flat[:n], "rank 0, K = %d, n = %d" % (K, n))
        c.set_vocabulary_neighbours(1)

        # k_assign_words_cells over one cell that is the whole vocabulary, by the project's layer builder
        words, order, coarse, first = c.build_vocabulary_cells(vocab, POOL[6:7])
        assert np.array_equal(words, vocab) and order.tolist() == list(range(K)) and first.tolist() == [0, K]
        c.set_vocabulary_cells(coarse, first)
        for n in COUNTS:
            _same(c.assign_words(DESC[:n]), flat[:n], "one cell, K = %d, n = %d" % (K, n))

        # C = min(K, 4) cells, all of them probed: the flat rows of the vocabulary in cell order, the lowest row on ties
        C = min(K, 4)
        words, order, coarse, first = c.build_vocabulary_cells(vocab, POOL[:C])
        assert len(coarse) == C and np.array_equal(words, vocab[order])
        ordered = V.assign(DESC, words)
        c.set_vocabulary(words)
        for n in COUNTS:
            _same(c.assign_words(DESC[:n]), ordered[:n], "flat in cell order, K = %d, n = %d" % (K, n))
        c.set_vocabulary_cells(coarse, first)
        c.set_vocabulary_probes(C)
        sweep0 = V.assign(DESC, coarse)
        for n in COUNTS:
            _same(c.assign_words(DESC[:n]), ordered[:n], "%d cells, %d probes, K = %d, n = %d" % (C, C, K, n))
            cells, dist2 = c.probe_cells(DESC[:n])
            _same(np.stack([cells[:, 0], dist2[:, 0]], axis=1), sweep0[:n], "sweep 0, C = %d, n = %d" % (C, n))

        # k_probe_cells over the frame's own edges: every row a cell of its own, so the sweeps are the neighbours' ranks
        c.set_vocabulary(vocab)
        c.set_vocabulary_cells(vocab, np.arange(K + 1, dtype=np.uint32))
        c.set_vocabulary_probes(min(8, K))
        for n in COUNTS:
            cells, dist2 = c.probe_cells(DESC[:n])
            _same(np.stack([cells, dist2], axis=2), ranks[:n, :min(8, K)], "probes over K = %d coarse rows, n = %d" % (K, n))
            _same(c.assign_words(DESC[:n]), flat[:n], "one row per cell, K = %d, n = %d" % (K, n))
    finally:
        c.set_vocabulary_probes(1)
        c.set_vocabulary_neighbours(1)
        c.set_vocabulary(None)
