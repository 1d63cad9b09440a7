"""GPU suite of Hamming embedding (hesaff_set_embedding, hesaff_train_embedding, hesaff_index_build_embedded,
hesaff_index_query_embedded, include/hesaff_amd.h; kernels_embed.h).  The reference is tests/embedding_ref.py: the definition in
numpy.  Every comparison is bit for bit - z, signatures, thresholds, counts, df, idf, norm2, dot, nq2, the float64 scores as uint64
bit patterns, the ranked images and the files."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from tests import embedding_ref as E
from tests import index_ref as R
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
E2E_IMAGES = ["band_160x120", "band_96x96", "band_160x120", "tiny_20x15", "band_96x96"]
E2E_KEYS = [221, 74, 221, 0, 74]
ARG = -2
I32 = np.iinfo(np.int32)
ALL = np.uint64((1 << 64) - 1)
Z_MAX = 128 * 127 * 255


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def ectx():
    with hesaff_amd.HesaffContext(_params(max_batch=5), device=0) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _one_hot():
    """P with z[i] = d[i]"""
    P = np.zeros((64, 128), np.int8)
    P[np.arange(64), np.arange(64)] = 1
    return P


def _with_embedding(ctx, K, P, tau):
    ctx.set_vocabulary(V.family("uniform", K, seed=K))
    ctx.set_embedding(P, tau)


# ---------------------------------------------------------------- projection and signatures

@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_project_equals_the_matrix_product(ectx, n):
    rng = np.random.RandomState(n)
    for P in (hesaff_amd.embedding_projection(n), rng.randint(-127, 128, (64, 128)).astype(np.int8), _one_hot()):
        for desc in (rng.randint(0, 256, (n, 128)).astype(np.uint8), V.family("extremes", n, seed=n)):
            z = ectx.project(desc, P)
            assert z.dtype == np.int32 and np.array_equal(z, E.project(P, desc))


@pytest.mark.gpu
def test_project_reaches_both_ends_of_the_range(ectx):
    d = np.full((65, 128), 255, np.uint8)
    d[64] = 0
    for v in (127, -127):
        z = ectx.project(d, np.full((64, 128), v, np.int8))
        assert (z[:64] == (Z_MAX if v > 0 else -Z_MAX)).all() and (z[64] == 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 33, 300])
def test_signatures_key_counts_and_sources(ectx, K):
    """n on both sides of a wavefront's 64 keys and over more than one block; host arrays with bare words and (word, dist2) rows,
    and device memory as a key array (stride 164, offset 36) and as a packed tensor; the sources are only read"""
    import torch
    rng = np.random.RandomState(K)
    P = hesaff_amd.embedding_projection(K)
    tau = rng.randint(-150000, 150000, (K, 64)).astype(np.int32)   # (z of a random key spreads over about +- 120 000)
    _with_embedding(ectx, K, P, tau)
    try:
        got_P, got_tau = ectx.embedding()
        assert np.array_equal(got_P, P) and np.array_equal(got_tau, tau)
        for n in (1, 63, 64, 65, 257):
            desc = rng.randint(0, 256, (n, 128)).astype(np.uint8)
            words = rng.randint(0, K, n).astype(np.int32)
            words[-1] = K - 1
            want = E.signatures(P, tau, desc, words)
            assert np.array_equal(ectx.embed(desc, words), want), (K, n, "bare words")
            rows = np.stack([words, np.full(n, -9, np.int32)], axis=1)
            assert np.array_equal(ectx.embed(desc, rows), want), (K, n, "(word, dist2) rows")
            recs = np.zeros((n, 164), np.uint8)
            recs[:, 36:] = desc
            for src, stride, offset in ((recs, 164, 36), (desc, 128, 0)):
                for wsrc, wstride in ((words, 1), (rows, 2)):
                    t = torch.from_numpy(src.copy()).cuda()
                    w = torch.from_numpy(wsrc.copy()).cuda()
                    out = torch.full((n + 1,), -1, dtype=torch.int64).cuda()
                    torch.cuda.synchronize()
                    ectx.embed_device(t.data_ptr(), n, stride, offset, w.data_ptr(), wstride, out.data_ptr())
                    got = out.cpu().numpy().view(np.uint64)
                    assert np.array_equal(got[:n], want) and got[n] == ALL, (K, n, stride, wstride)
                    assert np.array_equal(t.cpu().numpy(), src) and np.array_equal(w.cpu().numpy(), wsrc)
        assert len(ectx.embed(np.zeros((0, 128), np.uint8), np.zeros(0, np.int32))) == 0
    finally:
        ectx.set_vocabulary(None)


@pytest.mark.gpu
def test_signature_bits_are_strict_compares_in_their_places(ectx):
    """one-hot rows, z[i] = d[i]: thresholds at d - 1, d and d + 1 for bits 0, 31, 32 and 63 (the two tiles of P, the two lanes of a
    key, the first and last register) - only d - 1 sets the bit, and it sets that bit alone"""
    P = _one_hot()
    rng = np.random.RandomState(4)
    n = 70
    desc = rng.randint(1, 255, (n, 128)).astype(np.uint8)
    K = 3 * n
    tau = np.full((K, 64), I32.max, np.int32)
    words = np.zeros(n, np.int32)
    for bit in (0, 31, 32, 63):
        for delta in (-1, 0, 1):
            tau[:] = I32.max
            for k in range(n):
                words[k] = 3 * k + delta + 1
                tau[words[k], bit] = int(desc[k, bit]) + delta
            _with_embedding(ectx, K, P, tau)
            got = ectx.embed(desc, words)
            want = np.full(n, (1 << bit) if delta < 0 else 0, np.uint64)
            assert np.array_equal(got, want) and np.array_equal(got, E.signatures(P, tau, desc, words)), (bit, delta)
    # every bit in turn: bit i alone is set when only row i's threshold lies below
    tau = np.full((64, 64), I32.max, np.int32)
    tau[np.arange(64), np.arange(64)] = 0
    _with_embedding(ectx, 64, P, tau)
    got = ectx.embed(desc[:64], np.arange(64, dtype=np.int32))
    assert got.tolist() == [1 << i for i in range(64)]
    ectx.set_vocabulary(None)


@pytest.mark.gpu
def test_signatures_at_the_ends_of_the_range_and_of_int32(ectx):
    """P all 127 with d all 255 and P all -127: z = +- 4 145 280, against thresholds one below, equal and one above; thresholds
    INT32_MIN (every bit) and INT32_MAX (none); negative thresholds against negative z"""
    d = np.full((65, 128), 255, np.uint8)
    for v, z in ((127, Z_MAX), (-127, -Z_MAX)):
        P = np.full((64, 128), v, np.int8)
        tau = np.array([[z - 1] * 64, [z] * 64, [z + 1] * 64, [I32.min] * 64, [I32.max] * 64, [I32.min, I32.max] * 32], np.int32)
        _with_embedding(ectx, 6, P, tau)
        words = (np.arange(65) % 6).astype(np.int32)
        got = ectx.embed(d, words)
        want = np.array([ALL, 0, 0, ALL, 0, 0x5555555555555555], np.uint64)[words]
        assert np.array_equal(got, want) and np.array_equal(got, E.signatures(P, tau, d, words)), v
    rng = np.random.RandomState(8)
    P = -np.abs(hesaff_amd.embedding_projection(8))
    desc = rng.randint(0, 256, (130, 128)).astype(np.uint8)
    z = E.project(P, desc)
    assert (z <= 0).all()
    tau = np.sort(z, axis=0)[[10, 64, 120]].astype(np.int32)   # negative thresholds taken from the data: equal values occur
    _with_embedding(ectx, 3, P, tau)
    words = rng.randint(0, 3, 130).astype(np.int32)
    got = ectx.embed(desc, words)
    assert np.array_equal(got, E.signatures(P, tau, desc, words)) and len(np.unique(got)) > 60
    ectx.set_vocabulary(None)


# ---------------------------------------------------------------- thresholds

def _check_training(ctx, desc, words, K, P, what, device=False):
    want_tau, want_counts = E.thresholds(P, desc, words, K)
    if device:
        import torch
        recs = np.zeros((len(desc), 164), np.uint8)
        recs[:, 36:] = desc
        rows = np.stack([words, np.full(len(words), -3, np.int32)], axis=1)
        t = torch.from_numpy(recs).cuda()
        w = torch.from_numpy(rows).cuda()
        torch.cuda.synchronize()
        tau, counts = ctx.train_embedding_device(t.data_ptr(), len(desc), 164, 36, w.data_ptr(), 2, K, P)
        assert np.array_equal(t.cpu().numpy(), recs) and np.array_equal(w.cpu().numpy(), rows)
    else:
        tau, counts = ctx.train_embedding(desc, words, P, K)
    assert tau.dtype == np.int32 and counts.dtype == np.uint32 and tau.shape == (K, 64)
    assert np.array_equal(counts, want_counts), (what, "counts")
    assert np.array_equal(tau, want_tau), (what, "tau", np.argwhere(tau != want_tau)[:4].tolist())
    return tau, counts


@pytest.mark.gpu
def test_thresholds_word_sizes(ectx):
    """words with 0, 1, 2, 3, 64, 65 and 1025 keys, shuffled; host and device sources; two calls give the same bytes"""
    sizes = [0, 1, 2, 3, 64, 65, 1025, 0]
    rng = np.random.RandomState(12)
    words = np.concatenate([np.full(m, w, np.int32) for w, m in enumerate(sizes)])
    rng.shuffle(words)
    desc = rng.randint(0, 256, (len(words), 128)).astype(np.uint8)
    P = hesaff_amd.embedding_projection(12)
    tau, counts = _check_training(ectx, desc, words, len(sizes), P, "sizes")
    assert counts.tolist() == sizes and (tau[0] == 0).all() and (tau[7] == 0).all()
    tau2, counts2 = _check_training(ectx, desc, words, len(sizes), P, "sizes, device", device=True)
    assert tau2.tobytes() == tau.tobytes() and counts2.tobytes() == counts.tobytes()
    back = rng.permutation(len(words))   # the order of arrival does not show
    tau3, _ = _check_training(ectx, desc[back], words[back], len(sizes), P, "sizes, permuted")
    assert tau3.tobytes() == tau.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 33, 300, 4099])
def test_thresholds_vocabulary_sizes(ectx, K):
    """random words at every K at which the grouping changes its sub-counters (64 below K = 65, 16 at 300, 1 from 4097 on); at K = 33
    one word holds all the keys in a second run"""
    rng = np.random.RandomState(K)
    n = 3000
    desc = rng.randint(0, 256, (n, 128)).astype(np.uint8)
    P = hesaff_amd.embedding_projection(K + 1)
    _check_training(ectx, desc, rng.randint(0, K, n).astype(np.int32), K, P, "K = %d" % K)
    if K == 33:
        tau, counts = _check_training(ectx, desc, np.full(n, 5, np.int32), K, P, "a word that holds all the keys")
        assert counts[5] == n and counts.sum() == n and (tau[np.arange(K) != 5] == 0).all()


@pytest.mark.gpu
def test_thresholds_equal_values_duplicates_and_negative_z(ectx):
    rng = np.random.RandomState(21)
    P = hesaff_amd.embedding_projection(21)
    # all values equal: every key of a word is the same descriptor
    row = rng.randint(0, 256, (1, 128)).astype(np.uint8)
    desc = np.repeat(row, 130, axis=0)
    tau, _ = _check_training(ectx, desc, (np.arange(130) % 2).astype(np.int32), 2, P, "all equal")
    assert np.array_equal(tau[0], E.project(P, row)[0]) and np.array_equal(tau[1], tau[0])
    # duplicates straddling the median: one-hot rows over bytes of {7, 8}, so z takes two values, about half each, at even and odd m
    H = _one_hot()
    for m in (64, 65, 257):
        d = (7 + rng.randint(0, 2, (m, 128))).astype(np.uint8)
        d[: (m - 1) // 2 + 1, 0] = 7; d[(m - 1) // 2 + 1:, 0] = 8      # the median is the last 7
        d[: (m - 1) // 2, 1] = 7; d[(m - 1) // 2:, 1] = 8              # the median is the first 8
        tau, _ = _check_training(ectx, d[rng.permutation(m)], np.zeros(m, np.int32), 1, H, "duplicates, m = %d" % m)
        assert tau[0, 0] == 7 and tau[0, 1] == 8
    # negative z, down to the lower end of the range
    N = -np.abs(P)
    d = rng.randint(0, 256, (200, 128)).astype(np.uint8)
    d[:120] = 255
    tau, _ = _check_training(ectx, d, (np.arange(200) % 3).astype(np.int32), 3, N, "negative z")
    assert (tau < 0).all()
    tau, _ = _check_training(ectx, np.full((5, 128), 255, np.uint8), np.zeros(5, np.int32), 1, np.full((64, 128), -127, np.int8), "the lower end")
    assert (tau == -Z_MAX).all()
    tau, _ = _check_training(ectx, np.full((4, 128), 255, np.uint8), np.zeros(4, np.int32), 1, np.full((64, 128), 127, np.int8), "the upper end")
    assert (tau == Z_MAX).all()


@pytest.mark.gpu
def test_training_leaves_the_context_alone(ectx):
    rng = np.random.RandomState(30)
    P = hesaff_amd.embedding_projection(30)
    tau = rng.randint(-1000, 1000, (33, 64)).astype(np.int32)
    _with_embedding(ectx, 33, P, tau)
    desc = rng.randint(0, 256, (100, 128)).astype(np.uint8)
    before = ectx.embed(desc, np.arange(100, dtype=np.int32) % 33)
    ectx.train_embedding(desc, rng.randint(0, 7, 100).astype(np.int32), hesaff_amd.embedding_projection(31), 7)
    got_P, got_tau = ectx.embedding()
    assert np.array_equal(got_P, P) and np.array_equal(got_tau, tau) and ectx.vocabulary_size == 33
    assert np.array_equal(ectx.embed(desc, np.arange(100, dtype=np.int32) % 33), before)
    ectx.set_vocabulary(None)
    assert ectx.embedding() is None


# ---------------------------------------------------------------- the embedded index

K_IDX = 9
LIST_SIZES = [0, 1, 63, 64, 65, 200, 8, 5]   # keys of words 0 .. 7; word 8: one key in every image (idf 0)


@pytest.fixture(scope="module")
def collection():
    """8 images over 9 words: key lists of length 0, 1, 63, 64, 65 and 200; several keys of one image in one word; a word of every
    image, which is all the last image holds.  Signatures: a base per word with 0 .. 40 bits flipped, so that every threshold of the
    sweep admits some pairs and refuses others."""
    rng = np.random.RandomState(40)
    N = 8
    words = [[] for _ in range(N)]
    for w, m in enumerate(LIST_SIZES):
        owners = rng.randint(0, N - 1, m)
        if w == 6:
            owners[:] = 2                           # eight keys of one image in one word
        for i in owners:
            words[i].append(w)
    for i in range(N):
        words[i].append(8)
    words = [np.array(rng.permutation(w), np.int32) for w in words]
    base = rng.randint(0, 1 << 32, K_IDX).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, K_IDX).astype(np.uint64)

    def sig_of(w):
        g = base[w]
        for b in rng.permutation(64)[: rng.randint(0, 41)]:
            g ^= np.uint64(1) << np.uint64(b)
        return g
    sigs = [np.array([sig_of(w) for w in ws], np.uint64) for ws in words]
    ref = R.build(words, K_IDX)
    for a in ref[1:]:
        a.setflags(write=False)
    return words, sigs, ref, base


def _check_embedded_query(ctx, collection, qw, qs, T, top, what, device=False):
    words, sigs, ref, _ = collection
    want_im, want_sc, want_dot, want_score, want_nq2 = E.query(ref, words, sigs, qw, qs, T, top)
    if device:
        import torch
        tw = torch.from_numpy(np.ascontiguousarray(qw) if len(qw) else np.zeros(1, np.int32)).cuda()
        ts = torch.from_numpy(np.ascontiguousarray(qs).view(np.int64) if len(qs) else np.zeros(1, np.int64)).cuda()
        torch.cuda.synchronize()
        im, sc = ctx.query_embedded_index_device(tw.data_ptr(), ts.data_ptr(), len(qw), 1, T, top)
    else:
        im, sc = ctx.query_index(qw, top, signatures=qs, hamming=T)
    dot, score, nq2 = ctx.index_scores()
    assert nq2 == want_nq2, (what, "nq2")
    assert np.array_equal(dot, want_dot), (what, "dot", dot.tolist(), want_dot.tolist())
    assert np.array_equal(_bits(score), _bits(want_score)), (what, "scores")
    assert im.tolist() == want_im.tolist() and np.array_equal(_bits(sc), _bits(want_sc)), (what, "ranking")
    return dot


@pytest.mark.gpu
def test_embedded_build_equals_the_plain_build(ectx, collection):
    words, sigs, ref, _ = collection
    ectx.build_index(words, K_IDX)
    plain = [a.copy() for a in ectx.index_tables()]
    assert ectx.index_embedded() is None
    ectx.build_embedded_index(words, sigs, K_IDX)
    df, idf, norm2 = ectx.index_tables()
    for got, want, pl in zip((df, idf, norm2), ref[1:], plain):
        assert np.array_equal(got, want) and got.tobytes() == pl.tobytes()
    assert idf[8] == 0 and df[8] == len(words) and df[0] == 0
    assert ectx.index_info == (len(words), K_IDX, sum(len(w) for w in words), int(ref[1].sum()))
    # the key lists: per word the multiset of (image, signature), in any order
    offsets, images, lsigs = ectx.index_embedded()
    assert offsets[0] == 0 and offsets[-1] == sum(len(w) for w in words)
    assert np.diff(offsets.astype(np.int64)).tolist() == LIST_SIZES + [len(words)]
    for w in range(K_IDX):
        got = sorted(zip(images[offsets[w]:offsets[w + 1]].tolist(), lsigs[offsets[w]:offsets[w + 1]].tolist()))
        want = sorted((i, int(g)) for i, (ws, gs) in enumerate(zip(words, sigs)) for x, g in zip(ws, gs) if x == w)
        assert got == want, w
    # the device form from (word, dist2) rows gives the same index
    import torch
    rows = np.concatenate([np.stack([w, np.full(len(w), -5, np.int32)], axis=1) for w in words])
    tw = torch.from_numpy(rows).cuda()
    ts = torch.from_numpy(np.concatenate(sigs).view(np.int64)).cuda()
    torch.cuda.synchronize()
    ectx.build_embedded_index_device(tw.data_ptr(), ts.data_ptr(), [len(w) for w in words], 2, K_IDX)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(ectx.index_tables(), plain))
    o2, i2, s2 = ectx.index_embedded()
    assert np.array_equal(o2, offsets) and sorted(zip(i2.tolist(), s2.tolist())) == sorted(zip(images.tolist(), lsigs.tolist()))


@pytest.mark.gpu
def test_embedded_query_thresholds(ectx, collection):
    """T = 64 is the plain query bit for bit; T in {0, 1, 31, 32, 63} against the reference; dot never decreases with T; a plain
    query on the embedded index; an empty query; queries A, B, A"""
    words, sigs, ref, base = collection
    ectx.build_embedded_index(words, sigs, K_IDX)
    rng = np.random.RandomState(41)
    qa_w = np.concatenate([words[1], [0, 0, 6, 6, 8]]).astype(np.int32)
    qa_s = np.concatenate([sigs[1], base[[0, 0, 6, 6, 8]]])
    qb_w = rng.randint(0, K_IDX, 40).astype(np.int32)
    qb_s = base[qb_w] ^ np.uint64(0xF0F0)
    for qw, qs, name in ((qa_w, qa_s, "A"), (qb_w, qb_s, "B")):
        want = R.query(ref, qw, 5)
        im, sc = ectx.query_index(qw, 5, signatures=qs, hamming=64)
        dot, score, nq2 = ectx.index_scores()
        assert im.tolist() == want[0].tolist() and np.array_equal(_bits(sc), _bits(want[1])) and nq2 == want[4]
        assert np.array_equal(dot, want[2]) and np.array_equal(_bits(score), _bits(want[3])), name
        im2, sc2 = ectx.query_index(qw, 5)    # the plain query on the embedded index
        dot2, score2, nq2b = ectx.index_scores()
        assert im2.tolist() == im.tolist() and sc2.tobytes() == sc.tobytes() and dot2.tobytes() == dot.tobytes() and nq2b == nq2
        last = None
        for T in (0, 1, 31, 32, 63, 64):
            dot = _check_embedded_query(ectx, collection, qw, qs, T, 4, "%s, T = %d" % (name, T), device=(T in (1, 32)))
            assert last is None or (dot >= last).all(), (name, T)
            last = dot
        assert _check_embedded_query(ectx, collection, qw, qs, 0, 4, name).sum() < last.sum()
    # A, B, A: the tables are clean again after every query
    first = _check_embedded_query(ectx, collection, qa_w, qa_s, 24, 8, "A")
    _check_embedded_query(ectx, collection, qb_w, qb_s, 24, 8, "B")
    again = _check_embedded_query(ectx, collection, qa_w, qa_s, 24, 8, "A again")
    assert first.tobytes() == again.tobytes()
    # n = 0: images 0, 1, .. with score 0
    for device in (False, True):
        _check_embedded_query(ectx, collection, np.zeros(0, np.int32), np.zeros(0, np.uint64), 10, 3, "empty", device=device)
    im, sc = ectx.query_index(np.zeros(0, np.int32), 3, signatures=np.zeros(0, np.uint64), hamming=0)
    assert im.tolist() == [0, 1, 2] and (sc == 0).all()


@pytest.mark.gpu
def test_embedded_query_threshold_is_inclusive(ectx):
    """one key per image in one word beside a second word, image i's signature i bits away from the query's: threshold T admits
    exactly the images 0 .. T"""
    N = 65
    sig = np.uint64(0x0123456789ABCDEF)
    sigs = [np.array([int(sig) ^ ((1 << i) - 1), 0], np.uint64) for i in range(N)]
    words = [np.array([0, 1 + (i & 1)], np.int32) for i in range(N)]
    words[7] = np.array([3, 3], np.int32)   # (so that word 0 is not in every image: its idf is not 0)
    ectx.build_embedded_index(words, sigs, 4)
    idf = ectx.index_tables()[1]
    assert idf[0] > 0
    for T in (0, 1, 31, 32, 63, 64):
        ectx.query_index(np.array([0], np.int32), 1, signatures=np.array([sig], np.uint64), hamming=T)
        dot = ectx.index_scores()[0]
        want = np.where((np.arange(N) <= T) & (np.arange(N) != 7), int(idf[0]) ** 2, 0).astype(np.uint64)
        assert np.array_equal(dot, want), T


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("device", [False, True])
def test_embedded_build_and_query_forms_at_one_small_shape(ectx, device, stride):
    """hesaff_index_build_embedded[_device] and hesaff_index_query_embedded[_device] at word_stride 1 and 2: 3 images over K = 5 with
    the middle one empty, a query with repeats and a query of 0 words; a whole build of 0 words; and the first or the last word at
    -1 or K, refused under the entry point's own name with the index left as it was.  Everything here is host plumbing and per-key
    device code with no tile size in it, so the shape is small."""
    import torch
    K = 5
    words = [np.array([0, 3, 3, 4, 1, 0, 3], np.int32), np.zeros(0, np.int32), np.array([4, 2], np.int32)]
    sigs = [np.array([1, 2, 3, 0xFF, 5, 1, 7], np.uint64), np.zeros(0, np.uint64), np.array([0xF0, 9], np.uint64)]
    rows = (lambda w: np.stack([w, np.full(len(w), -7, np.int32)], axis=1)) if stride == 2 else (lambda w: w)

    def on_device(a):
        t = torch.from_numpy(np.ascontiguousarray(a) if a.size else np.zeros(2, a.dtype)).cuda()
        torch.cuda.synchronize()
        return t

    def build(ws, gs):
        if device:
            tw, ts = on_device(np.concatenate([rows(w) for w in ws])), on_device(np.concatenate(gs).view(np.int64))
            ectx.build_embedded_index_device(tw.data_ptr(), ts.data_ptr(), [len(w) for w in ws], stride, K)
        else:
            ectx.build_embedded_index([rows(w) for w in ws], gs, K)

    def query(qw, qs, T, top):
        if device:
            tw, ts = on_device(rows(qw)), on_device(qs.view(np.int64))
            return ectx.query_embedded_index_device(tw.data_ptr(), ts.data_ptr(), len(qw), stride, T, top)
        return ectx.query_index(rows(qw), top, signatures=qs, hamming=T)

    def check(ws, gs, what):
        ref = R.build(ws, K)
        df, idf, norm2 = ectx.index_tables()
        assert np.array_equal(df, ref[1]) and np.array_equal(idf, ref[2]) and np.array_equal(norm2, ref[3]), what
        assert ectx.index_info == (3, K, sum(len(w) for w in ws), int(ref[1].sum())), what
        offsets, images, lsigs = ectx.index_embedded()
        assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(np.bincount(np.concatenate(ws), minlength=K))])), what
        for w in range(K):
            got = sorted(zip(images[offsets[w]:offsets[w + 1]].tolist(), lsigs[offsets[w]:offsets[w + 1]].tolist()))
            assert got == sorted((i, int(g)) for i, (a, b) in enumerate(zip(ws, gs)) for x, g in zip(a, b) if x == w), (what, w)
        for qw, qs in ((np.array([3, 0, 3, 4], np.int32), np.array([3, 1, 6, 0xF1], np.uint64)), (np.zeros(0, np.int32), np.zeros(0, np.uint64))):
            for T in (0, 1, 64):
                want = E.query(ref, ws, gs, qw, qs, T, 3)
                im, sc = query(qw, qs, T, 3)
                dot, score, nq2 = ectx.index_scores()
                assert nq2 == want[4] and np.array_equal(dot, want[2]) and np.array_equal(_bits(score), _bits(want[3])), (what, len(qw), T)
                assert im.tolist() == want[0].tolist() and np.array_equal(_bits(sc), _bits(want[1])), (what, len(qw), T)

    what = "device %s, stride %d" % (device, stride)
    build([w[:0] for w in words], [g[:0] for g in sigs])
    check([w[:0] for w in words], [g[:0] for g in sigs], what + ", no word at all")
    build(words, sigs)
    check(words, sigs, what)
    suffix = "_device" if device else ""
    for at, w in ((0, -1), (0, K), (-1, -1), (-1, K)):
        bad = [a.copy() for a in words]
        bad[0 if at == 0 else 2][at] = w
        bad_query = np.array([3, 0, 4], np.int32)
        bad_query[at] = w
        with pytest.raises(hesaff_amd.HesaffError, match=r"hesaff_index_build_embedded%s: a word lies outside 0 \.\. vocabulary_size - 1$" % suffix):
            build(bad, sigs)
        with pytest.raises(hesaff_amd.HesaffError, match=r"hesaff_index_query_embedded%s: a word lies outside 0 \.\. vocabulary_size - 1$" % suffix):
            query(bad_query, np.array([3, 1, 0xF1], np.uint64), 8, 2)
    check(words, sigs, what + ", after the refusals")


@pytest.mark.gpu
def test_refusals_leave_the_index_the_vocabulary_and_the_embedding(ectx, collection):
    words, sigs, ref, base = collection
    L, h = ectx.L, ectx.h
    P = hesaff_amd.embedding_projection(50)
    tau = np.random.RandomState(50).randint(-5000, 5000, (33, 64)).astype(np.int32)
    im = np.zeros(4, np.int32); sc = np.zeros(4, np.float64); n = C.c_int()
    one = np.zeros(1, np.int32); sig = np.zeros(1, np.uint64); desc = np.zeros((1, 128), np.uint8)
    # no vocabulary, then no embedding
    ectx.set_vocabulary(None)
    assert L.hesaff_set_embedding(h, P.ctypes.data, tau.ctypes.data) == ARG and ectx.embedding() is None
    assert L.hesaff_stage_embed(h, 1, desc.ctypes.data, one.ctypes.data, 1, sig.ctypes.data) == ARG
    ectx.set_vocabulary(V.family("uniform", 33, seed=1))
    assert L.hesaff_stage_embed(h, 1, desc.ctypes.data, one.ctypes.data, 1, sig.ctypes.data) == ARG
    assert L.hesaff_get_signatures(h, 0, C.byref(C.c_void_p()), C.byref(n)) == ARG
    assert L.hesaff_get_signatures_device(h, C.byref(C.c_void_p()), C.byref(C.c_int64())) == ARG
    # an embedded query on a plain index, and with no index
    ectx.clear_index()
    assert L.hesaff_index_query_embedded(h, 1, one.ctypes.data, 1, sig.ctypes.data, 64, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)) == ARG
    ectx.build_index(words, K_IDX)
    assert L.hesaff_index_query_embedded(h, 1, one.ctypes.data, 1, sig.ctypes.data, 64, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)) == ARG
    assert L.hesaff_index_get_embedded(h, C.byref(n), one.ctypes.data, None, None) == ARG
    ectx.set_embedding(P, tau)
    ectx.build_embedded_index(words, sigs, K_IDX)
    state = [a.tobytes() for a in ectx.index_tables()] + [a.tobytes() for a in ectx.index_embedded()]
    keep = ectx.embed(np.full((3, 128), 9, np.uint8), np.array([0, 5, 32], np.int32))
    bad_P = P.copy(); bad_P[17, 3] = -128
    flat_w = np.concatenate(words); flat_s = np.concatenate(sigs); counts = np.array([len(w) for w in words], np.int32)
    out_of_range = flat_w.copy(); out_of_range[5] = K_IDX
    refusals = [
        L.hesaff_set_embedding(h, bad_P.ctypes.data, tau.ctypes.data),                       # an entry of -128
        L.hesaff_set_embedding(h, P.ctypes.data, None), L.hesaff_set_embedding(h, None, tau.ctypes.data),
        L.hesaff_stage_project(h, 1, desc.ctypes.data, bad_P.ctypes.data, np.zeros(64, np.int32).ctypes.data),
        L.hesaff_stage_embed(h, 1, desc.ctypes.data, np.array([33], np.int32).ctypes.data, 1, sig.ctypes.data),   # a word out of range
        L.hesaff_stage_embed(h, 1, desc.ctypes.data, np.array([-1], np.int32).ctypes.data, 1, sig.ctypes.data),
        L.hesaff_stage_embed(h, 1, desc.ctypes.data, one.ctypes.data, 3, sig.ctypes.data),
        L.hesaff_stage_embed(h, 1, None, one.ctypes.data, 1, sig.ctypes.data),
        L.hesaff_train_embedding(h, 1, desc.ctypes.data, np.array([2], np.int32).ctypes.data, 1, 2, P.ctypes.data, tau.ctypes.data, None),
        L.hesaff_train_embedding(h, 0, desc.ctypes.data, one.ctypes.data, 1, 2, P.ctypes.data, tau.ctypes.data, None),
        L.hesaff_train_embedding(h, (1 << 24) + 1, desc.ctypes.data, one.ctypes.data, 1, 2, P.ctypes.data, tau.ctypes.data, None),
        L.hesaff_train_embedding(h, 1, desc.ctypes.data, one.ctypes.data, 1, 2, bad_P.ctypes.data, tau.ctypes.data, None),
        L.hesaff_train_embedding(h, 1, desc.ctypes.data, one.ctypes.data, 1, 2, P.ctypes.data, None, None),
        L.hesaff_index_build_embedded(h, len(words), counts.ctypes.data, out_of_range.ctypes.data, 1, flat_s.ctypes.data, K_IDX),
        L.hesaff_index_build_embedded(h, len(words), counts.ctypes.data, flat_w.ctypes.data, 1, None, K_IDX),
        L.hesaff_index_build_embedded(h, 0, counts.ctypes.data, flat_w.ctypes.data, 1, flat_s.ctypes.data, K_IDX),
        L.hesaff_index_query_embedded(h, 1, one.ctypes.data, 1, sig.ctypes.data, -1, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)),
        L.hesaff_index_query_embedded(h, 1, one.ctypes.data, 1, sig.ctypes.data, 65, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)),
        L.hesaff_index_query_embedded(h, 1, np.array([K_IDX], np.int32).ctypes.data, 1, sig.ctypes.data, 8, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)),
        L.hesaff_index_query_embedded(h, 1, one.ctypes.data, 1, None, 8, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)),
        L.hesaff_index_query_embedded(h, 1, one.ctypes.data, 1, sig.ctypes.data, 8, 0, im.ctypes.data, sc.ctypes.data, C.byref(n)),
    ]
    import torch
    t = torch.zeros(64, dtype=torch.int64).cuda()
    torch.cuda.synchronize()
    p = t.data_ptr()
    refusals += [
        L.hesaff_embed_device(h, 1, p, 128, 0, p, 1, p + 4),            # signatures need 8-byte alignment
        L.hesaff_embed_device(h, 1, p + 2, 128, 0, p, 1, p), L.hesaff_embed_device(h, 1, p, 128, 0, p + 2, 1, p),
        L.hesaff_embed_device(h, 1, p, 126, 0, p, 1, p), L.hesaff_embed_device(h, 1, p, 128, 0, p, 0, p),
        L.hesaff_index_build_embedded_device(h, 1, np.array([1], np.int32).ctypes.data, p, 1, p + 4, K_IDX),
        L.hesaff_index_query_embedded_device(h, 1, p, 1, p + 4, 8, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)),
        L.hesaff_train_embedding_device(h, 1, p + 1, 128, 0, p, 1, 2, P.ctypes.data, tau.ctypes.data, None),
    ]
    assert refusals == [ARG] * len(refusals), refusals
    # everything is as it was, and works
    got_P, got_tau = ectx.embedding()
    assert np.array_equal(got_P, P) and np.array_equal(got_tau, tau) and ectx.vocabulary_size == 33
    assert [a.tobytes() for a in ectx.index_tables()] + [a.tobytes() for a in ectx.index_embedded()] == state
    assert np.array_equal(ectx.embed(np.full((3, 128), 9, np.uint8), np.array([0, 5, 32], np.int32)), keep)
    _check_embedded_query(ectx, collection, words[1], sigs[1], 20, 3, "after the refusals")
    # cells and probes leave the embedding; a new vocabulary removes it
    vocab = V.family("uniform", 33, seed=1)
    v2, _, coarse, first = ectx.build_vocabulary_cells(vocab, V.family("uniform", 4, seed=2))
    ectx.set_vocabulary_cells(coarse, first)
    ectx.set_vocabulary_probes(2)
    assert ectx.embedding() is not None
    ectx.set_vocabulary_cells(None)
    ectx.set_vocabulary_probes(1)
    assert ectx.embedding() is not None
    ectx.set_embedding(None)
    assert ectx.embedding() is None
    ectx.set_embedding(P, tau)
    ectx.set_vocabulary(vocab)
    assert ectx.embedding() is None
    ectx.set_vocabulary(None)
    ectx.clear_index()


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def e2e(ectx):
    """the five golden images detected with a vocabulary of 40 rows and no embedding: keys and (word, dist2) rows; a trained embedding"""
    vocab = V.family("uniform", 40, seed=71)
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    ectx.set_vocabulary(vocab)
    try:
        res = ectx.detect_batch(imgs)
        words = [ectx.words(i) for i in range(len(imgs))]
        with pytest.raises(hesaff_amd.HesaffError):
            ectx.signatures(0)
        desc = np.concatenate([k["desc"] for _, k in res])
        P = hesaff_amd.embedding_projection(71)
        tau, counts = ectx.train_embedding(desc, np.concatenate(words), P)
    finally:
        ectx.set_vocabulary(None)
    assert [len(k) for _, k in res] == E2E_KEYS
    want_tau, want_counts = E.thresholds(P, desc, np.concatenate(words)[:, 0], 40)
    assert np.array_equal(tau, want_tau) and np.array_equal(counts, want_counts)
    sigs = [E.signatures(P, tau, k["desc"], w[:, 0]) for (_, k), w in zip(res, words)]
    return imgs, res, words, vocab, P, tau, sigs


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["flat", "cells", "probes"])
def test_end_to_end_signatures_of_a_batch(ectx, e2e, mode):
    """detect_batch with a vocabulary and an embedding, through the flat assignment, a cell layer and two probes: signatures(i) is
    embed() of the returned descriptors and words, and the reference's; the keys are those of a context without an embedding"""
    imgs, res, words, vocab, P, tau, sigs = e2e
    try:
        if mode == "flat":
            ectx.set_vocabulary(vocab)
            ectx.set_embedding(P, tau)
            use_tau = tau
        else:
            v2, order, coarse, first = ectx.build_vocabulary_cells(vocab, V.family("uniform", 5, seed=72))
            ectx.set_vocabulary(v2)
            ectx.set_vocabulary_cells(coarse, first)
            ectx.set_vocabulary_probes(2 if mode == "probes" else 1)
            use_tau = np.ascontiguousarray(tau[order])
            ectx.set_embedding(P, use_tau)
        got = ectx.detect_batch(imgs)
        for i, ((nh, keys), (nh0, keys0)) in enumerate(zip(got, res)):
            assert nh == nh0 and keys.tobytes() == keys0.tobytes()
            w = ectx.words(i)
            g = ectx.signatures(i)
            assert g.dtype == np.uint64 and len(g) == len(keys) == len(w)
            assert np.array_equal(g, E.signatures(P, use_tau, keys["desc"], w[:, 0])), (mode, i)
            assert np.array_equal(g, ectx.embed(keys["desc"], w)), (mode, i)
            if mode == "flat":
                assert w.tobytes() == words[i].tobytes() and np.array_equal(g, sigs[i])
        with pytest.raises(hesaff_amd.HesaffError):
            ectx.signatures(len(imgs))
    finally:
        ectx.set_vocabulary_probes(1)
        ectx.set_vocabulary(None)


@pytest.mark.gpu
def test_end_to_end_device_resident_signatures(e2e):
    import torch
    imgs, res, words, vocab, P, tau, sigs = e2e
    img = imgs[0]
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_vocabulary(vocab)
        c.set_embedding(P, tau)
        t = torch.from_numpy(np.stack([img] * 3)).cuda()
        torch.cuda.synchronize()
        ch, cd, dkeys, total = c.detect_batch_device(t.data_ptr(), 3, img.shape[1], img.shape[0])
        assert total == 663
        ptr, rows = c.signatures_device()
        assert rows == 663 and ptr % 8 == 0
        got = torch.empty(663, dtype=torch.int64, device="cuda")
        hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        assert hip.hipMemcpy(C.c_void_p(got.data_ptr()), C.c_void_p(ptr), C.c_size_t(663 * 8), 3) == 0
        assert np.array_equal(got.cpu().numpy().view(np.uint64), np.concatenate([sigs[0]] * 3))
        # the index from the device-resident words and signatures, queried in place
        wptr, _ = c.words_device()
        # (the third copy cut in three, so that not every word lies in every image and idf is not 0 throughout)
        counts = [221, 221, 60, 80, 81]
        cuts = [(0, 221), (0, 221), (0, 60), (60, 140), (140, 221)]
        iw = [words[0][a:b, 0] for a, b in cuts]
        ig = [sigs[0][a:b] for a, b in cuts]
        c.build_embedded_index_device(wptr, ptr, counts, 2, 40)
        ref = R.build(iw, 40)
        for T in (0, 20):
            im, sc = c.query_embedded_index_device(wptr, ptr, 221, 2, T, 4)
            want = E.query(ref, iw, ig, iw[0], ig[0], T, 4)
            assert im.tolist() == want[0].tolist() and np.array_equal(_bits(sc), _bits(want[1])) and sc[0] > 0.0
            assert np.array_equal(c.index_scores()[0], want[2])
        c.set_embedding(None)
        with pytest.raises(hesaff_amd.HesaffError):
            c.signatures_device()
        assert c.words_device()[1] == 663


@pytest.mark.gpu
def test_process_files_writes_signature_files_and_cli_search(ectx, e2e, tmp_path):
    """HESAFF_OUT_WORDS with an embedding writes <image>.hesaff.sigs beside every words file; --resume counts it; without an
    embedding the words files are byte for byte the same and no signatures file appears; hesaff --search --hamming T prints the
    reference's ranking, and names a signatures file that is missing or of another count"""
    imgs, res, words, vocab, P, tau, sigs = e2e
    paths = []
    for j, name in enumerate(E2E_IMAGES):
        paths.append(str(tmp_path / ("%d_%s.pgm" % (j, name))))
        shutil.copy(os.path.join(GOLD, name + ".pgm"), paths[-1])
    plain_dir = tmp_path / "plain"
    plain_dir.mkdir()
    plain_outs = [str(plain_dir / ("%d.words" % j)) for j in range(5)]
    ectx.set_vocabulary(vocab)
    try:
        ectx.set_output_format(hesaff_amd.OUT_WORDS)
        st = ectx.process_files(paths, plain_outs)
        assert all(s[0] == 0 for s in st) and sorted(os.listdir(plain_dir)) == sorted(os.path.basename(o) for o in plain_outs)
        ectx.set_embedding(P, tau)
        ectx.set_output_format(hesaff_amd.OUT_TEXT | hesaff_amd.OUT_WORDS)
        st = ectx.process_files(paths)
        for j, p in enumerate(paths):
            assert st[j][0] == 0 and st[j][3] == E2E_KEYS[j]
            assert open(p + ".hesaff.words", "rb").read() == open(plain_outs[j], "rb").read()
            assert np.array_equal(hesaff_amd.read_signatures(p + ".hesaff.sigs"), sigs[j]), p
        # the words file alone under the caller's names: ".sigs" in the place of ".words", or appended
        ectx.set_output_format(hesaff_amd.OUT_WORDS)
        outs = [str(tmp_path / ("o%d.words" % j)) if j % 2 else str(tmp_path / ("o%d" % j)) for j in range(5)]
        st = ectx.process_files(paths, outs)
        for j, o in enumerate(outs):
            side = o[:-6] + ".sigs" if j % 2 else o + ".sigs"
            assert st[j][0] == 0 and open(o, "rb").read() == open(plain_outs[j], "rb").read()
            assert np.array_equal(hesaff_amd.read_signatures(side), sigs[j])
        # resume: a missing or cut signatures file makes the image's outputs again
        ectx.set_output_format(hesaff_amd.OUT_TEXT | hesaff_amd.OUT_WORDS)
        os.remove(paths[1] + ".hesaff.sigs")
        with open(paths[2] + ".hesaff.sigs", "r+b") as f:
            f.truncate(16 + 8 * 100)
        ectx.set_resume(True)
        st = ectx.process_files(paths)
        assert [s[1] for s in st] == [5, 3, 3, 5, 5], st   # HESAFF_FILE_SKIPPED, HESAFF_FILE_WRITTEN
        for j, p in enumerate(paths):
            assert np.array_equal(hesaff_amd.read_signatures(p + ".hesaff.sigs"), sigs[j])
    finally:
        ectx.set_resume(False)
        ectx.set_output_format(1)
        ectx.set_vocabulary(None)
    # the command-line search over the files
    wfiles = [p + ".hesaff.words" for p in paths]
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(wfiles) + "\n")
    iw = [w[:, 0] for w in words]
    ref = R.build(iw, 40)
    qs = sigs[1] ^ np.uint64(0x00FF00FF)   # the second image's keys, sixteen bits away from their signatures
    query = str(tmp_path / "query.hesaff.words")
    shutil.copy(wfiles[1], query)
    hesaff_amd.write_signatures(str(tmp_path / "query.hesaff.sigs"), qs)
    for T in (0, 16, 64):
        r = subprocess.run([EXE, "--search", str(lst), "--query", query, "--top", "5", "--hamming", str(T)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        want_im, want_sc = E.query(ref, iw, sigs, iw[1], qs, T, 5)[:2]
        lines = [l.split("\t") for l in r.stdout.strip().split("\n")]
        assert [l[1] for l in lines] == [wfiles[i] for i in want_im], T
        assert np.array_equal(_bits(np.array([float(l[2]) for l in lines])), _bits(want_sc)), T
    plain_run = subprocess.run([EXE, "--search", str(lst), "--query", query, "--top", "5"], capture_output=True, text=True, timeout=600)
    assert plain_run.returncode == 0 and plain_run.stdout == r.stdout   # T = 64 prints the plain search
    assert E.query(ref, iw, sigs, iw[1], qs, 0, 5)[2].sum() == 0 and E.query(ref, iw, sigs, iw[1], qs, 16, 5)[2].sum() > 0
    os.remove(paths[4] + ".hesaff.sigs")
    r = subprocess.run([EXE, "--search", str(lst), "--query", query, "--hamming", "16"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stdout == "" and (paths[4] + ".hesaff.sigs") in r.stderr
    hesaff_amd.write_signatures(paths[4] + ".hesaff.sigs", sigs[4][:-1])
    r = subprocess.run([EXE, "--search", str(lst), "--query", query, "--hamming", "16"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stdout == "" and (paths[4] + ".hesaff.sigs") in r.stderr and "73 signatures" in r.stderr
    r = subprocess.run([EXE, "--search", str(lst), "--query", query, "--hamming", "65"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "usage" in r.stderr


@pytest.mark.gpu
def test_cli_batch_with_an_embedding_file(e2e, tmp_path):
    """hesaff --batch --vocabulary v --train-embedding he.bin --seed S writes the embedding the library trains on the list's keys;
    --embedding he.bin then writes the signatures files; an embedding of another row count ends the run, named"""
    imgs, res, words, vocab, P, tau, sigs = e2e
    paths = []
    for j, name in enumerate(E2E_IMAGES):
        paths.append(str(tmp_path / ("%d_%s.pgm" % (j, name))))
        shutil.copy(os.path.join(GOLD, name + ".pgm"), paths[-1])
    lst = tmp_path / "images.txt"
    lst.write_text("\n".join(paths) + "\n")
    vfile, efile = str(tmp_path / "v.bin"), str(tmp_path / "he.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile, "--train-embedding", efile, "--seed", "71", "--devices", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "Trained the thresholds of 40 words on 590 keys of 5 images" in r.stdout, (r.stdout, r.stderr)
    got_P, got_tau = hesaff_amd.read_embedding(efile)
    assert np.array_equal(got_P, P) and np.array_equal(got_tau, tau)
    assert not any(f.endswith((".sift", ".words", ".sigs")) for f in os.listdir(tmp_path))
    r = subprocess.run([EXE, "--batch", str(lst), "--train-embedding", efile], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "usage" in r.stderr   # (needs --vocabulary)
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile, "--embedding", efile, "--devices", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for j, p in enumerate(paths):
        assert np.array_equal(hesaff_amd.read_signatures(p + ".hesaff.sigs"), sigs[j])
        assert np.array_equal(hesaff_amd.read_words(p + ".hesaff.words")[1]["word"], words[j][:, 0].astype(np.uint32))
    hesaff_amd.write_embedding(efile, P, tau[:39])
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile, "--embedding", efile, "--devices", "0"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and efile in r.stderr


def _fnv(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & ((1 << 64) - 1)
    return h


@pytest.mark.gpu
def test_end_to_end_cpp_members(e2e, tmp_path):
    """tests/native/embedding_search_keys.cpp: embeddingProjection, trainEmbedding, setEmbedding, signatures and the buildIndex /
    queryIndex overloads through hesaff.hpp hold what the Python path holds; an embedded query on a plain index is refused"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, res, words, vocab, P, tau, sigs = e2e
    exe = str(tmp_path / "embedding_search_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "embedding_search_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    r = subprocess.run([exe, vfile, "71", "20", "4"] + [os.path.join(GOLD, n + ".pgm") for n in E2E_IMAGES], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    iw = [w[:, 0] for w in words]
    want_im, want_sc = E.query(R.build(iw, 40), iw, sigs, iw[0], sigs[0], 20, 4)[:2]
    want = ["T %d" % _fnv(tau.tobytes())] + ["S %d %d %d" % (j, len(g), _fnv(g.tobytes())) for j, g in enumerate(sigs)]
    want += ["R %d %d %.17g" % (j + 1, i, v) for j, (i, v) in enumerate(zip(want_im, want_sc))] + ["P refused"]
    assert r.stdout.strip().split("\n") == want


@pytest.mark.gpu
def test_embedding_ms_are_event_times(ectx, e2e):
    imgs, res, words, vocab, P, tau, sigs = e2e
    ectx.set_vocabulary(vocab)
    ectx.set_embedding(P, tau)
    try:
        assert ectx.embedding_ms[0] == 0.0
        ectx.set_profiling(1)
        ectx.detect_batch(imgs[:3])   # (the time is that of the call's LAST batch: one whose images have keys)
        ectx.train_embedding(np.concatenate([k["desc"] for _, k in res]), np.concatenate(words), P)
        ms = ectx.embedding_ms
        assert all(0.0 < v < 1000.0 for v in ms), ms
    finally:
        ectx.set_profiling(0)
        ectx.set_vocabulary(None)
