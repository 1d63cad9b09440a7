"""GPU suite of the image index (hesaff_index_build / hesaff_index_query, include/hesaff_amd.h; kernels_index.h).  The reference is
tests/index_ref.py: the definition in numpy.  Every comparison is bit for bit - df, idf, norm2, dot, nq2, the float64 scores as
uint64 bit patterns, and the ranked images."""
import ctypes
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from tests import index_ref as R
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
E2E_IMAGES = ["band_160x120", "band_96x96", "band_160x120", "tiny_20x15", "band_96x96"]
E2E_KEYS = [221, 74, 221, 0, 74]
ARG = -2
MASK64 = (1 << 64) - 1


def hash_bits(total):
    """index_hash_bits of index_plan.h: the table has max(1024, the power of two >= 2 T) slots"""
    bits = 10
    while (1 << bits) < 2 * total:
        bits += 1
    return bits


def hash_slot(image, word, bits):
    """index_hash_slot of index_plan.h, the hash in use: the top bits of ((image << 20) | word) * 2^64 / phi"""
    return ((((image << 20) | word) * 0x9E3779B97F4A7C15) & MASK64) >> (64 - bits)


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def ictx():
    with hesaff_amd.HesaffContext(_params(max_batch=5), device=0) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _check_tables(ctx, ref, images, K, what):
    df, idf, norm2 = ctx.index_tables()
    assert df.dtype == np.uint32 and idf.dtype == np.uint32 and norm2.dtype == np.uint64
    assert np.array_equal(df, ref[1]), (what, "df")
    assert np.array_equal(idf, ref[2]), (what, "idf")
    assert np.array_equal(norm2, ref[3]), (what, "norm2")
    assert ctx.index_info == (len(images), K, sum(len(w) for w in images), int(ref[1].sum())), (what, ctx.index_info)


def _check_query(ctx, ref, words, top, what, device=False):
    want_im, want_sc, want_dot, want_score, want_nq2 = R.query(ref, words[:, 0] if words.ndim == 2 else words, top)
    if device:
        import torch
        t = torch.from_numpy(np.ascontiguousarray(words) if len(words) else np.zeros(1, np.int32)).cuda()
        torch.cuda.synchronize()
        im, sc = ctx.query_index_device(t.data_ptr(), len(words), words.ndim, top)
    else:
        im, sc = ctx.query_index(words, top)
    assert im.dtype == np.int32 and sc.dtype == np.float64 and len(im) == len(sc) == min(top, len(ref[0])), (what, len(im))
    dot, score, nq2 = ctx.index_scores()
    assert nq2 == want_nq2, (what, "nq2", nq2, want_nq2)
    assert np.array_equal(dot, want_dot), (what, "dot", np.nonzero(dot != want_dot)[0][:8].tolist())
    assert np.array_equal(_bits(score), _bits(want_score)), (what, "scores of every image")
    assert im.tolist() == want_im.tolist(), (what, "ranked images", im[:8].tolist(), want_im[:8].tolist())
    assert np.array_equal(_bits(sc), _bits(want_sc)), (what, "ranked scores")
    return im, sc


def _check_build(ctx, images, K, what, queries=(), device=False, stride=1, ref=None):
    images = [np.asarray(w, np.int32) for w in images]
    if stride == 2:   # (word, dist2) rows; dist2 is never read as a word
        images = [np.stack([w, np.full(len(w), -7, np.int32)], axis=1) if len(w) else np.zeros((0, 2), np.int32) for w in images]
    if device:
        import torch
        flat = np.concatenate(images) if sum(len(w) for w in images) else np.zeros((1,) if stride == 1 else (1, 2), np.int32)
        t = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
        torch.cuda.synchronize()
        ctx.build_index_device(t.data_ptr(), [len(w) for w in images], stride, K)
        assert np.array_equal(t.cpu().numpy(), flat)   # the source is only read
    else:
        ctx.build_index(images, K)
    if ref is None:
        ref = R.build([w[:, 0] if stride == 2 else w for w in images], K)
    _check_tables(ctx, ref, images, K, what)
    for q, top in queries:
        _check_query(ctx, ref, np.asarray(q, np.int32), top, what + ", query of %d words, top %d" % (len(q), top))
    return ref


def _collection(N, K, seed):
    """N images of 0 .. 40 random words; with N >= 3 the first, the middle and the last image have no key; word K - 1 lies in
    exactly one image"""
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, max(K - 1, 1), rng.randint(0, 41)).astype(np.int32) for _ in range(N)]
    if N >= 3:
        for i in (0, N // 2, N - 1):
            images[i] = np.zeros(0, np.int32)
    one = 1 if N >= 3 else 0
    images[one] = np.concatenate([images[one], [K - 1, K - 1]]).astype(np.int32)
    return images


# ---------------------------------------------------------------- build

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 33, 4099, 1 << 20])
def test_build_shapes(ictx, K):
    """N in {1, 2, 3, 65, 257} at this K: images of 0 keys first, in the middle and last, a word in exactly one image, host and
    device sources, word_stride 1 and 2, and two queries each (an indexed image, and random words with repeats)"""
    for N in (1, 2, 3, 65, 257):
        images = _collection(N, K, seed=100 + N)
        rng = np.random.RandomState(7 + N)
        queries = [(images[1 if N >= 3 else 0], 5), (rng.randint(0, K, 50), N)]
        ref = _check_build(ictx, images, K, "N = %d, K = %d, host" % (N, K), queries)
        for device, stride in ((True, 1), (False, 2), (True, 2)):
            _check_build(ictx, images, K, "N = %d, K = %d, device %s, stride %d" % (N, K, device, stride), device=device, stride=stride, ref=ref)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("device", [False, True])
def test_build_and_query_forms_at_one_small_shape(ictx, device, stride):
    """hesaff_index_build[_device] and hesaff_index_query[_device] at word_stride 1 and 2: 3 images over K = 5 with the middle one
    empty, a query with repeats and a query of 0 words; a whole build of 0 words; and the first or the last word at -1 or K, refused
    under the entry point's own name with the index left as it was.  Everything here is host plumbing and per-key device code with
    no tile size in it, so the shape is small."""
    import torch
    K = 5
    images = [np.array([0, 3, 3, 4, 1, 0, 3], np.int32), np.zeros(0, np.int32), np.array([4, 2], np.int32)]
    rows = (lambda w: np.stack([w, np.full(len(w), -7, np.int32)], axis=1)) if stride == 2 else (lambda w: w)
    what = "device %s, stride %d" % (device, stride)
    _check_build(ictx, [np.zeros(0, np.int32)] * 3, K, what + ", no word at all", device=device, stride=stride)
    assert ictx.index_info == (3, K, 0, 0)
    _check_query(ictx, R.build([[], [], []], K), rows(np.array([1, 1, 4], np.int32)), 2, what + ", against the empty index", device=device)
    ref = _check_build(ictx, images, K, what, device=device, stride=stride)
    for q, top in ((np.array([3, 0, 3, 4], np.int32), 3), (np.zeros(0, np.int32), 2)):
        _check_query(ictx, ref, rows(q), top, what + ", query of %d words" % len(q), device=device)
    suffix = "_device" if device else ""
    for at, w in ((0, -1), (0, K), (-1, -1), (-1, K)):
        bad_images = [a.copy() for a in images]
        bad_images[0 if at == 0 else 2][at] = w
        bad_query = np.array([3, 0, 4], np.int32)
        bad_query[at] = w
        with pytest.raises(hesaff_amd.HesaffError, match=r"hesaff_index_build%s: a word lies outside 0 \.\. vocabulary_size - 1$" % suffix):
            if device:
                t = torch.from_numpy(np.ascontiguousarray(np.concatenate([rows(a) for a in bad_images]))).cuda()
                torch.cuda.synchronize()
                ictx.build_index_device(t.data_ptr(), [len(a) for a in bad_images], stride, K)
            else:
                ictx.build_index([rows(a) for a in bad_images], K)
        with pytest.raises(hesaff_amd.HesaffError, match=r"hesaff_index_query%s: a word lies outside 0 \.\. vocabulary_size - 1$" % suffix):
            if device:
                t = torch.from_numpy(np.ascontiguousarray(rows(bad_query))).cuda()
                torch.cuda.synchronize()
                ictx.query_index_device(t.data_ptr(), len(bad_query), stride, 2)
            else:
                ictx.query_index(rows(bad_query), 2)
    _check_tables(ictx, ref, images, K, what + ", after the refusals")


@pytest.mark.gpu
def test_build_word_patterns(ictx):
    """all 4099 keys of an image in one word (one slot takes every atomic); every key a different word; a word in every image
    (idf 0) beside a word in exactly one; 257 images of one key each; a second build replacing the first"""
    one_word = [np.full(4099, 17, np.int32), np.array([17, 3], np.int32), np.array([3], np.int32)]
    ref = _check_build(ictx, one_word, 33, "4099 keys in one word", [(np.full(4099, 17, np.int32), 3), ([17], 3), ([3, 3, 17], 2)])
    assert ref[1][17] == 2 and ref[0][0][1].tolist() == [4099]
    distinct = [np.arange(4099, dtype=np.int32), np.arange(4099, dtype=np.int32)[::-1].copy(), np.arange(0, 4099, 2, dtype=np.int32)]
    _check_build(ictx, distinct, 4099, "every key a different word", [(np.arange(1, 4099, 2), 3), (np.arange(0, 4099, 2), 3)])
    everywhere = [np.array([0, 5], np.int32), np.array([0, 0, 6], np.int32), np.array([0], np.int32), np.array([0, 7, 7], np.int32)]
    ref = _check_build(ictx, everywhere, 8, "a word in every image", [([0], 4), ([0, 0, 7], 4), ([5, 6, 7], 2)])
    assert ref[2][0] == 0 and ref[1][0] == 4 and ref[1][5] == 1 and ref[2][5] == 512 and ref[3][2] == 0
    singles = [np.array([i % 33], np.int32) for i in range(257)]
    _check_build(ictx, singles, 33, "257 images of one key", [([5], 257), ([5, 6, 6], 10)])
    # the build before this one is gone: the tables are those of the last build alone
    _check_build(ictx, everywhere, 8, "a second build replaces the first", [([7], 4)])
    assert ictx.index_info == (4, 8, 9, 7)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [511, 512, 513])
def test_build_around_the_minimum_table_size(ictx, T):
    """T keys around the smallest table (1024 slots for T <= 512, 2048 beyond): distinct words of image 0 and 1 chosen from K = 4099
    so that their first slots are the LAST of the table - several keys per slot, and the probing wraps round to slot 0"""
    bits = hash_bits(T)
    assert (1 << bits) == (1024 if T <= 512 else 2048)
    half = T // 2
    picks = []
    for image, n in ((0, half), (1, T - half)):
        words = sorted(range(4099), key=lambda w: -hash_slot(image, w, bits))[:n]
        slots = [hash_slot(image, w, bits) for w in words]
        assert len(set(slots)) < len(slots)   # several keys share a first slot
        picks.append(np.array(words, np.int32))
    filled = sum(len(p) for p in picks)
    assert filled == T and min(hash_slot(i, int(w), bits) for i, p in enumerate(picks) for w in p) + T > (1 << bits)   # the run wraps
    rng = np.random.RandomState(T)
    images = [rng.permutation(picks[0]).astype(np.int32), rng.permutation(picks[1]).astype(np.int32), np.zeros(0, np.int32)]
    _check_build(ictx, images, 4099, "T = %d" % T, [(picks[0][:40], 3), (np.concatenate([picks[1][:9], picks[1][:9]]), 2)])
    _check_build(ictx, images, 4099, "T = %d, device" % T, device=True)


@pytest.mark.gpu
def test_build_colliding_words(ictx):
    """words of one image that all share ONE first slot under the hash in use (K = 2^20 leaves about 1000 per slot at 1024 slots), each
    twice, beside an image that holds every other one of them"""
    bits = hash_bits(200)
    same = list(itertools.islice((w for w in range(1 << 20) if hash_slot(0, w, bits) == 513), 100))
    assert len(same) == 100
    images = [np.repeat(np.array(same, np.int32), 2), np.array(same[::2], np.int32)]
    assert len(images[0]) + len(images[1]) <= 256
    ref = _check_build(ictx, images, 1 << 20, "one first slot", [(same[:10], 2), (same[1::2], 2)])
    assert ref[1][same[0]] == 2 and ref[1][same[1]] == 1


@pytest.mark.gpu
def test_build_largest_tf(ictx):
    """one image of 2^18 keys of one word beside two small ones: tf = 2^18, (tf idf)^2 and, queried with the same 2^18 words,
    tfq tf idf^2 = 2^36 * 149^2"""
    big = np.full(1 << 18, 1, np.int32)
    images = [big, np.array([0, 1], np.int32), np.array([0], np.int32)]
    ref = _check_build(ictx, images, 2, "tf = 2^18", [([1], 1)])
    assert ref[2][1] == 149 and int(ref[3][0]) == ((1 << 18) * 149) ** 2
    dot, _, nq2 = ictx.index_scores()
    assert int(dot[0]) == 149 ** 2 * (1 << 18) and nq2 == 149 ** 2
    _check_query(ictx, ref, big, 3, "tfq = 2^18")
    dot, _, nq2 = ictx.index_scores()
    assert int(dot[0]) == (1 << 36) * 149 ** 2 and nq2 == ((1 << 18) * 149) ** 2


# ---------------------------------------------------------------- query

@pytest.fixture(scope="module")
def qindex(ictx):
    """N = 66, K = 64: 64 random images, image 64 equal to image 7, image 65 without keys; word 0 in every image with keys but one
    (idf 5), word 63 in none"""
    rng = np.random.RandomState(21)
    images = [np.concatenate([[0], rng.randint(1, 63, rng.randint(1, 60))]).astype(np.int32) for _ in range(64)]
    images[3] = images[3][1:]
    images += [images[7].copy(), np.zeros(0, np.int32)]
    return images


def _build_q(ictx, qindex):
    ictx.build_index(qindex, 64)
    ref = R.build(qindex, 64)
    return ref


@pytest.mark.gpu
def test_query_edge_cases(ictx, qindex):
    ref = _build_q(ictx, qindex)
    N = len(qindex)
    assert ref[1][63] == 0 and ref[2][63] == 0 and ref[1][0] == 64
    # n = 0: images 0, 1, .. with score 0
    im, sc = _check_query(ictx, ref, np.zeros(0, np.int32), 5, "n = 0")
    assert im.tolist() == [0, 1, 2, 3, 4] and (sc == 0.0).all() and ictx.index_scores()[2] == 0
    # a word with df = 0 alone, and beside others; tfq = 1 and tfq = 4099
    im, sc = _check_query(ictx, ref, np.array([63], np.int32), 3, "df = 0")
    assert im.tolist() == [0, 1, 2] and (sc == 0.0).all()
    _check_query(ictx, ref, np.array([63, 5, 63, 9], np.int32), N, "df = 0 among others")
    _check_query(ictx, ref, np.array([5], np.int32), N, "tfq = 1")
    _check_query(ictx, ref, np.full(4099, 5, np.int32), N, "tfq = 4099")
    _check_query(ictx, ref, np.concatenate([np.full(4099, 5), np.arange(1, 63)]).astype(np.int32), N, "tfq = 4099 among others")
    # the query equal to an indexed image: the image and its twin tie at the top, the lower index first; top cuts between them
    im, sc = _check_query(ictx, ref, qindex[7], 2, "an indexed image")
    assert im.tolist() == [7, 64] and sc[0] == sc[1] and abs(sc[0] - 1.0) < 1e-15
    im, sc = _check_query(ictx, ref, qindex[7], 1, "top cuts between equal images")
    assert im.tolist() == [7]
    # top = N, top > N, top = 1024; device source and (word, dist2) rows
    assert len(_check_query(ictx, ref, qindex[9], N, "top = N")[0]) == N
    im, sc = _check_query(ictx, ref, qindex[9], N + 1, "top > N")
    assert len(im) == N and im[-1] == 65 and sc[-1] == 0.0
    assert len(_check_query(ictx, ref, qindex[9], 1024, "top = 1024")[0]) == N
    _check_query(ictx, ref, qindex[11], 7, "device", device=True)
    _check_query(ictx, ref, np.stack([qindex[11], np.full(len(qindex[11]), 1 << 30, np.int32)], axis=1), 7, "device rows", device=True)
    _check_query(ictx, ref, np.stack([qindex[11], np.full(len(qindex[11]), -1, np.int32)], axis=1), 7, "host rows")
    _check_query(ictx, ref, np.zeros(0, np.int32), 3, "n = 0, device", device=True)


@pytest.mark.gpu
def test_query_word_of_every_image(ictx):
    """idf = 0: a query of that word alone scores nothing, and beside another word it adds nothing"""
    images = [np.array([0, 5], np.int32), np.array([0, 0, 6], np.int32), np.array([0, 5, 5], np.int32)]
    ref = _check_build(ictx, images, 8, "idf 0")
    assert ref[2][0] == 0
    im, sc = _check_query(ictx, ref, np.array([0, 0, 0], np.int32), 3, "idf = 0 alone")
    assert im.tolist() == [0, 1, 2] and (sc == 0.0).all()
    a = _check_query(ictx, ref, np.array([5], np.int32), 3, "another word")
    b = _check_query(ictx, ref, np.array([0, 5, 0], np.int32), 3, "idf = 0 beside it")
    assert a[0].tolist() == b[0].tolist() == [0, 2, 1] and np.array_equal(_bits(a[1]), _bits(b[1]))


@pytest.mark.gpu
def test_queries_a_b_a_restore_the_tables(ictx, qindex):
    """A, B, A on one index: the third answer is byte-equal to the first - tfq is zero again after every query and dot is cleared
    before the next - and index_scores holds the LAST query's values until then"""
    ref = _build_q(ictx, qindex)
    A, B = qindex[20], np.concatenate([qindex[30], qindex[31], [63, 63]]).astype(np.int32)
    a1 = ictx.query_index(A, 10)
    s1 = ictx.index_scores()
    _check_query(ictx, ref, B, 10, "B")
    a2 = ictx.query_index(A, 10)
    s2 = ictx.index_scores()
    assert a1[0].tobytes() == a2[0].tobytes() and a1[1].tobytes() == a2[1].tobytes()
    assert s1[0].tobytes() == s2[0].tobytes() and s1[1].tobytes() == s2[1].tobytes() and s1[2] == s2[2]
    _check_query(ictx, ref, A, 10, "A again")


@pytest.mark.gpu
@pytest.mark.parametrize("N", [1025, 2049])
def test_top_1024_of_more_images(ictx, N):
    """top = 1024 with N = 1025 and 2049 (one and two strides of the selecting block, and one image beyond): many equal scores - the
    images repeat with period 300, hundreds score 0 - so the cut falls inside a run of ties"""
    rng = np.random.RandomState(N)
    base = [rng.randint(0, 200, rng.randint(1, 12)).astype(np.int32) for _ in range(300)]
    images = [base[i % 300] if i % 7 else np.zeros(0, np.int32) for i in range(N)]
    ref = _check_build(ictx, images, 200, "N = %d" % N)
    for q in (base[5], np.concatenate([base[8], base[9], base[10]]), np.array([199], np.int32)):
        for top in (1024, 1000, 1):
            im, sc = _check_query(ictx, ref, q, top, "N = %d, top = %d" % (N, top))
            assert (np.diff(sc) <= 0).all()


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def e2e(ictx):
    """the five golden images detected with a vocabulary of 40 rows set: keys, (word, dist2) rows, and the reference index on them"""
    vocab = V.family("uniform", 40, seed=71)
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    plain = ictx.detect_batch(imgs)
    ictx.set_vocabulary(vocab)
    try:
        res = ictx.detect_batch(imgs)
        words = [ictx.words(i) for i in range(len(imgs))]
    finally:
        ictx.set_vocabulary(None)
    assert [len(k) for _, k in res] == E2E_KEYS and [len(w) for w in words] == E2E_KEYS
    ref = R.build([w[:, 0] for w in words], 40)
    for a in ref[1:]:
        a.setflags(write=False)
    return imgs, plain, res, words, vocab, ref


def _check_e2e_ranking(im, sc):
    assert im[:2].tolist() == [0, 2] and sc[0] == sc[1] > 0.0   # the two band_160x120 tie at the top, in that order
    assert sc[im.tolist().index(3)] == 0.0                      # the keyless image


@pytest.mark.gpu
def test_end_to_end_from_the_words_of_images(ictx, e2e):
    imgs, plain, res, words, vocab, ref = e2e
    ictx.build_index(words, 40)
    _check_tables(ictx, ref, words, 40, "words(i)")
    im, sc = _check_query(ictx, ref, words[0], 5, "words of image 0")
    _check_e2e_ranking(im, sc)
    assert ictx.vocabulary_size == 0   # the index needs no vocabulary in the context


@pytest.mark.gpu
def test_end_to_end_device_resident_words_in_place(e2e):
    """detect_batch_device with a vocabulary leaves (word, dist2) rows on the device; the index is built from them where they are,
    and queried with the first image's rows in place: three copies of one image tie in index order"""
    import torch
    imgs, plain, res, words, vocab, _ = e2e
    img = imgs[0]
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_vocabulary(vocab)
        t = torch.from_numpy(np.stack([img] * 3)).cuda()
        torch.cuda.synchronize()
        ch, cd, dkeys, total = c.detect_batch_device(t.data_ptr(), 3, img.shape[1], img.shape[0])
        assert total == 663 and list(cd) == [221] * 3
        ptr, rows = c.words_device()
        assert rows == 663
        c.build_index_device(ptr, cd, 2, 40)
        ref = R.build([words[0][:, 0]] * 3, 40)
        _check_tables(c, ref, [words[0]] * 3, 40, "device-resident words")
        im, sc = c.query_index_device(ptr, 221, 2, 3)
        want = R.query(ref, words[0][:, 0], 3)
        assert im.tolist() == [0, 1, 2] == want[0].tolist() and np.array_equal(_bits(sc), _bits(want[1]))
        # detection with an index present: the keys do not change by a bit, and the index still answers
        ch2, cd2, dkeys2, total2 = c.detect_batch_device(t.data_ptr(), 3, img.shape[1], img.shape[0])
        from tests.test_gpu_parity import _device_keys
        assert total2 == 663 and _device_keys(dkeys2, total2)[:221].tobytes() == res[0][1].tobytes()
        im2, sc2 = c.query_index(words[0], 3)
        assert im2.tolist() == [0, 1, 2] and sc2.tobytes() == sc.tobytes()


@pytest.mark.gpu
def test_end_to_end_cli_search(ictx, e2e, tmp_path):
    """<image>.hesaff.words files of the five images, hesaff --search over them with the first as the query: rank, path and score
    (%.17g reads back to the same double) are the reference's; a file of another vocabulary size ends the run, named"""
    imgs, plain, res, words, vocab, ref = e2e
    paths = []
    for j, ((_, keys), w) in enumerate(zip(res, words)):
        paths.append(str(tmp_path / ("%d_%s.pgm.hesaff.words" % (j, E2E_IMAGES[j]))))
        hesaff_amd.write_words(paths[-1], keys, w, ictx.params.mrSize, 40)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    for top in (5, 2):
        r = subprocess.run([EXE, "--search", str(lst), "--query", paths[0], "--top", str(top)], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        want_im, want_sc = R.query(ref, words[0][:, 0], top)[:2]
        lines = [l.split("\t") for l in r.stdout.strip().split("\n")]
        assert [int(l[0]) for l in lines] == list(range(1, top + 1))
        assert [l[1] for l in lines] == [paths[i] for i in want_im]
        assert np.array_equal(_bits(np.array([float(l[2]) for l in lines])), _bits(want_sc))
        assert all(l[2] == "%.17g" % s for l, s in zip(lines, want_sc))
    other = str(tmp_path / "other.hesaff.words")
    hesaff_amd.write_words(other, res[1][1], words[1], ictx.params.mrSize, 41)
    lst.write_text("\n".join(paths + [other]) + "\n")
    r = subprocess.run([EXE, "--search", str(lst), "--query", paths[0]], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stdout == "" and other in r.stderr


@pytest.mark.gpu
def test_end_to_end_cpp_members(e2e, tmp_path):
    """tests/native/index_search_keys.cpp: buildIndex, queryIndex and clearIndex through hesaff.hpp hold what the Python path holds"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, plain, res, words, vocab, ref = e2e
    exe = str(tmp_path / "index_search_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "index_search_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    r = subprocess.run([exe, vfile, "4"] + [os.path.join(GOLD, n + ".pgm") for n in E2E_IMAGES], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want_im, want_sc = R.query(ref, words[0][:, 0], 4)[:2]
    assert r.stdout.strip().split("\n") == ["R %d %d %.17g" % (j + 1, i, s) for j, (i, s) in enumerate(zip(want_im, want_sc))] + ["C refused"]


# ---------------------------------------------------------------- refusals and isolation

@pytest.mark.gpu
def test_refusals_leave_the_context_its_index_and_its_vocabulary_alone(e2e):
    import torch
    imgs, plain, res, words, vocab, ref = e2e
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        L, h = c.L, c.h
        images = np.full(8, 7, np.int32); scores = np.full(8, 7.0); n = ctypes.c_int(7)
        ip, sp, np_ = images.ctypes.data, scores.ctypes.data, ctypes.byref(n)
        q = np.array([1, 2, 3], np.int32)
        # no index: queries, getters and the info are refused, clearing succeeds, nothing is written
        ni = ctypes.c_int(7)
        assert L.hesaff_index_query(h, 3, q.ctypes.data, 1, 4, ip, sp, np_) == ARG
        assert L.hesaff_index_get_scores(h, None, sp, None) == ARG and L.hesaff_index_get_tables(h, ip, None, None) == ARG
        assert L.hesaff_index_get_info(h, ctypes.byref(ni), None, None, None) == ARG and ni.value == 7
        assert L.hesaff_index_clear(h) == 0 and c.index_info is None
        with pytest.raises(hesaff_amd.HesaffError):
            c.index_scores()
        c.set_vocabulary(vocab)
        c.build_index(words, 40)

        def still_works(what):
            assert c.vocabulary_size == 40, what
            (nh, keys), = c.detect_batch(imgs[1:2])
            assert keys.tobytes() == res[1][1].tobytes() and np.array_equal(c.words(0), words[1]), what
            _check_tables(c, ref, words, 40, what)
            im, sc = _check_query(c, ref, words[0], 5, what)
            _check_e2e_ranking(im, sc)
        still_works("before")
        counts = np.array([2, 0, 1], np.int32); w3 = np.array([0, 1, 1], np.int32)
        t = torch.from_numpy(np.array([0, 1, 1, 0], np.int32)).cuda()
        torch.cuda.synchronize()
        dp = ctypes.c_void_p(t.data_ptr())
        cp, wp = counts.ctypes.data, w3.ctypes.data
        build, build_d, query, query_d = L.hesaff_index_build, L.hesaff_index_build_device, L.hesaff_index_query, L.hesaff_index_query_device
        # required pointers
        assert build(h, 3, None, wp, 1, 2) == ARG and build(h, 3, cp, None, 1, 2) == ARG
        assert build_d(h, 3, None, dp, 1, 2) == ARG and build_d(h, 3, cp, None, 1, 2) == ARG
        # counts outside the bounds: images, vocabulary, the keys of an image, the keys in all
        for n_images, k in ((0, 2), (-1, 2), ((1 << 20) + 1, 2), (3, 0), (3, -1), (3, (1 << 20) + 1)):
            big = np.zeros(max(n_images, 3), np.int32)
            assert build(h, n_images, big.ctypes.data, wp, 1, k) == ARG and build_d(h, n_images, big.ctypes.data, dp, 1, k) == ARG, (n_images, k)
        for bad in ([2, -1, 1], [2, (1 << 18) + 1, 1]):
            b = np.array(bad, np.int32)
            assert build(h, 3, b.ctypes.data, wp, 1, 2) == ARG and build_d(h, 3, b.ctypes.data, dp, 1, 2) == ARG, bad
        too_many = np.full(1025, 1 << 18, np.int32)   # 2^28 + 2^18 keys: refused before a word is read
        assert build(h, 1025, too_many.ctypes.data, wp, 1, 2) == ARG and build_d(h, 1025, too_many.ctypes.data, dp, 1, 2) == ARG
        # word_stride, alignment
        for stride in (0, 3, -1):
            assert build(h, 3, cp, wp, stride, 2) == ARG and build_d(h, 3, cp, dp, stride, 2) == ARG
            assert query(h, 3, wp, stride, 4, ip, sp, np_) == ARG and query_d(h, 3, dp, stride, 4, ip, sp, np_) == ARG
        assert build_d(h, 3, cp, ctypes.c_void_p(t.data_ptr() + 2), 1, 2) == ARG and query_d(h, 3, ctypes.c_void_p(t.data_ptr() + 2), 1, 4, ip, sp, np_) == ARG
        # a word outside 0 .. K - 1: found on the host while staging, on the device by the check kernel
        for at, w in ((0, -1), (2, 2), (1, 1 << 30)):
            bad = w3.copy(); bad[at] = w
            td = torch.from_numpy(bad).cuda()
            torch.cuda.synchronize()
            assert build(h, 3, cp, bad.ctypes.data, 1, 2) == ARG and build_d(h, 3, cp, ctypes.c_void_p(td.data_ptr()), 1, 2) == ARG, (at, w)
        for w in (-1, 40, 1 << 30):
            bad = np.array([1, w, 2], np.int32)
            td = torch.from_numpy(bad).cuda()
            torch.cuda.synchronize()
            assert query(h, 3, bad.ctypes.data, 1, 4, ip, sp, np_) == ARG and query_d(h, 3, ctypes.c_void_p(td.data_ptr()), 1, 4, ip, sp, np_) == ARG, w
        still_works("after the refused builds")
        # queries: n, top, required pointers
        for nq, top in ((-1, 4), ((1 << 18) + 1, 4), (3, 0), (3, -1), (3, 1025)):
            assert query(h, nq, wp, 1, top, ip, sp, np_) == ARG and query_d(h, nq, dp, 1, top, ip, sp, np_) == ARG, (nq, top)
        assert query(h, 3, None, 1, 4, ip, sp, np_) == ARG and query(h, 3, wp, 1, 4, None, sp, np_) == ARG
        assert query(h, 3, wp, 1, 4, ip, None, np_) == ARG and query(h, 3, wp, 1, 4, ip, sp, None) == ARG
        assert query_d(h, 3, None, 1, 4, ip, sp, np_) == ARG and query_d(h, 3, dp, 1, 4, None, sp, np_) == ARG
        ms = ctypes.c_float(7)
        assert L.hesaff_get_index_ms(h, None, ctypes.byref(ms)) == ARG and L.hesaff_get_index_ms(h, ctypes.byref(ms), None) == ARG
        assert (images == 7).all() and (scores == 7.0).all() and n.value == 7 and ms.value == 7.0
        for bad in (np.zeros(3, np.int64), np.zeros((3, 3), np.int32)):
            with pytest.raises(ValueError):
                c.query_index(bad, 3)
            with pytest.raises(ValueError):
                c.build_index([bad], 40)
        still_works("after the refused queries")
        # clearing: the index is gone, the context and its vocabulary are not
        c.clear_index()
        assert c.index_info is None and query(h, 3, wp, 1, 4, ip, sp, np_) == ARG and c.vocabulary_size == 40
        (nh, keys), = c.detect_batch(imgs[1:2])
        assert keys.tobytes() == res[1][1].tobytes()
        c.clear_index()


@pytest.mark.gpu
def test_detection_is_untouched_by_an_index(ictx, e2e):
    """the keys of a detecting call with an index present are byte-equal to those without one, and the index survives the call"""
    imgs, plain, res, words, vocab, ref = e2e
    ictx.clear_index()
    without = ictx.detect_batch(imgs)
    ictx.build_index(words, 40)
    with_index = ictx.detect_batch(imgs)
    for (na, a), (nb, b), (np_, p) in zip(without, with_index, plain):
        assert na == nb == np_ and a.tobytes() == b.tobytes() == p.tobytes()
    _check_tables(ictx, ref, words, 40, "after detection")
    _check_e2e_ranking(*_check_query(ictx, ref, words[0], 5, "after detection"))


@pytest.mark.gpu
def test_index_ms_are_event_times(ictx, qindex):
    ictx.set_profiling(1)
    try:
        ictx.build_index(qindex, 64)
        ictx.query_index(qindex[5], 10)
        ms = ictx.index_ms
        print("index_ms (build, query) for 66 images, K = 64:", ms)
        assert all(0.0 < v < 1000.0 for v in ms)
    finally:
        ictx.set_profiling(0)
    ictx.build_index(qindex, 64)
    ictx.query_index(qindex[5], 10)
    assert ictx.index_ms == (0.0, 0.0)
