"""GPU suite of the growing, durable index (hesaff_index_add*, hesaff_index_get_postings, hesaff_index_save / hesaff_index_load,
include/hesaff_amd.h; kernels_index_grow.h).  The reference is the numpy definition on the CONCATENATED collection
(tests/index_growth_ref.py over tests/index_ref.py and tests/embedding_ref.py).  Every comparison is bit for bit: df, idf, norm2 and
the offsets as arrays, the posting and key lists as per-word sorted multisets, dot, nq2, the float64 scores as uint64 bit patterns
and the ranked images."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from tests import embedding_ref as E
from tests import index_growth_ref as G
from tests import index_ref as R
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
ARG, IO = -2, -4
SIZES = [0, 1, 63, 64, 65, 200]


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def gctx():
    with hesaff_amd.HesaffContext(_params(max_batch=4), device=0) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _i32(images):
    return [np.asarray(w, np.int32) for w in images]


def _sorted_lists(offsets, first, second):
    """(word, first, second) of every list entry, sorted: the lists as per-word multisets, whatever K"""
    word = np.repeat(np.arange(len(offsets) - 1), np.diff(offsets.astype(np.int64)))
    order = np.lexsort((second, first, word))
    return word[order], np.asarray(first)[order], np.asarray(second)[order]


def _want_postings(ref, k):
    word = np.concatenate([w for w, _ in ref[0]] + [np.zeros(0, np.int64)])
    image = np.concatenate([np.full(len(w), i, np.int64) for i, (w, _) in enumerate(ref[0])] + [np.zeros(0, np.int64)])
    tf = np.concatenate([c for _, c in ref[0]] + [np.zeros(0, np.int64)])
    order = np.lexsort((tf, image, word))
    return word[order], image[order], tf[order]


def _want_keys(images, sigs):
    word = np.concatenate([np.asarray(w, np.int64) for w in images] + [np.zeros(0, np.int64)])
    image = np.concatenate([np.full(len(w), i, np.int64) for i, w in enumerate(images)] + [np.zeros(0, np.int64)])
    sig = np.concatenate([np.asarray(g, np.uint64) for g in sigs] + [np.zeros(0, np.uint64)])
    order = np.lexsort((sig, image, word))
    return word[order], image[order], sig[order]


def _check_index(ctx, images, K, what, sigs=None, ref=None):
    """the context's index against the build of `images`: tables, offsets, lists"""
    ref = R.build(images, K) if ref is None else ref
    df, idf, norm2 = ctx.index_tables()
    assert np.array_equal(df, ref[1]), (what, "df")
    assert np.array_equal(idf, ref[2]), (what, "idf")
    assert np.array_equal(norm2, ref[3]), (what, "norm2", np.nonzero(norm2 != ref[3])[0][:8].tolist())
    assert ctx.index_info == (len(images), K, sum(len(w) for w in images), int(ref[1].sum())), (what, ctx.index_info)
    offsets, im, tf = ctx.index_postings()
    assert offsets.dtype == im.dtype == tf.dtype == np.uint32
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(ref[1].astype(np.int64))])), (what, "offsets")
    for got, want, name in zip(_sorted_lists(offsets, im, tf), _want_postings(ref, K), ("word", "image", "tf")):
        assert np.array_equal(got, want), (what, "postings", name)
    emb = ctx.index_embedded()
    assert (emb is None) == (sigs is None), (what, "embedded")
    if sigs is not None:
        counts = np.bincount(np.concatenate(_i32(images) + [np.zeros(0, np.int32)]), minlength=K)
        assert np.array_equal(emb[0], np.concatenate([[0], np.cumsum(counts)])), (what, "key offsets")
        for got, want, name in zip(_sorted_lists(*emb), _want_keys(images, sigs), ("word", "image", "sig")):
            assert np.array_equal(got, want), (what, "key lists", name)
    return ref


def _check_query(ctx, ref, images, q, top, what, sigs=None, qs=None, T=None):
    q = np.asarray(q, np.int32)
    if T is None:
        want = R.query(ref, q, top)
        im, sc = ctx.query_index(q, top)
    else:
        want = E.query(ref, images, sigs, q, qs, T, top)
        im, sc = ctx.query_index(q, top, signatures=qs, hamming=T)
    dot, score, nq2 = ctx.index_scores()
    assert nq2 == want[4], (what, "nq2")
    assert np.array_equal(dot, want[2]), (what, "dot")
    assert np.array_equal(_bits(score), _bits(want[3])), (what, "scores of every image")
    assert im.tolist() == want[0].tolist() and np.array_equal(_bits(sc), _bits(want[1])), (what, "ranking")


def _scores_are_zero(ctx, what):
    dot, score, nq2 = ctx.index_scores()
    assert not dot.any() and not score.any() and nq2 == 0, what


def _add_and_check(ctx, old, new, K, what, queries=(), old_sigs=None, new_sigs=None, T=(0, 24, 64)):
    """build(old), add(new), and everything against build(old + new)"""
    old, new = _i32(old), _i32(new)
    ctx.build_index(old, K, signatures=old_sigs)
    if queries:
        ctx.query_index(np.asarray(queries[0], np.int32), 3)   # (so that there IS a last query whose values the add has to clear)
    ctx.add_to_index(new, signatures=new_sigs)
    _scores_are_zero(ctx, what)
    images = old + new
    sigs = None if old_sigs is None else list(old_sigs) + list(new_sigs)
    ref = _check_index(ctx, images, K, what, sigs)
    for q in queries:
        q = np.asarray(q, np.int32)
        _check_query(ctx, ref, images, q, min(len(images), 1024), what + ", query of %d" % len(q))
        if sigs is not None:
            qs = _sig_for(q, 5)
            for t in T:
                _check_query(ctx, ref, images, q, 7, what + ", T = %d" % t, sigs, qs, t)
    return ref


def _sig_for(words, seed):
    """signatures in which keys of one word collide (two values per word) and differ in few bits"""
    rng = np.random.RandomState(seed + len(words))
    base = (np.asarray(words, np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0x5555)
    flip = np.where(rng.randint(0, 2, len(words)) == 1, np.uint64(0xFFFFFF), np.uint64(0))
    return (base ^ flip).astype(np.uint64)


def _random_images(n, K, seed, most=40):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, K, rng.randint(0, most + 1)).astype(np.int32) for _ in range(n)]


# ---------------------------------------------------------------- add against rebuild

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 33, 300])
def test_add_against_rebuild(gctx, K):
    """N = 1, m = 1; then 70 images and 37 more, plain and embedded, with queries of an old image, of a new one and of random words"""
    _add_and_check(gctx, [[0]], [[K - 1, K - 1]], K, "N = 1, m = 1", [[0], [K - 1]])
    old, new = _random_images(70, K, 1), _random_images(37, K, 2)
    rng = np.random.RandomState(K)
    queries = [old[3], new[5], rng.randint(0, K, 50)]
    _add_and_check(gctx, old, new, K, "70 + 37, K = %d" % K, queries)
    _add_and_check(gctx, old, new, K, "70 + 37 embedded, K = %d" % K, queries, [_sig_for(w, 1) for w in old], [_sig_for(w, 2) for w in new])


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("embedded", [False, True])
def test_add_forms_at_one_small_shape(gctx, embedded, device, stride):
    """hesaff_index_add[_embedded][_device] at word_stride 1 and 2 behind a build of 2 images over K = 5: an add of 3 images with
    the middle one empty, an add of images that hold no word at all, and the first or the last word at -1 or K, refused under the
    entry point's own name with the index left as it was.  Everything here is host plumbing and per-key device code with no tile
    size in it, so the shape is small."""
    import torch
    K = 5
    old = _i32([[1, 1, 4], [0]])
    new = _i32([[0, 3, 3, 4, 1, 0, 3], [], [4, 2]])
    rows = (lambda w: np.stack([w, np.full(len(w), -7, np.int32)], axis=1)) if stride == 2 else (lambda w: w)

    def add(ws, gs):
        if not device:
            gctx.add_to_index([rows(w) for w in ws], signatures=gs)
            return
        flat = np.concatenate([rows(w) for w in ws])
        tw = torch.from_numpy(np.ascontiguousarray(flat) if flat.size else np.zeros(2, np.int32)).cuda()
        ts = None if gs is None else torch.from_numpy(np.concatenate(list(gs) + [np.zeros(1, np.uint64)]).view(np.int64)).cuda()
        torch.cuda.synchronize()
        gctx.add_to_index_device(tw.data_ptr(), [len(w) for w in ws], stride, sigs_ptr=None if ts is None else ts.data_ptr())

    def sigs_of(ws, seed):
        return [_sig_for(w, seed) for w in ws] if embedded else None
    what = "embedded %s, device %s, stride %d" % (embedded, device, stride)
    old_sigs, new_sigs = sigs_of(old, 1), sigs_of(new, 2)
    gctx.build_index(old, K, signatures=old_sigs)
    none = [w[:0] for w in new]
    add(none, sigs_of(none, 3))
    images, sigs = old + none, old_sigs + sigs_of(none, 3) if embedded else None
    _check_index(gctx, images, K, what + ", an add of no word at all", sigs)
    add(new, new_sigs)
    images, sigs = images + new, sigs + new_sigs if embedded else None
    ref = _check_index(gctx, images, K, what, sigs)
    q = np.array([3, 0, 3, 4], np.int32)
    _check_query(gctx, ref, images, q, 8, what)
    if embedded:
        _check_query(gctx, ref, images, q, 8, what + ", T = 24", sigs, _sig_for(q, 5), 24)
    name = "hesaff_index_add%s%s" % ("_embedded" if embedded else "", "_device" if device else "")
    for at, w in ((0, -1), (0, K), (-1, -1), (-1, K)):
        bad = [a.copy() for a in new]
        bad[0 if at == 0 else 2][at] = w
        with pytest.raises(hesaff_amd.HesaffError, match=name + r": a word lies outside 0 \.\. vocabulary_size - 1$"):
            add(bad, new_sigs)
    _check_index(gctx, images, K, what + ", after the refusals", sigs, ref)


@pytest.mark.gpu
def test_embedded_add_equals_the_embedded_build_of_all_images(gctx):
    """an embedded build of 4 images and an embedded add of 2 against ONE embedded build of the 6, both on the device: the key lists
    (hesaff_index_get_embedded) and the postings (hesaff_index_get_postings) are equal as multisets per word, the offsets and the
    tables as arrays.  K = 9; word 7 is in no old image, word 2 in no new one, word 8 in none."""
    K = 9
    old = _i32([[0, 1, 1, 2, 6], [2, 2, 3], [], [4, 5, 0, 0, 2, 6]])
    new = _i32([[7, 7, 0, 1, 3], [4, 7, 5, 5, 6]])
    assert 7 not in np.concatenate(old) and 2 not in np.concatenate(new) and 8 not in np.concatenate(old + new)
    old_sigs, new_sigs = [_sig_for(w, 1) for w in old], [_sig_for(w, 2) for w in new]

    def lists():
        return [a.tobytes() for a in gctx.index_tables()] + [a.tobytes() for a in _sorted_lists(*gctx.index_postings())] + \
               [a.tobytes() for a in _sorted_lists(*gctx.index_embedded())] + [gctx.index_postings()[0].tobytes(), gctx.index_embedded()[0].tobytes()]
    gctx.build_index(old + new, K, signatures=old_sigs + new_sigs)
    whole, info = lists(), gctx.index_info
    gctx.build_index(old, K, signatures=old_sigs)
    gctx.add_to_index(new, signatures=new_sigs)
    assert lists() == whole and gctx.index_info == info
    _check_index(gctx, old + new, K, "4 + 2 images", old_sigs + new_sigs)


@pytest.mark.gpu
@pytest.mark.parametrize("K,most", [(1, 3), (33, 40), (300, 40), (5000, 12)])
def test_add_over_many_tiles(gctx, K, most):
    """2500 old images and 600 new ones: the merge runs over many tiles of 1024 positions - one list through all of them (K = 1), a few
    long lists per tile, and at K = 5000 hundreds of short lists and empty words inside every tile - plain and embedded"""
    old, new = _random_images(2500, K, 3, most), _random_images(600, K, 4, most)
    ref = _add_and_check(gctx, old, new, K, "many tiles, K = %d" % K, [old[7], new[9]])
    assert K == 1 or int(R.build(old, K)[1].sum()) > 8 * 1024
    gctx.build_index(old, K, signatures=[_sig_for(w, 1) for w in old])
    gctx.add_to_index(new, signatures=[_sig_for(w, 2) for w in new])
    _check_index(gctx, old + new, K, "many tiles embedded, K = %d" % K, [_sig_for(w, 1) for w in old] + [_sig_for(w, 2) for w in new], ref=ref)


@pytest.mark.gpu
def test_add_with_a_million_words(gctx):
    """K = 2^20 with a handful of keys in words 0 and K - 1 and in a few between: runs of half a million empty words in the old and
    the new offsets, and the cursors of every word written"""
    K = 1 << 20
    old = [[0, 0, K - 1], [], [K - 1, 5], [0]]
    new = [[K - 1], [0, 0, 0, K // 2], [], [K - 1, K - 2]]
    _add_and_check(gctx, old, new, K, "K = 2^20", [[0, K - 1], [K // 2, K - 2, 5], [17]])
    _add_and_check(gctx, old, new, K, "K = 2^20 embedded", [[0, K - 1]], [_sig_for(np.asarray(w, np.int32), 1) for w in old], [_sig_for(np.asarray(w, np.int32), 2) for w in new],
                   T=(0, 64))


def _lists_of_sizes(sizes, first_word, step, n_images, seed):
    """images in which word first_word + j * step is held by sizes[j] distinct images (a posting list of that length)"""
    rng = np.random.RandomState(seed)
    images = [[] for _ in range(n_images)]
    for j, m in enumerate(sizes):
        for i in rng.permutation(n_images)[:m]:
            images[i] += [first_word + j * step] * int(rng.randint(1, 4))
    return [np.array(rng.permutation(w), np.int32) for w in images]


@pytest.mark.gpu
def test_add_list_lengths_and_runs_of_empty_words(gctx):
    """old and new lists of 0, 1, 63, 64, 65 and 200 postings in every combination (old size j against new size (j + s) % 6 for three
    shifts s), the used words 7 apart from word 40 of K = 300: empty runs before, between and behind them in both offset tables"""
    K = 300
    for shift in (0, 1, 3):
        old = _lists_of_sizes(SIZES, 40, 7, 200, 10 + shift)
        new = _lists_of_sizes(SIZES[shift:] + SIZES[:shift], 40, 7, 200, 20 + shift)
        ref = _add_and_check(gctx, old, new, K, "shift %d" % shift, [old[0], new[1], [40 + 7 * 5, 47]])
        assert ref[1][40:40 + 7 * 6:7].tolist() == [a + b for a, b in zip(SIZES, SIZES[shift:] + SIZES[:shift])]
        assert not ref[1][:40].any() and not ref[1][76:].any()
    # a new word inside an old empty run and an old word the add does not touch
    _add_and_check(gctx, [[10, 290], [290]], [[150], [150, 11]], K, "new words between old ones", [[150, 290], [10, 11]])
    old = _lists_of_sizes(SIZES, 40, 7, 200, 31)
    new = _lists_of_sizes(SIZES[::-1], 40, 7, 200, 32)
    _add_and_check(gctx, old, new, K, "embedded list lengths", [old[0], new[1]], [_sig_for(w, 3) for w in old], [_sig_for(w, 4) for w in new])


@pytest.mark.gpu
def test_add_images_without_keys_and_single_words(gctx):
    K = 33
    old = _random_images(9, K, 5)
    old[4] = np.zeros(0, np.int32)                                            # an old image with no keys
    new = [np.zeros(0, np.int32), np.full(500, 17, np.int32), np.zeros(0, np.int32)]   # new images with no keys; all new keys in one word, tf = 500
    ref = _add_and_check(gctx, old, new, K, "keyless images, one word", [old[0], new[1], [17]])
    assert ref[0][10][1].tolist() == [500] and ref[3][4] == 0 and ref[3][9] == 0
    # tf > 1 throughout: new images that repeat few words many times
    rng = np.random.RandomState(6)
    new = [np.repeat(rng.randint(0, K, 3), rng.randint(2, 90, 3)).astype(np.int32) for _ in range(5)]
    _add_and_check(gctx, old, new, K, "tf > 1", [new[0], old[1]])
    # m images with no keys at all: only N changes, yet every idf and every norm does
    before = R.build(old, K)
    ref = _add_and_check(gctx, old, [[], [], []], K, "only N changes", [old[0], old[2]])
    assert np.array_equal(ref[1], before[1]) and (ref[2][ref[1] > 0] > before[2][ref[1] > 0]).all() and (ref[3][:9][before[3] > 0] > before[3][before[3] > 0]).all()


@pytest.mark.gpu
def test_add_moves_an_idf_to_zero_and_back(gctx):
    """word 3 in two of three images, the add brings its df to N + m: idf 0, the old norms shrink; word 5 in every old image (idf 0)
    and in none of the new ones: rare again, the old norms grow"""
    K = 8
    old = [[3, 5], [3, 3, 5], [5, 1]]
    ref0 = R.build(_i32(old), K)
    assert ref0[2][5] == 0 and ref0[2][3] > 0
    ref = _add_and_check(gctx, old, [[3, 1]], K, "df reaches N + m", [[3], [3, 1], [5]])
    assert ref[1][3] == 3 and ref[2][3] > 0                                  # (image 2 does not hold word 3)
    ref = _add_and_check(gctx, old, [[3, 1]], K, "df reaches N + m")
    full = _add_and_check(gctx, [[3, 5], [3, 3, 5]], [[3, 3, 3]], K, "idf falls to 0", [[3], [3, 5]])
    assert full[2][3] == 0 and full[2][5] > 0 and full[3][2] == 0
    before = R.build(_i32([[3, 5], [3, 3, 5]]), K)
    assert before[2][3] == 0 and before[2][5] == 0 and not before[3].any() and full[3][0] > 0   # the old norms come back from zero
    rare = _add_and_check(gctx, old, [[1], [2], [1, 2]], K, "an idf-0 word is rare again", [[5], [5, 3]])
    assert rare[2][5] > 0 and (rare[3][:2] > ref0[3][:2]).all()   # (images 0 and 1 hold word 5 and word 3, whose idf grows too)


@pytest.mark.gpu
def test_add_up_to_the_largest_index(gctx):
    """N + m = 2^20 exactly, almost all images without keys; one image more is refused.  The expected tables are the definition
    written out for the few images that hold keys (index_ref.build over a million images is a million numpy calls)"""
    N, K = 1 << 20, 33
    holders = {0: [1, 2, 2], 70000: [2, 30], N - 3: [30, 30, 30, 7], N - 2: [7, 1], N - 1: [32]}
    counts = np.zeros(N, np.int32)
    for i, w in holders.items():
        counts[i] = len(w)
    flat = np.array([w for i in sorted(holders) for w in holders[i]], np.int32)
    cut = N - 2                                                              # the last two images are added
    n_old = int(counts[:cut].sum())
    L, h = gctx.L, gctx.h
    assert L.hesaff_index_build(h, cut, counts.ctypes.data, flat.ctypes.data, 1, K) == 0
    assert L.hesaff_index_add(h, 2, counts[cut:].ctypes.data, flat[n_old:].ctypes.data, 1) == 0
    assert gctx.index_info == (N, K, len(flat), 9)
    df = np.zeros(K, np.uint32)
    for w in holders.values():
        df[np.unique(w)] += 1
    idf = np.array([R.ilog2_q8(N, int(d)) if d else 0 for d in df], np.uint64)
    norm2 = np.zeros(N, np.uint64)
    for i, w in holders.items():
        u, c = np.unique(w, return_counts=True)
        norm2[i] = ((c.astype(np.uint64) * idf[u]) ** 2).sum(dtype=np.uint64)
    got = gctx.index_tables()
    assert np.array_equal(got[0], df) and np.array_equal(got[1], idf.astype(np.uint32)) and np.array_equal(got[2], norm2)
    offsets, im, tf = gctx.index_postings()
    _, gi, gt = _sorted_lists(offsets, im, tf)
    assert list(zip(gi.tolist(), gt.tolist())) == [(0, 1), (N - 2, 1), (0, 2), (70000, 1), (N - 3, 1), (N - 2, 1), (70000, 1), (N - 3, 3), (N - 1, 1)]
    im, sc = gctx.query_index(np.array([32], np.int32), 2)
    assert im.tolist() == [N - 1, 0] and sc[0] == 1.0 and sc[1] == 0.0
    state = [a.tobytes() for a in gctx.index_tables()]
    one = np.zeros(1, np.int32)
    assert L.hesaff_index_add(h, 1, one.ctypes.data, None, 1) == ARG         # N + m = 2^20 + 1
    assert [a.tobytes() for a in gctx.index_tables()] == state and gctx.index_info[0] == N


@pytest.mark.gpu
def test_adds_in_a_row_and_in_one(gctx):
    """three adds in a row against one build; an add of (A, B) against the adds of A then B: the same index, lists as multisets"""
    K = 300
    parts = [_random_images(n, K, 40 + n) for n in (20, 1, 13, 30)]
    sig_parts = [[_sig_for(w, i) for w in p] for i, p in enumerate(parts)]
    for sigs in (None, sig_parts):
        gctx.build_index(parts[0], K, signatures=None if sigs is None else sigs[0])
        for j in (1, 2, 3):
            gctx.add_to_index(parts[j], signatures=None if sigs is None else sigs[j])
        images = sum(parts, [])
        all_sigs = None if sigs is None else sum(sigs, [])
        ref = _check_index(gctx, images, K, "three adds", all_sigs)
        _check_query(gctx, ref, images, parts[3][2], 10, "three adds")
        lists_stepwise = _sorted_lists(*gctx.index_postings())
        gctx.build_index(parts[0], K, signatures=None if sigs is None else sigs[0])
        gctx.add_to_index(parts[1] + parts[2] + parts[3], signatures=None if sigs is None else sigs[1] + sigs[2] + sigs[3])
        _check_index(gctx, images, K, "one add of all", all_sigs, ref=ref)
        assert all(np.array_equal(a, b) for a, b in zip(lists_stepwise, _sorted_lists(*gctx.index_postings())))


@pytest.mark.gpu
def test_add_host_and_device_forms_and_strides(gctx):
    """the host form against the device form, (word, dist2) rows against bare words, plain and embedded: one index"""
    import torch
    K = 300
    old, new = _random_images(30, K, 50), _random_images(11, K, 51)
    old_s, new_s = [_sig_for(w, 1) for w in old], [_sig_for(w, 2) for w in new]
    images = old + new
    ref = R.build(images, K)
    rows = [np.stack([w, np.full(len(w), -7, np.int32)], axis=1) if len(w) else np.zeros((0, 2), np.int32) for w in new]
    counts = [len(w) for w in new]
    for embedded in (False, True):
        sigs = old_s + new_s if embedded else None
        gctx.build_index(old, K, signatures=old_s if embedded else None)
        gctx.add_to_index(rows, signatures=new_s if embedded else None)
        _check_index(gctx, images, K, "host rows", sigs, ref=ref)
        ts = torch.from_numpy(np.concatenate(new_s).view(np.int64)).cuda()
        for stride, flat in ((1, np.concatenate(new)), (2, np.concatenate(rows))):
            t = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
            torch.cuda.synchronize()
            gctx.build_index(old, K, signatures=old_s if embedded else None)
            gctx.add_to_index_device(t.data_ptr(), counts, stride, ts.data_ptr() if embedded else None)
            assert np.array_equal(t.cpu().numpy(), flat)   # the source is only read
            _check_index(gctx, images, K, "device, stride %d" % stride, sigs, ref=ref)
        _check_query(gctx, ref, images, new[3], 9, "after the device add")
        if embedded:
            _check_query(gctx, ref, images, new[3], 9, "after the device add, T = 24", sigs, new_s[3], 24)


@pytest.mark.gpu
def test_growth_ms_are_event_times(gctx):
    old, new = _random_images(30, 33, 60), _random_images(5, 33, 61)
    gctx.set_profiling(1)
    try:
        gctx.build_index(old, 33)
        gctx.add_to_index(new)
        ms = gctx.index_growth_ms
        print("index_growth_ms (insert, tables, merge, scatter, load):", ms)
        assert all(0.0 < v < 1000.0 for v in ms[:4])
    finally:
        gctx.set_profiling(0)
    gctx.build_index(old, 33)
    gctx.add_to_index(new)
    assert gctx.index_growth_ms[:4] == (0.0, 0.0, 0.0, 0.0)


# ---------------------------------------------------------------- save and load

@pytest.fixture(scope="module")
def saved(gctx, tmp_path_factory):
    """a plain and an embedded index of 40 images over K = 33, saved by the module's context"""
    d = tmp_path_factory.mktemp("index_files")
    K = 33
    images = _random_images(40, K, 70)
    images[7] = np.zeros(0, np.int32)
    sigs = [_sig_for(w, 7) for w in images]
    ref = R.build(images, K)
    paths = {}
    for name, s in (("plain", None), ("embedded", sigs)):
        gctx.build_index(images, K, signatures=s)
        paths[name] = str(d / (name + ".index"))
        gctx.save_index(paths[name])
    return K, images, sigs, ref, paths


@pytest.mark.gpu
def test_save_and_load_in_a_fresh_context(gctx, saved):
    K, images, sigs, ref, paths = saved
    more = _random_images(6, K, 71)
    more_s = [_sig_for(w, 8) for w in more]
    for name in ("plain", "embedded"):
        s = sigs if name == "embedded" else None
        f = hesaff_amd.read_index_file(paths[name])
        assert (f["embedded"], f["k"], f["n_images"], f["n_keys"], f["n_postings"]) == (s is not None, K, 40, sum(len(w) for w in images), int(ref[1].sum()))
        assert np.array_equal(f["df"], ref[1]) and f["postings"][:, 0].max() < 40
        with hesaff_amd.HesaffContext(device=0) as c:
            assert c.index_info is None
            c.load_index(paths[name])
            _scores_are_zero(c, "after a load")
            _check_index(c, images, K, "loaded " + name, s, ref=ref)
            for q in (images[3], images[20], [5, 5, 9]):
                _check_query(c, ref, images, q, 40, "loaded " + name)
                if s is not None:
                    for T in (0, 24, 64):
                        _check_query(c, ref, images, q, 7, "loaded, T = %d" % T, s, _sig_for(np.asarray(q, np.int32), 7), T)
            # a plain query on a loaded embedded index is the plain index's (above); an add after a load against a rebuild
            c.add_to_index(more, signatures=more_s if s is not None else None)
            ref2 = _check_index(c, images + more, K, "add after load", None if s is None else s + more_s)
            _check_query(c, ref2, images + more, more[2], 46, "add after load")
            # a save of the loaded and grown index loads again to the same
            again = paths[name] + ".again"
            c.save_index(again)
            gctx.load_index(again)
            _check_index(gctx, images + more, K, "saved again", None if s is None else s + more_s, ref=ref2)


@pytest.mark.gpu
def test_load_replaces_an_existing_index(gctx, saved):
    K, images, sigs, ref, paths = saved
    gctx.build_index(_i32([[0, 1], [1]]), 2)
    gctx.query_index(np.array([1], np.int32), 2)
    gctx.load_index(paths["embedded"])
    _scores_are_zero(gctx, "a load clears the last query")
    _check_index(gctx, images, K, "load over a plain index", sigs, ref=ref)
    gctx.load_index(paths["plain"])
    _check_index(gctx, images, K, "load over an embedded index", None, ref=ref)
    gctx.set_profiling(1)
    try:
        gctx.load_index(paths["embedded"])
        assert 0.0 < gctx.index_growth_ms[4] < 1000.0
    finally:
        gctx.set_profiling(0)


@pytest.mark.gpu
def test_load_an_index_without_postings(gctx, tmp_path):
    gctx.build_index(_i32([[], [], []]), 33)
    p = str(tmp_path / "empty.index")
    gctx.save_index(p)
    assert os.path.getsize(p) == 40 + 136
    gctx.build_index(_i32([[1]]), 2)
    gctx.load_index(p)
    _check_index(gctx, [np.zeros(0, np.int32)] * 3, 33, "no postings")
    gctx.add_to_index(_i32([[4, 4], []]))
    _check_index(gctx, _i32([[], [], [], [4, 4], []]), 33, "grown from nothing")


@pytest.mark.gpu
def test_device_side_load_refusals(gctx, saved, tmp_path):
    """each file differs from a valid one in one field; the previous index answers as before after every refusal"""
    K, images, sigs, ref, paths = saved
    n_images, n_keys, df, post, kc, ki, ks = G.file_arrays(images, K, sigs)
    p = str(tmp_path / "valid.index")
    hesaff_amd.write_index_file(p, n_images, n_keys, df, post, kc, ki, ks)
    gctx.load_index(p)
    _check_index(gctx, images, K, "the valid file", sigs, ref=ref)
    previous = [np.array([0, 1, 1], np.int32), np.array([1], np.int32), np.array([0], np.int32)]
    gctx.build_index(previous, 2)
    pref = R.build(previous, 2)
    owner = int(np.argmax([len(w) for w in images]))            # the image with the most keys
    rows = np.nonzero(post[:, 0] == owner)[0]
    room = (1 << 18) - len(images[owner])
    assert post[rows[0], 1] + room + 1 <= 1 << 18 and len(rows) >= 2
    cases = []

    def case(name, rule, post_=post, n_keys_=n_keys, kc_=kc, ki_=ki, plain=False):
        cases.append((name, rule, (n_images, n_keys_, df, post_) + (() if plain else (kc_, ki_, ks))))
    bad = post.copy(); bad[5, 0] = n_images
    case("image", "image is not below n_images", bad, plain=True)
    bad = post.copy(); bad[5, 0] = 0xffffffff
    case("image_huge", "image is not below n_images", bad, plain=True)
    bad = post.copy(); n0 = n_keys - int(bad[9, 1]); bad[9, 1] = 0
    case("tf_zero", "tf is outside", bad, n0, plain=True)
    bad = post.copy(); bad[9, 1] = (1 << 18) + 1
    case("tf_big", "tf is outside", bad, plain=True)
    bad = post.copy(); bad[rows[0], 1] += room; bad[rows[1], 1] += 1   # two valid tf, one image's sum 2^18 + 1
    case("image_sum", "tf sum is above", bad, n_keys + room + 1, plain=True)
    case("total", "tf of all postings is not n_keys", post, n_keys + 1, plain=True)
    bad = post.copy(); bad[9, 1] += 1                                  # the same in an embedded file: n_keys is the key arrays' too
    case("total_embedded", "tf of all postings is not n_keys", bad)
    used = np.nonzero(kc)[0]
    bad = kc.copy(); bad[used[0]] += 1; bad[used[1]] -= 1              # the sum intact: only the device sees it
    case("key_count", "key count is not the tf", kc_=bad)
    bad = ki.copy(); bad[-1] = n_images
    case("key_image", "key's image is not below n_images", ki_=bad)
    for name, rule, arrays in cases:
        path = str(tmp_path / (name + ".index"))
        open(path, "wb").write(G.file_bytes(*arrays))
        assert hesaff_amd.read_index_file(path)["n_images"] == n_images, name      # the host reader finds nothing wrong
        with pytest.raises(hesaff_amd.HesaffError) as e:
            gctx.load_index(path)
        assert e.value.code == ARG and rule in str(e.value), (name, str(e.value))
        _check_index(gctx, previous, 2, "after the refused " + name, ref=pref)
        _check_query(gctx, pref, previous, [1, 0], 3, "after the refused " + name)
    # what the reader refuses is refused with its code, and a missing file too
    open(str(tmp_path / "torn.index"), "wb").write(G.file_bytes(n_images, n_keys, df, post)[:-8])
    for path in (str(tmp_path / "torn.index"), str(tmp_path / "none.index")):
        with pytest.raises(hesaff_amd.HesaffError) as e:
            gctx.load_index(path)
        assert e.value.code == IO
    _check_index(gctx, previous, 2, "after the torn file", ref=pref)
    gctx.clear_index()
    with pytest.raises(hesaff_amd.HesaffError):
        gctx.save_index(str(tmp_path / "never.index"))
    assert not os.path.exists(str(tmp_path / "never.index"))


# ---------------------------------------------------------------- refusals of the add

@pytest.mark.gpu
def test_add_refusals_leave_index_vocabulary_and_embedding_alone():
    import torch
    K = 33
    images = _random_images(12, K, 80)
    sigs = [_sig_for(w, 9) for w in images]
    vocab = V.family("uniform", K, seed=3)
    P = E.projection(5)
    tau = np.zeros((K, 64), np.int32)
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        L, h = c.L, c.h
        add, add_d, add_e, add_ed = L.hesaff_index_add, L.hesaff_index_add_device, L.hesaff_index_add_embedded, L.hesaff_index_add_embedded_device
        counts = np.array([2, 0, 1], np.int32); w3 = np.array([0, 1, 1], np.int32); s3 = np.array([1, 2, 3], np.uint64)
        t = torch.from_numpy(np.array([0, 1, 1, 0], np.int32)).cuda()
        ts = torch.from_numpy(np.array([1, 2, 3, 4], np.int64)).cuda()
        torch.cuda.synchronize()
        cp, wp, sp, dp, dsp = counts.ctypes.data, w3.ctypes.data, s3.ctypes.data, C.c_void_p(t.data_ptr()), C.c_void_p(ts.data_ptr())
        # no index
        assert add(h, 3, cp, wp, 1) == ARG and add_d(h, 3, cp, dp, 1) == ARG and add_e(h, 3, cp, wp, 1, sp) == ARG and add_ed(h, 3, cp, dp, 1, dsp) == ARG
        assert c.index_info is None
        with pytest.raises(hesaff_amd.HesaffError):
            c.index_postings()
        c.set_vocabulary(vocab)
        c.set_embedding(P, tau)
        for embedded in (False, True):
            c.build_index(images, K, signatures=sigs if embedded else None)

            def state():
                s = [a.tobytes() for a in c.index_tables()] + [a.tobytes() for a in c.index_postings()] + [repr(c.index_info)]
                if embedded:
                    s += [a.tobytes() for a in c.index_embedded()]
                gp, gt = c.embedding()
                return s + [gp.tobytes(), gt.tobytes(), repr(c.vocabulary_size)]
            before = state()
            if embedded:
                host = lambda m, cnt, w, stride, s=sp: add_e(h, m, cnt, w, stride, s)
                dev = lambda m, cnt, w, stride, s=dsp: add_ed(h, m, cnt, w, stride, s)
                # a plain add on an embedded index; a missing or misaligned signature pointer
                assert add(h, 3, cp, wp, 1) == ARG and add_d(h, 3, cp, dp, 1) == ARG
                assert add_e(h, 3, cp, wp, 1, None) == ARG and add_ed(h, 3, cp, dp, 1, None) == ARG
                assert add_ed(h, 3, cp, dp, 1, C.c_void_p(ts.data_ptr() + 4)) == ARG
            else:
                host = lambda m, cnt, w, stride: add(h, m, cnt, w, stride)
                dev = lambda m, cnt, w, stride: add_d(h, m, cnt, w, stride)
                # an embedded add on a plain index
                assert add_e(h, 3, cp, wp, 1, sp) == ARG and add_ed(h, 3, cp, dp, 1, dsp) == ARG
            # m < 1, N + m > 2^20
            big = np.zeros(1 << 20, np.int32)
            for m in (0, -1, (1 << 20) - 11, 1 << 20, (1 << 20) + 1):
                assert host(m, big.ctypes.data, wp, 1) == ARG and dev(m, big.ctypes.data, dp, 1) == ARG, m
            # a count outside 0 .. 2^18
            for bad in ([2, -1, 1], [2, (1 << 18) + 1, 1]):
                b = np.array(bad, np.int32)
                assert host(3, b.ctypes.data, wp, 1) == ARG and dev(3, b.ctypes.data, dp, 1) == ARG, bad
            # n_keys + new keys > 2^28: refused before a word is read
            too_many = np.full(1024, 1 << 18, np.int32)
            assert host(1024, too_many.ctypes.data, wp, 1) == ARG and dev(1024, too_many.ctypes.data, dp, 1) == ARG
            # the stride, required pointers, alignment
            for stride in (0, 3, -1):
                assert host(3, cp, wp, stride) == ARG and dev(3, cp, dp, stride) == ARG
            assert host(3, None, wp, 1) == ARG and host(3, cp, None, 1) == ARG and dev(3, None, dp, 1) == ARG and dev(3, cp, None, 1) == ARG
            assert dev(3, cp, C.c_void_p(t.data_ptr() + 2), 1) == ARG
            # a word outside 0 .. K - 1: on the host while staging, on the device by the check kernel, before anything is built
            for at, w in ((0, -1), (2, K), (1, 1 << 30)):
                bad = w3.copy(); bad[at] = w
                td = torch.from_numpy(bad).cuda()
                torch.cuda.synchronize()
                assert host(3, cp, bad.ctypes.data, 1) == ARG and dev(3, cp, C.c_void_p(td.data_ptr()), 1) == ARG, (at, w)
            assert "a word lies outside" in c.last_error() if hasattr(c, "last_error") else True
            assert state() == before, "embedded" if embedded else "plain"
            # and the context works: the same add, now well-formed
            c.add_to_index([w3[:2], w3[:0], w3[2:]], signatures=[s3[:2], s3[:0], s3[2:]] if embedded else None)
            _check_index(c, images + [w3[:2], w3[:0], w3[2:]], K, "after the refusals", sigs + [s3[:2], s3[:0], s3[2:]] if embedded else None)
        out = np.full(8, 7, np.uint32)
        c.clear_index()
        assert L.hesaff_index_get_postings(h, out.ctypes.data, None, None) == ARG and (out == 7).all()
        ms = [C.c_float(7) for _ in range(5)]
        assert L.hesaff_get_index_growth_ms(h, None, *[C.byref(x) for x in ms[1:]]) == ARG and all(x.value == 7.0 for x in ms)


# ---------------------------------------------------------------- end to end on the golden images

E2E_IMAGES = ["band_160x120", "band_96x96", "tiny_20x15", "band_131x77"]


@pytest.fixture(scope="module")
def e2e(gctx):
    """the three band images and the keyless tiny one detected with a vocabulary of 40 rows and an embedding: keys, (word, dist2)
    rows, signatures.  The index holds the first three (two band images and the tiny one); the third band image is the one added"""
    vocab = V.family("uniform", 40, seed=71)
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    gctx.set_vocabulary(vocab)
    gctx.set_embedding(E.projection(11), np.zeros((40, 64), np.int32))
    try:
        res = gctx.detect_batch(imgs)
        words = [gctx.words(i) for i in range(len(imgs))]
        sigs = [gctx.signatures(i).copy() for i in range(len(imgs))]
    finally:
        gctx.set_vocabulary(None)
    assert [len(w) for w in words][:3] == [221, 74, 0] and len(words[3]) > 0
    bare = [w[:, 0] for w in words]
    ref = R.build(bare, 40)
    return imgs, res, words, bare, sigs, vocab, ref


@pytest.mark.gpu
def test_end_to_end_the_fourth_image_added(gctx, e2e):
    imgs, res, words, bare, sigs, vocab, ref = e2e
    for s in (None, sigs):
        gctx.build_index(words[:3], 40, signatures=None if s is None else s[:3])
        gctx.add_to_index(words[3:], signatures=None if s is None else s[3:])
        _check_index(gctx, bare, 40, "three images and the fourth", s, ref=ref)
        for q in (0, 3):
            _check_query(gctx, ref, bare, bare[q], 4, "words of image %d" % q)
            if s is not None:
                _check_query(gctx, ref, bare, bare[q], 4, "words of image %d, T = 24" % q, s, s[q], 24)
    im, sc = gctx.query_index(words[3], 4)
    assert im[0] == 3 and abs(sc[0] - 1.0) < 1e-15 and sc[im.tolist().index(2)] == 0.0


@pytest.mark.gpu
def test_end_to_end_cli(gctx, e2e, tmp_path):
    """--search --save-index over three words files, --index --add of the fourth, --index --query: the ranking printed equals
    --search's over the full list line for line, plain, with --hamming and with --verify; the pair of files is rewritten whole"""
    imgs, res, words, bare, sigs, vocab, ref = e2e
    paths = []
    for j, ((_, keys), w, g) in enumerate(zip(res, words, sigs)):
        paths.append(str(tmp_path / ("%d_%s.pgm.hesaff.words" % (j, E2E_IMAGES[j]))))
        hesaff_amd.write_words(paths[-1], keys, w, gctx.params.mrSize, 40)
        hesaff_amd.write_signatures(paths[-1][:-len(".words")] + ".sigs", g)
    full, three, more = tmp_path / "full.txt", tmp_path / "three.txt", tmp_path / "more.txt"
    full.write_text("\n".join(paths) + "\n"); three.write_text("\n".join(paths[:3]) + "\n"); more.write_text(paths[3] + "\n")

    def run(*args):
        r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (args, r.stderr)
        return r.stdout
    for hamming in ((), ("--hamming", "24")):
        idx = str(tmp_path / ("idx%d.bin" % len(hamming)))
        assert run("--search", three, "--save-index", idx, *hamming) == ""
        assert open(idx + ".list").read() == "\n".join(paths[:3]) + "\n"
        f = hesaff_amd.read_index_file(idx)
        assert (f["n_images"], f["k"], f["embedded"]) == (3, 40, bool(hamming))
        assert run("--index", idx, "--add", more) == ""
        assert open(idx + ".list").read() == "\n".join(paths) + "\n"
        f = hesaff_amd.read_index_file(idx)
        assert (f["n_images"], f["n_keys"], f["embedded"]) == (4, sum(len(w) for w in words), bool(hamming)) and np.array_equal(f["df"], ref[1])
        assert sorted(os.listdir(str(tmp_path))).count(os.path.basename(idx)) == 1 and not [n for n in os.listdir(str(tmp_path)) if ".part" in n or ".new" in n]
        for q, top in ((3, 4),) if hamming else ((0, 4), (3, 2)):
            want = run("--search", full, "--query", paths[q], "--top", top, *hamming)
            got = run("--index", idx, "--query", paths[q], "--top", top, *hamming)
            assert got == want and len(want.strip().split("\n")) == top
            want_im = (E.query(ref, bare, sigs, bare[q], sigs[q], 24, top) if hamming else R.query(ref, bare[q], top))[0]
            assert [l.split("\t")[1] for l in got.strip().split("\n")] == [paths[i] for i in want_im]
    # --verify takes the candidates' rows from the index's list
    plain = str(tmp_path / "idx0.bin")
    want = run("--search", full, "--query", paths[0], "--top", 3, "--verify")
    assert run("--index", plain, "--query", paths[0], "--top", 3, "--verify") == want and len(want.strip().split("\n")[0].split("\t")) == 4
    # a failed add leaves the old pair: the list names a file that does not exist
    before = (open(idx, "rb").read(), open(idx + ".list").read())
    more.write_text(str(tmp_path / "no_such.hesaff.words") + "\n")
    r = subprocess.run([EXE, "--index", idx, "--add", str(more)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stdout == "" and "no_such" in r.stderr
    assert (open(idx, "rb").read(), open(idx + ".list").read()) == before
    # an embedded query on a plain index is refused, named
    r = subprocess.run([EXE, "--index", str(tmp_path / "idx0.bin"), "--query", paths[0], "--hamming", "24"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stdout == ""


@pytest.mark.gpu
def test_end_to_end_cpp_members(e2e, tmp_path):
    """tests/native/index_growth_members.cpp: buildIndex over three images, addToIndex of the fourth, saveIndex, loadIndex into a second
    detector and queryIndex through hesaff.hpp print what the Python path holds"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, res, words, bare, sigs, vocab, ref = e2e
    exe = str(tmp_path / "index_growth_members")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "index_growth_members.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    r = subprocess.run([exe, vfile, str(tmp_path / "members.index")] + [os.path.join(GOLD, n + ".pgm") for n in E2E_IMAGES], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want_im, want_sc = R.query(ref, bare[3], 4)[:2]
    ranked = ["%d %d %.17g" % (j + 1, i, s) for j, (i, s) in enumerate(zip(want_im, want_sc))]
    assert r.stdout.strip().split("\n") == ["A " + l for l in ranked] + ["L " + l for l in ranked] + ["P refused"]
    f = hesaff_amd.read_index_file(str(tmp_path / "members.index"))
    assert f["n_images"] == 4 and np.array_equal(f["df"], ref[1])
