"""GPU suite of removal from the image index (hesaff_index_remove, hesaff_get_index_remove_ms, include/hesaff_amd.h;
kernels_index_remove.h).  The reference is the numpy definition on the REMAINING images (tests/index_remove_ref.py over
tests/index_ref.py and tests/embedding_ref.py), never the code under test.  Every comparison is bit for bit: df, idf, norm2 and the
offsets as arrays, the posting and key lists as per-word sorted multisets, dot, nq2, the float64 scores as uint64 bit patterns, the
ranked images and the remap."""
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
from tests import index_remove_ref as X
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
ARG = -2
SIZES = [0, 1, 63, 64, 65, 200]
TILE = 1024   # HS_GROW_TILE: positions per block
SCAN = 4096   # elements per block of the scan


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


def _want_postings(ref):
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
    """the context's index against the numpy build of `images`: tables, offsets, lists"""
    ref = R.build(images, K) if ref is None else ref
    df, idf, norm2 = ctx.index_tables()
    assert np.array_equal(df, ref[1]), (what, "df")
    assert np.array_equal(idf, ref[2]), (what, "idf")
    assert np.array_equal(norm2, ref[3]), (what, "norm2", np.nonzero(norm2 != ref[3])[0][:8].tolist())
    assert ctx.index_info == (len(images), K, sum(len(w) for w in images), int(ref[1].sum())), (what, ctx.index_info)
    offsets, im, tf = ctx.index_postings()
    assert np.array_equal(offsets, np.concatenate([[0], np.cumsum(ref[1].astype(np.int64))])), (what, "offsets")
    for got, want, name in zip(_sorted_lists(offsets, im, tf), _want_postings(ref), ("word", "image", "tf")):
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


def _sig_for(words, seed):
    """signatures in which keys of one word collide (two values per word) and differ in few bits"""
    rng = np.random.RandomState(seed + len(words))
    base = (np.asarray(words, np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0x5555)
    flip = np.where(rng.randint(0, 2, len(words)) == 1, np.uint64(0xFFFFFF), np.uint64(0))
    return (base ^ flip).astype(np.uint64)


def _random_images(n, K, seed, most=40):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, K, rng.randint(0, most + 1)).astype(np.int32) for _ in range(n)]


def _remove_and_check(ctx, images, gone, K, what, queries=(), sigs=None, T=(0, 24, 64), built=False):
    """build(images) unless the context holds it, remove(gone), and everything against the numpy build of what remains"""
    images = _i32(images)
    if not built:
        ctx.build_index(images, K, signatures=sigs)
    if queries:
        ctx.query_index(np.asarray(queries[0], np.int32), 3)   # (so that there IS a last query whose values the removal has to clear)
    remap = ctx.remove_from_index(gone)
    ref, want_remap = X.remove(images, gone, K)
    assert remap.dtype == np.int32 and np.array_equal(remap, want_remap), (what, "remap")
    _scores_are_zero(ctx, what)
    left = X.remaining(images, gone)
    left_sigs = None if sigs is None else X.remaining(sigs, gone)
    _check_index(ctx, left, K, what, left_sigs, ref=ref)
    for q in queries:
        q = np.asarray(q, np.int32)
        _check_query(ctx, ref, left, q, min(len(left), 1024), what + ", query of %d" % len(q))
        if sigs is not None:
            qs = _sig_for(q, 5)
            for t in T:
                _check_query(ctx, ref, left, q, 7, what + ", T = %d" % t, left_sigs, qs, t)
    return ref


def _both(ctx, images, gone, K, what, queries=(), T=(0, 24, 64)):
    """plain and embedded"""
    images = _i32(images)
    ref = _remove_and_check(ctx, images, gone, K, what, queries)
    _remove_and_check(ctx, images, gone, K, what + ", embedded", queries, [_sig_for(w, 1) for w in images], T)
    return ref


# ---------------------------------------------------------------- removal against rebuild

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 33, 300])
def test_remove_against_rebuild(gctx, K):
    """N = 2, m = 1 (either image); then 107 random images with 37 removed, plain and embedded, with queries of an image that
    stays, of one that went and of random words"""
    two = [[0, K - 1], [K - 1, K - 1]]
    for g in (0, 1):
        _both(gctx, two, [g], K, "N = 2, image %d goes" % g, [[0], [K - 1]])
    images = _random_images(107, K, 1)
    rng = np.random.RandomState(K)
    gone = rng.permutation(107)[:37]
    stays = [i for i in range(107) if i not in set(gone.tolist())]
    queries = [images[stays[3]], images[gone[5]], rng.randint(0, K, 50)]
    _both(gctx, images, gone, K, "107 - 37, K = %d" % K, queries)


@pytest.mark.gpu
@pytest.mark.parametrize("K,most", [(1, 3), (33, 40), (5000, 12)])
def test_remove_over_many_tiles(gctx, K, most):
    """2500 images with 900 removed: both passes run over many tiles of 1024 positions - one list through all of them (K = 1), a few
    long lists per tile whose runs cross wavefronts and blocks (K = 33), and at K = 5000 hundreds of short lists and empty words
    inside every tile - plain and embedded"""
    images = _random_images(2500, K, 3, most)
    gone = np.random.RandomState(4).permutation(2500)[:900]
    assert K == 1 or int(R.build(images, K)[1].sum()) > 8 * TILE
    _both(gctx, images, gone, K, "many tiles, K = %d" % K, [images[7], images[int(gone[9])]], T=(24,))


def _lists_of_sizes(sizes, first_word, step, n_images, seed):
    """images in which word first_word + j * step is held by sizes[j] distinct images (a posting list of that length)"""
    rng = np.random.RandomState(seed)
    images = [[] for _ in range(n_images)]
    for j, m in enumerate(sizes):
        for i in rng.permutation(n_images)[:m]:
            images[i] += [first_word + j * step] * int(rng.randint(1, 4))
    return [np.array(rng.permutation(w), np.int32) for w in images]


def _ascending_file(images, K, sigs, path):
    """the index of `images` as a file with every list in ascending image order.  A file's order is the loaded index's: after
    load_index(path) the position in a list is the rank among the word's holders"""
    hesaff_amd.write_index_file(path, *G.file_arrays(images, K, sigs))
    return path


@pytest.mark.gpu
@pytest.mark.parametrize("embedded", [False, True])
def test_remove_at_every_place_of_lists_of_wave_sizes(gctx, embedded, tmp_path):
    """lists of 0, 1, 63, 64, 65 and 200 postings, the used words 7 apart from word 40 of K = 300 (runs of empty words before,
    between and behind), loaded from a file so that the order inside each list is known; of each list the first posting is removed,
    the last, all but one, and every one (its word ends at df 0) - which for the list of one is the only one"""
    K = 300
    images = _lists_of_sizes(SIZES, 40, 7, 260, 11)
    sigs = [_sig_for(w, 2) for w in images] if embedded else None
    path = _ascending_file(images, K, sigs, str(tmp_path / "lists.index"))
    full = R.build(images, K)
    assert full[1][40:40 + 7 * 6:7].tolist() == SIZES
    for j, size in enumerate(SIZES[1:], 1):
        word = 40 + 7 * j
        holders = [i for i, w in enumerate(images) if word in w]   # ascending: the list's order after the load
        assert len(holders) == size
        for name, gone in (("first", holders[:1]), ("last", holders[-1:]), ("all but one", holders[:-1] if size > 1 else holders), ("every one", holders)):
            gctx.load_index(path)
            ref = _remove_and_check(gctx, images, gone, K, "list of %d, %s" % (size, name), [images[holders[0]], [word, 47]] if name == "first" else (), sigs, T=(24,),
                                    built=True)
            left = size - len(gone)
            assert ref[1][word] == left and (left > 0 or ref[2][word] == 0)
            assert not ref[1][:40].any() and not ref[1][76:].any()


@pytest.mark.gpu
def test_remove_from_one_list_across_tiles_and_from_a_wave_of_64_words(gctx, tmp_path):
    """word 5 is held by 2600 of 2700 images: one list of more than two tiles, its runs crossing wavefronts, blocks and tiles, with
    survivors and removed postings alternating, in blocks of 64, and in blocks of 1024; and words 100 .. 227 are held by one image
    each, once: wavefronts whose 64 positions belong to 64 different words, each list losing its only posting or keeping it"""
    K = 300
    rng = np.random.RandomState(21)
    images = [np.array(([5] * int(rng.randint(1, 3)) if i < 2600 else []) + ([100 + i] if i < 128 else []) + ([250] if i % 3 == 0 else []), np.int32) for i in range(2700)]
    sigs = [_sig_for(w, 3) for w in images]
    patterns = {"every second": np.arange(0, 2700, 2), "blocks of 64": np.array([i for i in range(2700) if (i // 64) % 2 == 1]),
                "blocks of 1024": np.array([i for i in range(2700) if (i // TILE) % 2 == 0]), "all of the list but one": np.arange(1, 2650),
                "one of the single words": np.array([37]), "all of the single words": np.arange(0, 128)}
    for s in (None, sigs):
        path = _ascending_file(images, K, s, str(tmp_path / ("long%d.index" % (s is not None))))
        for name, gone in patterns.items():
            gctx.load_index(path)
            _remove_and_check(gctx, images, gone, K, name, [[5, 250, 101]], s, T=(24,), built=True)


@pytest.mark.gpu
def test_remove_moves_an_idf_to_zero_and_back(gctx):
    K = 8
    # word 1 loses its last posting: df 0, idf 0
    ref = _both(gctx, [[3, 5], [3, 3, 5], [5, 1], [2]], [2], K, "a word's last posting goes", [[1], [3, 5]])
    assert ref[1][1] == 0 and ref[2][1] == 0
    # word 3 is in two of three images; the third goes: idf 0, and the norms of the two shrink
    images = [[3, 5, 2], [3, 3, 5], [5, 1]]
    before = R.build(_i32(images), K)
    ref = _both(gctx, images, [2], K, "a word ends up in every image", [[3], [3, 2]])
    assert before[2][3] > 0 and ref[2][3] == 0 and ref[3][0] < before[3][0] and ref[3][1] == 0
    # a keyless image goes and word 7 is left in every image
    images = [[7, 1], [7], [7, 2], []]
    before = R.build(_i32(images), K)
    ref = _both(gctx, images, [3], K, "the keyless image goes: word 7 is in every image", [[7], [7, 1]])
    assert before[2][7] > 0 and ref[2][7] == 0
    ref = _both(gctx, images, [1], K, "a holder goes: word 7 stays rare", [[7], [7, 1]])
    assert ref[2][7] > 0 and ref[1][7] == 2
    # the reverse: word 7 is in 399 of 400 images, 256 log2(400 / 399) < 1: idf 0; 380 of its holders go and 19 of 20 hold it: rare
    # again, and the norms of the images that stay come back from what word 2 alone gave them
    images = [[2, 1]] + [[7, 2] if i % 2 else [7] for i in range(399)]
    before = R.build(_i32(images), K)
    ref = _both(gctx, images, np.arange(1, 381), K, "an idf-0 word is rare again", [[7], [7, 2]], T=(24,))
    assert before[2][7] == 0 and before[1][7] == 399 and ref[1][7] == 19 and ref[2][7] > 0 and (ref[3][1:] > 0).all()


@pytest.mark.gpu
@pytest.mark.parametrize("N", [SCAN - 1, SCAN, SCAN + 1, 2 * SCAN + 1])
def test_remove_across_the_scan_blocks(gctx, N):
    """almost all images keyless, N on the edges of the scan's blocks of 4096 flags; the first, the last, every second, and all but
    the last image go.  The images around every block edge hold keys, so a wrong remap shows in the postings and the norms"""
    K = 33
    rng = np.random.RandomState(N)
    images = [np.zeros(0, np.int32)] * N
    for i in [0, 1, 2, N - 3, N - 2, N - 1] + [e + d for e in (SCAN, 2 * SCAN) for d in (-2, -1, 0, 1) if 0 <= e + d < N]:
        images[i] = rng.randint(0, K, 5).astype(np.int32)
    for name, gone in (("the first", [0]), ("the last", [N - 1]), ("every second", np.arange(0, N, 2)), ("every other second", np.arange(1, N, 2)),
                       ("all but the last", np.arange(N - 1)[::-1])):
        _remove_and_check(gctx, images, gone, K, "N = %d, %s" % (N, name), [images[N - 1]])


def _holders_case(ctx, N, K, holders, gone, embedded=False):
    """an index of N images of which only `holders` (number -> words) hold keys, built through the C interface (a million Python lists
    are slow); `gone` removed; the remaining images are few enough, or keyless enough, for index_ref"""
    counts = np.zeros(N, np.int32)
    for i, w in holders.items():
        counts[i] = len(w)
    flat = np.array([w for i in sorted(holders) for w in holders[i]], np.int32)
    sig = _sig_for(flat, 9)
    if embedded:
        assert ctx.L.hesaff_index_build_embedded(ctx.h, N, counts.ctypes.data, flat.ctypes.data, 1, sig.ctypes.data, K) == 0
    else:
        assert ctx.L.hesaff_index_build(ctx.h, N, counts.ctypes.data, flat.ctypes.data, 1, K) == 0
    remap = ctx.remove_from_index(gone)
    assert np.array_equal(remap, X.remap(N, gone))
    starts = np.concatenate([[0], np.cumsum(counts)])
    stay = np.nonzero(remap >= 0)[0]
    left = [flat[starts[i]:starts[i + 1]] for i in stay]
    left_sigs = [sig[starts[i]:starts[i + 1]] for i in stay] if embedded else None
    return left, left_sigs


@pytest.mark.gpu
def test_remove_with_a_million_words_and_from_a_million_images(gctx):
    K = 1 << 20
    images = [[0, 0, K - 1], [], [K - 1, 5], [0], [K - 1], [0, 0, 0, K // 2], [], [K - 1, K - 2]]
    _both(gctx, images, [2, 5], K, "K = 2^20", [[0, K - 1], [K // 2, K - 2, 5], [17]], T=(0, 64))
    # N = 2^20, all images keyless but a handful
    N, K = 1 << 20, 33
    holders = {0: [1, 2, 2], 70000: [2, 30], N - 3: [30, 30, 30, 7], N - 2: [7, 1], N - 1: [32]}
    for embedded in (False, True):
        left, sigs = _holders_case(gctx, N, K, holders, np.delete(np.arange(N), 70000), embedded)   # m = N - 1: one image stays
        assert len(left) == 1
        ref = _check_index(gctx, left, K, "m = N - 1", sigs)
        assert ref[1][[2, 30]].tolist() == [1, 1] and not ref[2].any()
    gone = np.delete(np.arange(N), [0, 5, 70000, N - 2])[::-1]                                      # four stay, one of them keyless
    left, _ = _holders_case(gctx, N, K, holders, gone)
    ref = _check_index(gctx, left, K, "m = N - 4")
    _check_query(gctx, ref, left, [2, 1, 7], 4, "m = N - 4")
    left, _ = _holders_case(gctx, N, K, holders, [70000, N - 1])                                    # m = 2 of 2^20: the others renumber
    assert len(left) == N - 2
    df, idf, norm2 = gctx.index_tables()
    want_df = np.zeros(K, np.uint32)
    kept = {0: holders[0], N - 4: holders[N - 3], N - 3: holders[N - 2]}
    for w in kept.values():
        want_df[np.unique(w)] += 1
    want_idf = np.array([R.ilog2_q8(N - 2, int(d)) if d else 0 for d in want_df], np.uint64)
    want_norm2 = np.zeros(N - 2, np.uint64)
    for i, w in kept.items():
        u, c = np.unique(w, return_counts=True)
        want_norm2[i] = ((c.astype(np.uint64) * want_idf[u]) ** 2).sum(dtype=np.uint64)
    assert np.array_equal(df, want_df) and np.array_equal(idf, want_idf.astype(np.uint32)) and np.array_equal(norm2, want_norm2)
    assert gctx.index_info == (N - 2, K, 9, 6)
    _, gi, gt = _sorted_lists(*gctx.index_postings())
    assert list(zip(gi.tolist(), gt.tolist())) == [(0, 1), (N - 3, 1), (0, 2), (N - 4, 1), (N - 3, 1), (N - 4, 3)]


@pytest.mark.gpu
def test_remove_images_without_keys_and_whole_words(gctx):
    K = 33
    images = _random_images(12, K, 5)
    images[4] = np.zeros(0, np.int32)
    images[9] = np.zeros(0, np.int32)
    before = R.build(images, K)
    # removed images without keys: only N changes, yet every idf and every norm does
    ref = _both(gctx, images, [9, 4], K, "only N changes", [images[0], images[2]])
    assert np.array_equal(ref[1], before[1]) and (ref[2][ref[1] > 0] <= before[2][ref[1] > 0]).all() and (ref[2] != before[2]).any()
    # tf > 1 throughout, and image 1 holds all 500 keys of word 17
    rng = np.random.RandomState(6)
    images = [np.repeat(rng.randint(0, 16, 3), rng.randint(2, 90, 3)).astype(np.int32) for _ in range(7)]
    images[1] = np.concatenate([images[1], np.full(500, 17, np.int32)])
    ref = _both(gctx, images, [1], K, "all keys of a word go", [images[0], [17], images[1]])
    assert ref[1][17] == 0 and ref[2][17] == 0
    ref = _both(gctx, images, [0, 6, 3], K, "tf > 1", [images[1], [17]])
    assert ref[0][0][1].max() == 500


# ---------------------------------------------------------------- composition

@pytest.mark.gpu
def test_remove_composes_with_add_and_with_itself(gctx):
    K = 300
    A, B = _random_images(40, K, 41), _random_images(17, K, 42)
    sa, sb = [_sig_for(w, 1) for w in A], [_sig_for(w, 2) for w in B]

    def state():
        emb = gctx.index_embedded()
        return [a.tobytes() for a in gctx.index_tables()] + [a.tobytes() for a in _sorted_lists(*gctx.index_postings())] + [gctx.index_postings()[0].tobytes(), repr(gctx.index_info)] + \
               ([] if emb is None else [a.tobytes() for a in _sorted_lists(*emb)] + [emb[0].tobytes()])
    for embedded in (False, True):
        s = (lambda x: x) if embedded else (lambda x: None)
        # an add of B to A followed by a removal of B gives A's index
        gctx.build_index(A, K, signatures=s(sa))
        gctx.add_to_index(B, signatures=s(sb))
        gctx.remove_from_index(np.arange(40, 57))
        refA = _check_index(gctx, A, K, "A + B - B", s(sa))
        _check_query(gctx, refA, A, A[3], 40, "A + B - B")
        # numbers given unsorted equal the sorted call; a removal in two calls, the second numbered by the first's remap, equals one
        images, sigs = A + B, sa + sb
        gone = np.random.RandomState(43).permutation(57)[:20]
        gctx.build_index(images, K, signatures=s(sigs))
        r_unsorted = gctx.remove_from_index(gone)
        one = state()
        _check_index(gctx, X.remaining(images, gone), K, "unsorted", s(X.remaining(sigs, gone)))
        gctx.build_index(images, K, signatures=s(sigs))
        assert np.array_equal(gctx.remove_from_index(np.sort(gone)), r_unsorted) and state() == one
        gctx.build_index(images, K, signatures=s(sigs))
        first = gctx.remove_from_index(gone[:8])
        second = gctx.remove_from_index(first[gone[8:]])
        assert (first[gone[8:]] >= 0).all() and state() == one
        assert np.array_equal(np.where(first >= 0, second[np.maximum(first, 0)], -1), r_unsorted)
        # remove then add equals the build of the result
        gctx.add_to_index(B[:5], signatures=s(sb[:5]))
        left = X.remaining(images, gone) + B[:5]
        ref = _check_index(gctx, left, K, "remove then add", s(X.remaining(sigs, gone) + sb[:5]))
        _check_query(gctx, ref, left, B[2], 42, "remove then add")
        if embedded:
            _check_query(gctx, ref, left, B[2], 7, "remove then add, T = 24", X.remaining(sigs, gone) + sb[:5], sb[2], 24)


# ---------------------------------------------------------------- persistence and batches

@pytest.mark.gpu
def test_save_load_and_batches_around_a_removal(gctx, tmp_path):
    K = 33
    images = _random_images(40, K, 70)
    images[7] = np.zeros(0, np.int32)
    sigs = [_sig_for(w, 7) for w in images]
    gone = [3, 39, 0, 21, 22]
    left, left_sigs = X.remaining(images, gone), X.remaining(sigs, gone)
    ref = R.build(left, K)
    queries = [images[5], images[3], np.array([5, 5, 9], np.int32), np.zeros(0, np.int32)]
    qsigs = [_sig_for(q, 7) for q in queries]
    for name, s, ls in (("plain", None, None), ("embedded", sigs, left_sigs)):
        gctx.build_index(images, K, signatures=s)

        def rows_equal_single_calls(what):
            for kw in ({},) if s is None else ({}, {"hamming": 24}):
                bi, bs = gctx.query_index_batch(queries, 9, **({"signatures": qsigs, **kw} if kw else {}))
                for j, q in enumerate(queries):
                    im, sc = gctx.query_index(q, 9, **({"signatures": qsigs[j], **kw} if kw else {}))
                    assert np.array_equal(bi[j], im) and np.array_equal(_bits(bs[j]), _bits(sc)), (name, what, j)
        rows_equal_single_calls("before")
        gctx.remove_from_index(gone)
        rows_equal_single_calls("after")
        bi, bs = gctx.query_index_batch(queries, 9)
        for j, q in enumerate(queries):
            want = R.query(ref, q, 9)
            assert bi[j].tolist() == want[0].tolist() and np.array_equal(_bits(bs[j]), _bits(want[1])), (name, j)
        # save after a removal and load in a fresh context
        path = str(tmp_path / (name + ".index"))
        gctx.save_index(path)
        f = hesaff_amd.read_index_file(path)
        assert (f["embedded"], f["k"], f["n_images"], f["n_keys"], f["n_postings"]) == (s is not None, K, 35, sum(len(w) for w in left), int(ref[1].sum()))
        with hesaff_amd.HesaffContext(device=0) as c:
            c.load_index(path)
            _check_index(c, left, K, "loaded " + name, ls, ref=ref)
            _check_query(c, ref, left, images[5], 35, "loaded " + name)
            # load an index and then remove from it
            more = [1, 34, 6]
            _remove_and_check(c, left, more, K, "removed after the load, " + name, [images[5], left[1]], ls, built=True)


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_remove_refusals_leave_index_vocabulary_and_embedding_alone():
    K = 33
    images = _random_images(12, K, 80)
    sigs = [_sig_for(w, 9) for w in images]
    vocab = V.family("uniform", K, seed=3)
    P = E.projection(5)
    tau = np.zeros((K, 64), np.int32)
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        L, h = c.L, c.h
        remove = L.hesaff_index_remove
        out = np.full(16, -77, np.int32)
        one = np.array([1], np.int32)
        assert remove(h, 1, one.ctypes.data, out.ctypes.data) == ARG and (out == -77).all()     # no index
        assert c.index_info is None
        with pytest.raises(hesaff_amd.HesaffError):
            c.remove_from_index([0])
        c.set_vocabulary(vocab)
        c.set_embedding(P, tau)
        for embedded in (False, True):
            c.build_index(images, K, signatures=sigs if embedded else None)
            ref = R.build(images, K)

            def state():
                s = [a.tobytes() for a in c.index_tables()] + [a.tobytes() for a in c.index_postings()] + [repr(c.index_info)]
                if embedded:
                    s += [a.tobytes() for a in c.index_embedded()]
                gp, gt = c.embedding()
                return s + [gp.tobytes(), gt.tobytes(), repr(c.vocabulary_size)]
            before = state()

            def refused(m, numbers, names=None):
                a = None if numbers is None else np.array(numbers, np.int32)
                assert remove(h, m, None if a is None else a.ctypes.data, out.ctypes.data) == ARG, (m, numbers)
                assert (out == -77).all(), (m, numbers)
                if names is not None:
                    assert names in L.hesaff_last_error(h).decode(), L.hesaff_last_error(h).decode()
            assert remove(None, 1, one.ctypes.data, out.ctypes.data) == ARG
            refused(1, None)
            for m in (0, -1, 12, 13, 1 << 20):
                refused(m, list(range(12)) + [0] * 4)
            refused(2, [3, -1], "image -1 lies outside 0 .. 11")
            refused(2, [12, 3], "image 12 lies outside 0 .. 11")
            refused(1, [1 << 30])
            refused(3, [5, 7, 5], "image 5 is given twice")
            refused(11, [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0], "image 0 is given twice")
            with pytest.raises(hesaff_amd.HesaffError, match="image 4 is given twice") as e:
                c.remove_from_index([4, 4])
            assert e.value.code == ARG
            assert state() == before, "embedded" if embedded else "plain"
            # the previous index answers a query, and the same call well-formed works
            _check_query(c, ref, images, images[2], 12, "after the refusals")
            remap = c.remove_from_index([5, 7])
            assert np.array_equal(remap, X.remap(12, [5, 7]))
            _check_index(c, X.remaining(images, [5, 7]), K, "after the refusals", X.remaining(sigs, [5, 7]) if embedded else None)
        c.clear_index()
        ms = [C.c_float(7) for _ in range(4)]
        assert L.hesaff_get_index_remove_ms(h, None, *[C.byref(x) for x in ms[1:]]) == ARG and all(x.value == 7.0 for x in ms)
        assert L.hesaff_get_index_remove_ms(None, *[C.byref(x) for x in ms]) == ARG


@pytest.mark.gpu
def test_remove_ms_are_event_times(gctx):
    images = _random_images(30, 33, 60)
    sigs = [_sig_for(w, 1) for w in images]
    gctx.build_index(images, 33)
    gctx.remove_from_index([2])
    assert gctx.index_remove_ms() == (0.0, 0.0, 0.0, 0.0)
    gctx.set_profiling(1)
    try:
        gctx.build_index(images, 33)
        gctx.remove_from_index([2, 5])
        ms = gctx.index_remove_ms()
        print("index_remove_ms (count, tables, compact, keys):", ms)
        assert all(0.0 < v < 1000.0 for v in ms[:3]) and ms[3] == 0.0
        gctx.build_index(images, 33, signatures=sigs)
        gctx.remove_from_index([2, 5])
        ms = gctx.index_remove_ms()
        assert all(0.0 < v < 1000.0 for v in ms)
    finally:
        gctx.set_profiling(0)
    gctx.remove_from_index([0])
    assert gctx.index_remove_ms() == (0.0, 0.0, 0.0, 0.0)


# ---------------------------------------------------------------- end to end on the golden images

E2E_IMAGES = ["band_160x120", "band_96x96", "tiny_20x15", "band_131x77"]
E2E_GONE = 1


@pytest.fixture(scope="module")
def e2e(gctx):
    """the three band images and the keyless tiny one detected with a vocabulary of 40 rows and an embedding: keys, (word, dist2)
    rows, signatures.  The index holds all four; the second goes"""
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
    left = X.remaining(bare, [E2E_GONE])
    return imgs, res, words, bare, sigs, vocab, left, R.build(left, 40)


@pytest.mark.gpu
def test_end_to_end_python(gctx, e2e):
    imgs, res, words, bare, sigs, vocab, left, ref = e2e
    for s in (None, sigs):
        gctx.build_index(words, 40, signatures=s)
        assert gctx.remove_from_index([E2E_GONE]).tolist() == [0, -1, 1, 2]
        ls = None if s is None else X.remaining(s, [E2E_GONE])
        _check_index(gctx, left, 40, "four images less the second", ls, ref=ref)
        for q in (0, 1, 3):
            _check_query(gctx, ref, left, bare[q], 3, "words of image %d" % q)
            if s is not None:
                _check_query(gctx, ref, left, bare[q], 3, "words of image %d, T = 24" % q, ls, s[q], 24)
    im, sc = gctx.query_index(words[3], 3)
    assert im[0] == 2 and abs(sc[0] - 1.0) < 1e-15


@pytest.mark.gpu
def test_end_to_end_cli(gctx, e2e, tmp_path):
    """--search --save-index over the four words files, --index --remove of the second (named twice), --index --query: the ranking
    printed equals --search's over the list without the removed file line for line, plain and with --hamming; the pair of files is
    rewritten whole"""
    imgs, res, words, bare, sigs, vocab, left, ref = e2e
    paths = []
    for j, ((_, keys), w, g) in enumerate(zip(res, words, sigs)):
        paths.append(str(tmp_path / ("%d_%s.pgm.hesaff.words" % (j, E2E_IMAGES[j]))))
        hesaff_amd.write_words(paths[-1], keys, w, gctx.params.mrSize, 40)
        hesaff_amd.write_signatures(paths[-1][:-len(".words")] + ".sigs", g)
    kept = X.remaining(paths, [E2E_GONE])
    full, rest, gone = tmp_path / "full.txt", tmp_path / "rest.txt", tmp_path / "gone.txt"
    full.write_text("\n".join(paths) + "\n"); rest.write_text("\n".join(kept) + "\n"); gone.write_text(paths[E2E_GONE] + "\n" + paths[E2E_GONE] + "\n")

    def run(*args):
        r = subprocess.run([EXE] + [str(a) for a in args], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (args, r.stderr)
        return r.stdout
    for hamming in ((), ("--hamming", "24")):
        idx = str(tmp_path / ("idx%d.bin" % len(hamming)))
        assert run("--search", full, "--save-index", idx, *hamming) == ""
        assert run("--index", idx, "--remove", gone) == ""
        assert open(idx + ".list").read() == "\n".join(kept) + "\n"
        f = hesaff_amd.read_index_file(idx)
        assert (f["n_images"], f["n_keys"], f["embedded"]) == (3, sum(len(w) for w in left), bool(hamming)) and np.array_equal(f["df"], ref[1])
        assert not [n for n in os.listdir(str(tmp_path)) if ".part" in n or ".new" in n]
        for q, top in ((3, 3), (E2E_GONE, 2)):
            want = run("--search", rest, "--query", paths[q], "--top", top, *hamming)
            got = run("--index", idx, "--query", paths[q], "--top", top, *hamming)
            assert got == want and len(want.strip().split("\n")) == top
            ls = X.remaining(sigs, [E2E_GONE])
            want_im = (E.query(ref, left, ls, bare[q], sigs[q], 24, top) if hamming else R.query(ref, bare[q], top))[0]
            assert [l.split("\t")[1] for l in got.strip().split("\n")] == [kept[i] for i in want_im]
    # a path the list no longer holds is refused, named, and leaves the pair
    before = (open(idx, "rb").read(), open(idx + ".list").read())
    r = subprocess.run([EXE, "--index", idx, "--remove", str(gone)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stdout == "" and paths[E2E_GONE] in r.stderr and len(r.stderr.strip().split("\n")) == 1
    assert (open(idx, "rb").read(), open(idx + ".list").read()) == before


@pytest.mark.gpu
def test_end_to_end_cpp_members(e2e, tmp_path):
    """tests/native/index_remove_members.cpp: buildIndex over the four images, removeFromIndex of the second and queryIndex through
    hesaff.hpp print what the Python path holds"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, res, words, bare, sigs, vocab, left, ref = e2e
    exe = str(tmp_path / "index_remove_members")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "index_remove_members.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    r = subprocess.run([exe, vfile, str(E2E_GONE)] + [os.path.join(GOLD, n + ".pgm") for n in E2E_IMAGES], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want_im, want_sc = R.query(ref, bare[3], 4)[:2]
    assert r.stdout.strip().split("\n") == ["M %d %d" % (i, v) for i, v in enumerate(X.remap(4, [E2E_GONE]))] + \
        ["R %d %d %.17g" % (j + 1, i, s) for j, (i, s) in enumerate(zip(want_im, want_sc))] + ["T refused", "A refused", "P refused"]
