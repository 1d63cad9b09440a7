"""GPU suite of vocabulary neighbours (hesaff_set_vocabulary_neighbours, include/hesaff_amd.h; k_assign_neighbours,
kernels_neighbours.h).  The reference is tests/neighbours_ref.py: int64 differences and a stable argsort in numpy.  Every comparison is
bit for bit - the rows, whose ties the reference alone decides, their order and the distances."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import FROM_SHAPES, OUT_BIN, OUT_WORDS, _binding
from tests import embedding_ref as E
from tests import index_ref as I
from tests import neighbours_ref as N
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
E2E_IMAGES = ["band_160x120", "band_96x96", "band_160x120", "tiny_20x15", "band_96x96"]
E2E_KEYS = [221, 74, 221, 0, 74]
COUNTS = (1, 31, 32, 33, 63, 64, 65, 255, 256, 257)            # the key-tile, wavefront and block borders
SIZES = (1, 2, 7, 8, 9, 31, 32, 33, 63, 64, 65, 4099)          # below, at and above R; the word-tile borders; 129 tiles
RANKS = (1, 2, 3, 4, 8)                                        # both ends, and every list capacity (2, 4, 8) full and not full
ARG = -2

_ref = {}


def reference(desc, vocab, tag):
    """N.neighbours at R = 8, computed once per tagged (desc, vocab) pair; the answer at R is its first R ranks by definition"""
    if tag not in _ref:
        _ref[tag] = N.neighbours(desc, vocab, 8)
        _ref[tag].setflags(write=False)
    return _ref[tag]


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).reshape(len(want), int(np.prod(want.shape[1:]))).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d keys differ, first %s: got %s, want %s" % (what, len(bad), len(want), bad[:6].tolist(),
                                                                                  got[bad[:2]].tolist(), want[bad[:2]].tolist())


def _const(vals):
    return np.stack([np.full(128, v, np.uint8) for v in vals])


@pytest.fixture(scope="module")
def nctx():
    """a context of its own with max_batch = 2 (the session's context keeps no vocabulary and R = 1)"""
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        assert c.vocabulary_size == 0 and c.vocabulary_neighbours() == 1
        yield c
        c.set_vocabulary_neighbours(1)
        c.set_vocabulary(None)


def _run(nctx, desc, vocab, R):
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(R)
    return nctx.assign_neighbours(desc)


# ---------------------------------------------------------------- the stage operator: random rows with ties

def _alphabet(name, rows, seed):
    """bytes from a small alphabet, so that equal distances are everywhere: {0, 1} (dist2 = the Hamming distance, 0 .. 128) and
    {0, 255} (255^2 times it: the largest values there are)"""
    rng = np.random.RandomState(seed)
    letters = np.array({"bits": [0, 1], "extremes": [0, 255]}[name], np.uint8)
    return letters[rng.randint(0, len(letters), (rows, 128))]


@pytest.mark.gpu
@pytest.mark.parametrize("family", ("bits", "extremes"))
@pytest.mark.parametrize("K", SIZES)
def test_stage_random_rows_with_ties(nctx, family, K):
    """n in COUNTS, R in RANKS against one K: every (n, R) pair through hesaff_stage_assign_neighbours"""
    desc = _alphabet(family, 257, seed=11)
    vocab = np.ascontiguousarray(_alphabet(family, 4099, seed=12)[:K])
    want = reference(desc, vocab, ("random", family, K))
    if K >= 64:   # the cut of the list falls inside a tie for many keys: the tie rule decides what the list holds, not only its order
        assert (want[:, 3, 1] == want[:, 4, 1]).sum() >= 100
    nctx.set_vocabulary(vocab)
    for R in RANKS:
        nctx.set_vocabulary_neighbours(R)
        for n in COUNTS:
            _same(nctx.assign_neighbours(desc[:n]), want[:n, :R], "%s, K = %d, R = %d, n = %d" % (family, K, R, n))
    present = want[:, :, 0] >= 0
    assert (present.sum(axis=1) == min(K, 8)).all() and (want[~present] == N.NONE).all()


# ---------------------------------------------------------------- the stage operator: constructed rows

@pytest.mark.gpu
@pytest.mark.parametrize("K", (5, 8, 33, 300))
def test_all_rows_identical(nctx, K):
    """the tie rule, and the cut inside a tie: rows 0 .. R - 1 at one distance"""
    vocab = _const([9] * K)
    desc = _const([10, 9, 200])
    for R in RANKS:
        got = _run(nctx, desc, vocab, R)
        for i, d2 in enumerate((128, 0, 128 * 191 * 191)):
            want = [[k, d2] if k < K else list(N.NONE) for k in range(R)]
            assert got[i].tolist() == want, (K, R, i, got[i].tolist())


@pytest.mark.gpu
def test_one_accumulator_element_across_tiles_then_the_two_lane_halves(nctx):
    """the nearest are rows 5, 37, 69, ... - one accumulator element of one lane, tile after tile: a running best per element would keep
    one of them, the per-lane list must keep all.  Then rows 0 .. 3 (lower lane half) against 4 .. 7 (upper half) of one tile,
    interleaved in distance: only the merge across the halves puts them in order"""
    vocab = _const([200] * 300)
    for j in range(8):
        vocab[5 + 32 * j] = 50 + (7 - j)          # nearer the later the tile: every one is inserted at the head
    desc = _const([50])
    for R in RANKS:
        got = _run(nctx, desc, vocab, R)
        assert got[0, :, 0].tolist() == [5 + 32 * (7 - r) for r in range(R)], (R, got.tolist())
        assert got[0, :, 1].tolist() == [128 * r * r for r in range(R)]
    vocab = _const([200] * 40)
    for r, row in enumerate((4, 0, 5, 1, 6, 2, 7, 3)):   # alternating halves
        vocab[row] = 50 + r
    for R in RANKS:
        got = _run(nctx, desc, vocab, R)
        assert got[0, :, 0].tolist() == [4, 0, 5, 1, 6, 2, 7, 3][:R], (R, got.tolist())
    vocab = _const([200] * 40)
    vocab[4:8] = _const([50, 51, 52, 53])                # all of the upper half first, then all of the lower
    vocab[0:4] = _const([54, 55, 56, 57])
    for R in RANKS:
        assert _run(nctx, desc, vocab, R)[0, :, 0].tolist() == [4, 5, 6, 7, 0, 1, 2, 3][:R]


@pytest.mark.gpu
@pytest.mark.parametrize("R", RANKS)
def test_nearest_rows_end_a_final_tile_that_is_mostly_pad(nctx, R):
    """K = 33 (one real row in the last tile, 31 pad rows) and K = R + 1: the nearest rows are the last real ones; a pad row never appears,
    also while the lists hold fewer than R real rows"""
    for K in (33, R + 1):
        vocab = _const([250] * K)
        near = list(range(K - 1, max(K - 1 - 8, -1), -1))       # K - 1 nearest, then K - 2, ...
        for r, row in enumerate(near):
            vocab[row] = 20 + r
        desc = _const([20, 19])
        got = _run(nctx, desc, vocab, R)
        want = N.neighbours(desc, vocab, R)
        assert want[0, :, 0].tolist() == near[:R] and (want[:, :, 0] < K).all() and (want[:, :, 0] >= 0).all()
        _same(got, want, "K = %d, R = %d" % (K, R))
    got = _run(nctx, _const([20]), _const([250] * 3), 8)          # K < R: the ranks that do not exist
    assert got[0].tolist() == [[0, 128 * 230 * 230], [1, 128 * 230 * 230], [2, 128 * 230 * 230]] + [list(N.NONE)] * 5


@pytest.mark.gpu
@pytest.mark.parametrize("R", RANKS)
def test_insertion_at_the_head_and_no_insertion_at_all(nctx, R):
    """the single nearest row is K - 1 while the others come early (the last tile inserts at the head of a full list), and the reverse
    (after the first tile nothing is ever inserted)"""
    K = 4099
    desc = _const([100])
    vocab = _const([240] * K)
    vocab[:8] = _const([110 + r for r in range(8)])
    vocab[K - 1] = 101
    got = _run(nctx, desc, vocab, R)
    assert got[0, :, 0].tolist() == ([K - 1] + list(range(8)))[:R], got.tolist()
    _same(got, N.neighbours(desc, vocab, R), "head")
    vocab[K - 1] = 240
    vocab[:8] = _const([101 + r for r in range(8)])
    got = _run(nctx, desc, vocab, R)
    assert got[0, :, 0].tolist() == list(range(8))[:R]
    _same(got, N.neighbours(desc, vocab, R), "none")


@pytest.mark.gpu
@pytest.mark.parametrize("R", RANKS)
def test_equal_distance_at_the_cut_goes_to_the_lower_row(nctx, R):
    """the R-th and the (R + 1)-th row at equal distance, in pairs (a, b), a < b: both in one lane ((3, 8): elements 3 and 4 of the lower
    half - by the C/D map, row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5), a lane meets its rows in ascending order), in the two
    halves with the higher row met by the other lane ((3, 4), (4, 8), (7, 8)), and in two tiles ((8, 36), (7, 32), (36, 4098)).  The
    pair is placed in both orders of the bytes that make the distance; the lower row takes the last rank"""
    K = 4099
    desc = _const([100])
    for a, b in ((3, 8), (3, 4), (4, 8), (7, 8), (8, 36), (7, 32), (36, 4098)):
        for va, vb in ((90, 110), (110, 90)):             # the same distance from either side
            vocab = _const([240] * K)
            nearer = [r for r in range(40, 40 + 3 * 8, 3)][:R - 1]   # R - 1 rows that are nearer, elsewhere
            for r, row in enumerate(nearer):
                vocab[row] = 101 + r
            vocab[a], vocab[b] = va, vb
            got = _run(nctx, desc, vocab, R)
            assert got[0, :, 0].tolist() == nearer + [a], ((a, b), R, got.tolist())
            assert got[0, R - 1, 1] == 128 * 100
            if R < 8:
                nctx.set_vocabulary_neighbours(R + 1)
                assert nctx.assign_neighbours(desc)[0, :, 0].tolist() == nearer + [a, b]


@pytest.mark.gpu
def test_largest_and_zero_distance_in_one_list(nctx):
    vocab = _const([255, 0, 255, 0])
    desc = _const([0, 255])
    far = 128 * 255 * 255
    assert far == 8323200
    got = _run(nctx, desc, vocab, 4)
    assert got.tolist() == [[[1, 0], [3, 0], [0, far], [2, far]], [[0, 0], [2, 0], [1, far], [3, far]]]


@pytest.mark.gpu
def test_asymmetric_rows_pin_the_accumulator_map(nctx):
    """key i = byte i at position i mod 128, zero elsewhere; word k = byte 3k + 1 (mod 256) at position k mod 128: which (key, word) pair
    an accumulator element belongs to decides nearly every answer, at every rank"""
    n, K = 200, 300
    desc = np.zeros((n, 128), np.uint8)
    desc[np.arange(n), np.arange(n) % 128] = np.arange(n) % 256
    vocab = np.zeros((K, 128), np.uint8)
    vocab[np.arange(K), np.arange(K) % 128] = (3 * np.arange(K) + 1) % 256
    want = N.neighbours(desc, vocab, 8)
    swapped, shifted = N.neighbours(vocab[:n], desc, 8), N.neighbours(desc, np.roll(vocab, 32, axis=0), 8)
    assert (want[:, :, 0] != swapped[:, :, 0]).mean() > 0.4 and (want[:, :, 0] != shifted[:, :, 0]).mean() > 0.9
    _same(_run(nctx, desc, vocab, 8), want, "asymmetric rows")


# ---------------------------------------------------------------- properties

@pytest.fixture(scope="module")
def mixed():
    """257 keys against 4099 rows of uniform bytes with planted duplicates and exact matches"""
    vocab = V.family("uniform", 4099, seed=100 + 4099)
    desc = V.family("uniform", 257, seed=7)
    vocab[40] = vocab[5]
    vocab[5 + 32 * 100] = vocab[5]
    desc[2] = vocab[5]
    desc[3] = vocab[4098]
    return desc, vocab, reference(desc, vocab, "mixed")


@pytest.mark.gpu
def test_rank_zero_is_the_plain_assignment_and_r_is_a_prefix_of_eight(nctx, mixed):
    desc, vocab, want = mixed
    assert want[2, :3].tolist() == [[5, 0], [40, 0], [3205, 0]] and want[3, 0].tolist() == [4098, 0]
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(1)
    plain = nctx.assign_words(desc)
    assert np.array_equal(plain, V.assign(desc, vocab))
    eight = None
    for R in (8, 4, 3, 2, 1):
        nctx.set_vocabulary_neighbours(R)
        got = nctx.assign_neighbours(desc)
        eight = got if R == 8 else eight
        _same(got, want[:, :R], "R = %d" % R)
        assert np.array_equal(got[:, 0], plain) and np.array_equal(got, eight[:, :R])
        assert np.array_equal(nctx.assign_words(desc), plain)          # the words keep their bytes under every R
        rows = got[:, :, 0]
        assert all(len(set(r.tolist())) == R for r in rows)            # every row of a list is distinct


@pytest.mark.gpu
def test_device_forms_equal_the_host_form(nctx, mixed):
    """hesaff_assign_neighbours_device on a [65, 164] tensor (descriptor 36 bytes in, the other bytes 0xFF) and packed [65, 128]; and
    hesaff_assign_words_device under R = 3: the words in the caller's array, the neighbours in the context's (neighbours_device)"""
    import torch
    desc, vocab, want = mixed
    desc = desc[:65]
    rec = np.full((65, 164), 0xFF, np.uint8)
    rec[:, 36:] = desc
    nctx.set_vocabulary(vocab)
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    for R in (1, 3, 8):
        nctx.set_vocabulary_neighbours(R)
        host = nctx.assign_neighbours(desc)
        _same(host, want[:65, :R], "host form, R = %d" % R)
        for src, stride, offset in ((rec, 164, 36), (desc, 128, 0)):
            t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
            out = torch.full((65, R, 2), -7, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            nctx.assign_neighbours_device(t.data_ptr(), 65, stride, offset, out.data_ptr())
            _same(out.cpu().numpy(), host, "stride %d, R = %d" % (stride, R))
    nctx.set_vocabulary_neighbours(3)
    t = torch.from_numpy(rec).cuda()
    words = torch.full((65, 2), -7, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    nctx.assign_words_device(t.data_ptr(), 65, 164, 36, words.data_ptr())
    assert np.array_equal(words.cpu().numpy(), want[:65, 0])
    ptr, rows, r = nctx.neighbours_device()
    assert rows == 65 and r == 3
    got = torch.empty((65, 3, 2), dtype=torch.int32, device="cuda")
    assert hip.hipMemcpy(ctypes.c_void_p(got.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(65 * 3 * 8), 3) == 0
    _same(got.cpu().numpy(), want[:65, :3], "neighbours beside assign_words_device")


@pytest.mark.gpu
def test_all_keys_at_once_equals_one_key_per_call(nctx, mixed):
    desc, vocab, want = mixed
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(4)
    _same(nctx.assign_neighbours(desc), want[:, :4], "all at once")
    single = np.concatenate([nctx.assign_neighbours(desc[i:i + 1]) for i in range(0, 257, 3)])
    _same(single, want[::3, :4], "one key per call")
    assert nctx.assign_neighbours(desc[:0]).shape == (0, 4, 2)


# ---------------------------------------------------------------- state

@pytest.mark.gpu
def test_setting_survives_set_vocabulary_and_one_after_four_is_the_plain_context(nctx, mixed):
    desc, vocab, want = mixed
    L, h = nctx.L, nctx.h
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(4)
    nctx.set_vocabulary(vocab[:300])
    assert nctx.vocabulary_neighbours() == 4 and nctx.assign_neighbours(desc[:3]).shape == (3, 4, 2)
    nctx.set_vocabulary(None)
    assert nctx.vocabulary_neighbours() == 4
    nctx.set_vocabulary(vocab)
    _same(nctx.assign_neighbours(desc), want[:, :4], "R = 4 after three vocabularies")
    for bad in (0, 9, -1, 1 << 20):
        assert L.hesaff_set_vocabulary_neighbours(h, bad) == ARG and nctx.vocabulary_neighbours() == 4
    r = ctypes.c_int(7)
    assert L.hesaff_get_vocabulary_neighbours(h, None) == ARG
    img = hesaff_amd.read_pnm(os.path.join(GOLD, "band_96x96.pgm"))
    (nh, keys), = nctx.detect_batch([img])
    four, words4 = nctx.neighbours(0), nctx.words(0)
    assert four.shape == (74, 4, 2) and np.array_equal(four[:, 0], words4)
    _same(four, N.neighbours(keys["desc"], vocab, 4), "detect_batch, R = 4")
    nctx.set_vocabulary_neighbours(1)
    assert nctx.vocabulary_neighbours() == 1 and np.array_equal(nctx.words(0), words4)   # the words stay readable
    (nh1, keys1), = nctx.detect_batch([img])
    assert keys1.tobytes() == keys.tobytes() and np.array_equal(nctx.words(0), words4)
    one = nctx.neighbours(0)
    assert one.shape == (74, 1, 2) and np.array_equal(one[:, 0], words4)
    p = ctypes.c_void_p(); n = ctypes.c_int(); tot = ctypes.c_int64()
    assert L.hesaff_get_neighbours(h, 0, ctypes.byref(p), ctypes.byref(n), ctypes.byref(r)) == 0 and r.value == 1 and n.value == 74
    assert L.hesaff_get_neighbours_device(h, ctypes.byref(p), ctypes.byref(tot), ctypes.byref(r)) == ARG   # the last call was a host call


@pytest.mark.gpu
def test_cells_and_neighbours_refuse_each_other_in_both_orders(nctx, mixed):
    desc, vocab, want = mixed
    L, h = nctx.L, nctx.h
    vocab = np.ascontiguousarray(vocab[:300])
    coarse = V.family("uniform", 3, seed=5)
    first = np.array([0, 100, 200, 300], np.uint32)
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(3)
    before = nctx.assign_neighbours(desc)
    assert L.hesaff_set_vocabulary_cells(h, 3, coarse.ctypes.data, first.ctypes.data) == ARG
    msg = L.hesaff_last_error(h).decode()
    assert "neighbours" in msg and "cell layer" in msg and "do not combine" in msg, msg
    assert nctx.vocabulary_cells() == 0 and nctx.vocabulary_neighbours() == 3
    assert np.array_equal(nctx.assign_neighbours(desc), before) and np.array_equal(nctx.assign_words(desc), before[:, 0])
    assert L.hesaff_set_vocabulary_cells(h, 0, None, None) == 0      # removing a layer is always allowed
    nctx.set_vocabulary_neighbours(1)
    nctx.set_vocabulary_cells(coarse, first)
    through = nctx.assign_words(desc)
    assert L.hesaff_set_vocabulary_neighbours(h, 3) == ARG
    msg = L.hesaff_last_error(h).decode()
    assert "neighbours" in msg and "cell layer" in msg and "do not combine" in msg, msg
    assert nctx.vocabulary_neighbours() == 1 and nctx.vocabulary_cells() == 3
    assert np.array_equal(nctx.assign_words(desc), through)
    assert L.hesaff_set_vocabulary_neighbours(h, 1) == 0             # ... and so is the default
    _same(nctx.assign_neighbours(desc), want_flat(desc, vocab), "R = 1 beside a layer: the whole vocabulary")
    nctx.set_vocabulary_cells(None, None)
    nctx.set_vocabulary_neighbours(3)
    assert np.array_equal(nctx.assign_neighbours(desc), before)
    img = hesaff_amd.read_pnm(os.path.join(GOLD, "band_96x96.pgm"))
    (nh, keys), = nctx.detect_batch([img])
    _same(nctx.neighbours(0), N.neighbours(keys["desc"], vocab, 3), "detects and assigns as before")


def want_flat(desc, vocab):
    return V.assign(desc, vocab).reshape(-1, 1, 2)


@pytest.mark.gpu
def test_refusals_leave_the_last_result_readable(nctx, mixed):
    import torch
    desc, vocab, want = mixed
    L, h = nctx.L, nctx.h
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(3)
    img = hesaff_amd.read_pnm(os.path.join(GOLD, "band_96x96.pgm"))
    (nh, keys), = nctx.detect_batch([img])
    last = nctx.neighbours(0)
    p = ctypes.c_void_p(); n = ctypes.c_int(); r = ctypes.c_int(); tot = ctypes.c_int64()
    out = np.full((4, 3, 2), 7, np.int32)
    t = torch.zeros((4, 164), dtype=torch.uint8, device="cuda")
    o = torch.zeros((4, 3, 2), dtype=torch.int32, device="cuda")
    d4 = np.ascontiguousarray(desc[:4])
    refusals = [
        L.hesaff_set_vocabulary_neighbours(h, 0), L.hesaff_set_vocabulary_neighbours(h, 9),
        L.hesaff_get_neighbours(h, 0, None, ctypes.byref(n), ctypes.byref(r)), L.hesaff_get_neighbours(h, 0, ctypes.byref(p), None, ctypes.byref(r)),
        L.hesaff_get_neighbours(h, 0, ctypes.byref(p), ctypes.byref(n), None), L.hesaff_get_neighbours(h, 1, ctypes.byref(p), ctypes.byref(n), ctypes.byref(r)),
        L.hesaff_get_neighbours(h, -1, ctypes.byref(p), ctypes.byref(n), ctypes.byref(r)),
        L.hesaff_get_neighbours_device(h, None, ctypes.byref(tot), ctypes.byref(r)), L.hesaff_get_neighbours_device(h, ctypes.byref(p), None, ctypes.byref(r)),
        L.hesaff_get_neighbours_device(h, ctypes.byref(p), ctypes.byref(tot), None),
        L.hesaff_get_neighbours_device(h, ctypes.byref(p), ctypes.byref(tot), ctypes.byref(r)),   # the last call was a host call
        L.hesaff_stage_assign_neighbours(h, -1, d4.ctypes.data, out.ctypes.data), L.hesaff_stage_assign_neighbours(h, 4, None, out.ctypes.data),
        L.hesaff_stage_assign_neighbours(h, 4, d4.ctypes.data, None),
        L.hesaff_assign_neighbours_device(h, -1, ctypes.c_void_p(t.data_ptr()), 164, 36, ctypes.c_void_p(o.data_ptr())),
        L.hesaff_assign_neighbours_device(h, 4, None, 164, 36, ctypes.c_void_p(o.data_ptr())),
        L.hesaff_assign_neighbours_device(h, 4, ctypes.c_void_p(t.data_ptr()), 164, 36, None),
    ]
    for stride, offset in ((127, 0), (124, 0), (164, -4), (164, 40), (128, 4), (166, 36), (164, 38), (164, 37)):
        refusals.append(L.hesaff_assign_neighbours_device(h, 4, ctypes.c_void_p(t.data_ptr()), stride, offset, ctypes.c_void_p(o.data_ptr())))
    assert refusals == [ARG] * len(refusals), refusals
    assert (out == 7).all() and int(o.cpu().abs().sum()) == 0
    assert nctx.vocabulary_neighbours() == 3 and np.array_equal(nctx.neighbours(0), last) and np.array_equal(nctx.words(0), last[:, 0])
    # without a vocabulary the getters and the operators refuse; the count stays
    nctx.set_vocabulary(None)
    assert L.hesaff_get_neighbours(h, 0, ctypes.byref(p), ctypes.byref(n), ctypes.byref(r)) == ARG
    assert L.hesaff_stage_assign_neighbours(h, 4, d4.ctypes.data, out.ctypes.data) == ARG and (out == 7).all()
    assert L.hesaff_assign_neighbours_device(h, 4, ctypes.c_void_p(t.data_ptr()), 164, 36, ctypes.c_void_p(o.data_ptr())) == ARG
    assert nctx.vocabulary_neighbours() == 3
    (nh2, keys2), = nctx.detect_batch([img])
    assert keys2.tobytes() == keys.tobytes()


@pytest.mark.gpu
def test_assign_ms_reports_the_neighbours_launch(nctx, mixed):
    desc, vocab, want = mixed
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(4)
    nctx.set_profiling(1)
    try:
        nctx.assign_neighbours(desc)
        ms = nctx.assign_ms
        print("assign_ms for 257 keys, K = 4099, R = 4: %.4f" % ms)
        assert 0.0 < ms < 1000.0
        nctx.assign_words(desc)
        assert 0.0 < nctx.assign_ms < 1000.0
    finally:
        nctx.set_profiling(0)
    nctx.assign_neighbours(desc)
    assert nctx.assign_ms == 0.0


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def e2e(nctx):
    """the five images, their keys and words at R = 1, and the vocabulary of the end-to-end tests: every descriptor of the first two
    images (so that every key's rank 0 has dist2 0) and five random rows; the reference at R = 8 per image; an embedding whose
    thresholds are the reference's lower medians over these keys"""
    nctx.set_vocabulary_neighbours(1)
    nctx.set_vocabulary(None)
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    plain = nctx.detect_batch(imgs)
    assert [len(k) for _, k in plain] == E2E_KEYS
    vocab = np.concatenate([plain[0][1]["desc"], plain[1][1]["desc"], V.family("uniform", 5, seed=77)])
    assert len(vocab) == 300
    want = [reference(k["desc"], vocab, "e2e%d" % i) for i, (_, k) in enumerate(plain)]
    assert all((w[:, 0, 1] == 0).all() for w in want) and (want[0][:, 1, 1] > 0).sum() >= 200
    nctx.set_vocabulary(vocab)
    nctx.detect_batch(imgs)
    words1 = [nctx.words(i) for i in range(5)]
    for w1, w in zip(words1, want):
        assert np.array_equal(w1, w[:, 0])
    P = hesaff_amd.embedding_projection(5)
    desc = np.concatenate([k["desc"] for _, k in plain])
    tau, _ = E.thresholds(P, desc, np.concatenate(words1)[:, 0], 300)
    return imgs, plain, vocab, want, words1, P, tau


def _check_images(nctx, results, e2e, R, what):
    imgs, plain, vocab, want, words1 = e2e[:5]
    for i, ((_, keys), (nh, pk)) in enumerate(zip(results, plain)):
        assert keys.tobytes() == pk.tobytes(), "%s: keys of image %d" % (what, i)
        got = nctx.neighbours(i)
        assert got.shape == (E2E_KEYS[i], R, 2)
        _same(got, want[i][:, :R], "%s: image %d" % (what, i))
        assert nctx.words(i).tobytes() == words1[i].tobytes(), "%s: words of image %d" % (what, i)
    for bad in (len(imgs), -1):
        with pytest.raises(hesaff_amd.HesaffError):
            nctx.neighbours(bad)


@pytest.mark.gpu
@pytest.mark.parametrize("R", (3, 8))
def test_end_to_end_host_entry_points(nctx, e2e, R):
    """five images of two sizes interleaved, max_batch = 2: neighbours(i) is the reference on the keys of image i through every host
    entry point; words(i) is byte for byte what R = 1 gives; the image without keys has count 0 and a NULL pointer"""
    imgs, plain, vocab = e2e[:3]
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(R)
    _check_images(nctx, nctx.detect_batch(imgs), e2e, R, "detect_batch")
    p = ctypes.c_void_p(1); n = ctypes.c_int(-1); r = ctypes.c_int(-1)
    assert nctx.L.hesaff_get_neighbours(nctx.h, 3, ctypes.byref(p), ctypes.byref(n), ctypes.byref(r)) == 0
    assert n.value == 0 and p.value is None and r.value == R
    regions = nctx.detect_regions(imgs)
    _check_images(nctx, [(len(g), k) for g, k in regions], e2e, R, "detect_regions")
    _check_images(nctx, nctx.detect_batch_f32([im.astype(np.float32) for im in imgs]), e2e, R, "detect_batch_f32")
    shapes = [g[g["outcome"] >= 1] for g, _ in regions]
    described = nctx.describe_regions(imgs, shapes, FROM_SHAPES)
    _check_images(nctx, [(len(g), k) for g, k in described], e2e, R, "describe_regions")
    seen = {}

    def sink(indices, out):
        for i, (nh, keys) in zip(indices, out):
            seen[i] = nctx.neighbours(i)
        return 0
    nctx.detect_batch_cb(imgs, sink)
    assert sorted(seen) == [0, 1, 2, 3, 4]
    for i in range(5):
        _same(seen[i], e2e[3][i][:, :R], "sink: image %d" % i)
    with pytest.raises(hesaff_amd.HesaffError):
        nctx.neighbours(0)


@pytest.mark.gpu
def test_end_to_end_device_resident(e2e):
    import torch
    from tests.test_gpu_parity import _device_keys
    imgs, plain, vocab, want = e2e[:4]
    img = imgs[0]
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_vocabulary(vocab)
        c.set_vocabulary_neighbours(3)
        with pytest.raises(hesaff_amd.HesaffError):
            c.neighbours_device()
        t = torch.from_numpy(np.stack([img] * 3)).cuda()
        torch.cuda.synchronize()
        ch, cd, dkeys, total = c.detect_batch_device(t.data_ptr(), 3, img.shape[1], img.shape[0])
        assert cd.tolist() == [221] * 3 and total == 663
        keys = _device_keys(dkeys, total)
        ptr, rows, r = c.neighbours_device()
        wptr, wrows = c.words_device()
        assert rows == total and r == 3 and wrows == total
        got = torch.empty((total, 3, 2), dtype=torch.int32, device="cuda")
        gotw = torch.empty((total, 2), dtype=torch.int32, device="cuda")
        assert hip.hipMemcpy(ctypes.c_void_p(got.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(total * 24), 3) == 0
        assert hip.hipMemcpy(ctypes.c_void_p(gotw.data_ptr()), ctypes.c_void_p(wptr), ctypes.c_size_t(total * 8), 3) == 0
        got, gotw = got.cpu().numpy(), gotw.cpu().numpy()
        for b in range(3):
            assert keys[221 * b:221 * (b + 1)].tobytes() == plain[0][1].tobytes()
            _same(got[221 * b:221 * (b + 1)], want[0][:, :3], "device-resident, image %d" % b)
        assert np.array_equal(gotw, got[:, 0])
        with pytest.raises(hesaff_amd.HesaffError):
            c.neighbours(0)   # the last call was not a host call


@pytest.mark.gpu
def test_end_to_end_signatures_per_rank(nctx, e2e):
    """with an embedding: signatures(i) is rank 0's, as without neighbours; a (key, rank) pair's signature is the reference's under
    that rank's word, through the stage operator on the neighbours' column"""
    imgs, plain, vocab, want, words1, P, tau = e2e
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(3)
    nctx.set_embedding(P, tau)
    try:
        res = nctx.detect_batch(imgs)
        differ = 0
        for i, (_, keys) in enumerate(res):
            nb = nctx.neighbours(i)
            _same(nb, want[i][:, :3], "image %d" % i)
            assert np.array_equal(nctx.signatures(i), E.signatures(P, tau, keys["desc"], nb[:, 0, 0]))
            per_rank = [nctx.embed(keys["desc"], np.ascontiguousarray(nb[:, r])) for r in range(3)]
            for r in range(3):
                assert np.array_equal(per_rank[r], E.signatures(P, tau, keys["desc"], nb[:, r, 0])), (i, r)
            differ += int((per_rank[0] != per_rank[1]).sum()) if len(keys) else 0
        assert differ > 300   # the rank's word matters
    finally:
        nctx.set_embedding(None)


# ---------------------------------------------------------------- files, CLI, C++

def _copies(tmp_path):
    paths = []
    for j, n in enumerate(E2E_IMAGES):
        paths.append(str(tmp_path / ("%d_%s.pgm" % (j, n))))
        shutil.copyfile(os.path.join(GOLD, n + ".pgm"), paths[-1])
    return paths


def _key_rows(keys, mr, tmp_path):
    """the five floats of every key as the words file holds them, a WORDS_ROW_DTYPE row per key (word 0)"""
    ref = str(tmp_path / "ref.bin")
    hesaff_amd.write_bin(ref, keys, mr)
    b = hesaff_amd.read_bin(ref)
    rows = np.zeros(len(b), hesaff_amd.WORDS_ROW_DTYPE)
    for f in ("x", "y", "a", "b", "c"):
        rows[f] = b[f]
    return rows


def _words_bytes(rows, K):
    import struct
    return b"HESAFFW1" + struct.pack("<II", K, len(rows)) + rows.tobytes()


def _expected_files(e2e, R, tmp_path, with_sigs):
    imgs, plain, vocab, want, words1, P, tau = e2e
    mr = hesaff_amd.default_params().mrSize
    out = []
    for i, (_, keys) in enumerate(plain):
        nb = want[i][:, :R]
        rows = _key_rows(keys, mr, tmp_path)
        if with_sigs:
            sg = np.stack([E.signatures(P, tau, keys["desc"], nb[:, r, 0]) for r in range(R)], axis=1) if len(keys) else np.zeros((0, R), np.uint64)
            out.append(hesaff_amd.expand_rows(rows, nb, sg))
        else:
            out.append((hesaff_amd.expand_rows(rows, nb), None))
    return out


@pytest.mark.gpu
def test_process_files_writes_a_row_per_key_and_rank(nctx, e2e, tmp_path):
    imgs, plain, vocab, want, words1, P, tau = e2e
    paths = _copies(tmp_path)
    nctx.set_vocabulary(vocab)
    try:
        # R = 1: the parent's files
        nctx.set_vocabulary_neighbours(1)
        nctx.set_output_format(OUT_WORDS)
        outs1 = [str(tmp_path / ("one%d.words" % i)) for i in range(5)]
        st = nctx.process_files(paths, outs1)
        one = _expected_files(e2e, 1, tmp_path, False)
        for i, o in enumerate(outs1):
            assert st[i][0] == 0 and open(o, "rb").read() == _words_bytes(one[i][0], 300)
            assert len(one[i][0]) == E2E_KEYS[i] and not os.path.exists(o[:-6] + ".sigs")
        # R = 3, no embedding
        nctx.set_vocabulary_neighbours(3)
        nctx.set_output_format(OUT_BIN | OUT_WORDS)
        st = nctx.process_files(paths)
        three = _expected_files(e2e, 3, tmp_path, False)
        for i, p in enumerate(paths):
            assert st[i][0] == 0 and st[i][3] == E2E_KEYS[i], (p, st[i])
            assert len(three[i][0]) == 3 * E2E_KEYS[i]
            assert open(p + ".hesaff.words", "rb").read() == _words_bytes(three[i][0], 300), p
            assert not os.path.exists(p + ".hesaff.sigs")
            vs, rows = hesaff_amd.read_words(p + ".hesaff.words")
            assert vs == 300 and np.array_equal(rows, three[i][0])
        # R = 3 with an embedding: the signatures file row for row
        nctx.set_embedding(P, tau)
        nctx.set_output_format(OUT_WORDS)
        outs = [str(tmp_path / ("emb%d.words" % i)) for i in range(5)]
        st = nctx.process_files(paths, outs)
        emb = _expected_files(e2e, 3, tmp_path, True)
        for i, o in enumerate(outs):
            assert st[i][0] == 0 and open(o, "rb").read() == _words_bytes(emb[i][0], 300)
            assert np.array_equal(hesaff_amd.read_signatures(o[:-6] + ".sigs"), emb[i][1]), o
        # back to R = 1 with the embedding: the parent's files again
        nctx.set_vocabulary_neighbours(1)
        outs = [str(tmp_path / ("back%d.words" % i)) for i in range(5)]
        st = nctx.process_files(paths, outs)
        for i, o in enumerate(outs):
            assert st[i][0] == 0 and open(o, "rb").read() == _words_bytes(one[i][0], 300)
            assert np.array_equal(hesaff_amd.read_signatures(o[:-6] + ".sigs"), E.signatures(P, tau, plain[i][1]["desc"], words1[i][:, 0]))
    finally:
        nctx.set_embedding(None)
        nctx.set_output_format(1)
        nctx.set_vocabulary_neighbours(1)


@pytest.mark.gpu
def test_process_files_leaves_out_the_ranks_a_small_vocabulary_lacks(nctx, e2e, tmp_path):
    """K = 2 < R = 3, with an embedding: two rows per key, no row for the absent rank, the signatures row for row"""
    imgs, plain = e2e[:2]
    vocab = V.family("uniform", 2, seed=3)
    P = hesaff_amd.embedding_projection(6)
    tau = np.arange(128, dtype=np.int32).reshape(2, 64) * 1000 + 300000
    keys = plain[1][1]
    nb = N.neighbours(keys["desc"], vocab, 3)
    assert (nb[:, 2, 0] == -1).all() and (nb[:, :2, 0] >= 0).all()
    src = str(tmp_path / "img.pgm")
    shutil.copyfile(os.path.join(GOLD, "band_96x96.pgm"), src)
    nctx.set_vocabulary(vocab)
    nctx.set_vocabulary_neighbours(3)
    nctx.set_embedding(P, tau)
    try:
        nctx.set_output_format(OUT_WORDS)
        st = nctx.process_files([src])
        assert st[0][0] == 0 and st[0][3] == 74
        sg = np.stack([E.signatures(P, tau, keys["desc"], np.maximum(nb[:, r, 0], 0)) for r in range(3)], axis=1)
        rows, sigs = hesaff_amd.expand_rows(_key_rows(keys, hesaff_amd.default_params().mrSize, tmp_path), nb, sg)
        assert len(rows) == 148
        assert open(src + ".hesaff.words", "rb").read() == _words_bytes(rows, 2)
        assert np.array_equal(hesaff_amd.read_signatures(src + ".hesaff.sigs"), sigs)
    finally:
        nctx.set_embedding(None)
        nctx.set_output_format(1)
        nctx.set_vocabulary_neighbours(1)


def _bits(a):
    return np.asarray(a, np.float64).view(np.uint64)


@pytest.mark.gpu
def test_cli_neighbours_files_and_queries(e2e, tmp_path):
    """hesaff --neighbours 3, single image and --batch beside --embedding: the files are expand_rows of the arrays; without the switch
    byte for byte the files of R = 1.  The expanded file of a query image goes through --search --query, --hamming 24 and --verify
    unchanged: the printed scores are the references' on the expanded rows"""
    imgs, plain, vocab, want, words1, P, tau = e2e
    paths = _copies(tmp_path)
    vfile, efile = str(tmp_path / "vocab.bin"), str(tmp_path / "embed.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    hesaff_amd.write_embedding(efile, P, tau)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    one = _expected_files(e2e, 1, tmp_path, True)
    three = _expected_files(e2e, 3, tmp_path, True)
    # the database: R = 1, with signatures
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile, "--embedding", efile, "--words-only"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    db = tmp_path / "db"
    db.mkdir()
    wfiles = []
    for i, p in enumerate(paths):
        assert open(p + ".hesaff.words", "rb").read() == _words_bytes(one[i][0], 300), p
        assert np.array_equal(hesaff_amd.read_signatures(p + ".hesaff.sigs"), one[i][1])
        wfiles.append(str(db / ("%d.hesaff.words" % i)))
        shutil.move(p + ".hesaff.words", wfiles[-1])
        shutil.move(p + ".hesaff.sigs", wfiles[-1][:-6] + ".sigs")
    # the same list with --neighbours 3
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile, "--embedding", efile, "--words-only", "--neighbours", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for i, p in enumerate(paths):
        assert open(p + ".hesaff.words", "rb").read() == _words_bytes(three[i][0], 300), p
        assert np.array_equal(hesaff_amd.read_signatures(p + ".hesaff.sigs"), three[i][1])
    # a single image
    single = str(tmp_path / "single.pgm")
    shutil.copyfile(paths[1], single)
    r = subprocess.run([EXE, single, "--vocabulary", vfile, "--neighbours", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(single + ".hesaff.words", "rb").read() == _words_bytes(three[1][0], 300)
    assert open(single + ".hesaff.sift", "rb").read() == hesaff_amd.format_sift(plain[1][1], hesaff_amd.default_params().mrSize)
    r = subprocess.run([EXE, single, "--vocabulary", vfile], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and open(single + ".hesaff.words", "rb").read() == _words_bytes(one[1][0], 300)
    # image 1's expanded file as the query
    dbl = tmp_path / "db.txt"
    dbl.write_text("\n".join(wfiles) + "\n")
    query = paths[1] + ".hesaff.words"
    iw = [w[:, 0] for w in words1]
    ig = [s for _, s in one]
    ref = I.build(iw, 300)
    qrows, qsigs = three[1]
    qw = qrows["word"].astype(np.int64)
    r = subprocess.run([EXE, "--search", str(dbl), "--query", query, "--top", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    plain_lines = [l.split("\t") for l in r.stdout.strip().split("\n")]
    want_im, want_sc = I.query(ref, qw, 5)[:2]
    assert [l[1] for l in plain_lines] == [wfiles[i] for i in want_im]
    assert np.array_equal(_bits([float(l[2]) for l in plain_lines]), _bits(want_sc))
    r = subprocess.run([EXE, "--search", str(dbl), "--query", query, "--top", "5", "--hamming", "24"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = [l.split("\t") for l in r.stdout.strip().split("\n")]
    want_im, want_sc = E.query(ref, iw, ig, qw, qsigs, 24, 5)[:2]
    assert [l[1] for l in lines] == [wfiles[i] for i in want_im]
    assert np.array_equal(_bits([float(l[2]) for l in lines]), _bits(want_sc))
    assert want_im[0] in (1, 4) and want_sc[0] > 0
    r = subprocess.run([EXE, "--search", str(dbl), "--query", query, "--top", "5", "--verify"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    vlines = [l.split("\t") for l in r.stdout.strip().split("\n")]
    assert len(vlines) == 5 and all(len(l) == 4 for l in vlines)
    assert sorted((l[1], l[2]) for l in vlines) == sorted((l[1], l[2]) for l in plain_lines)   # the plain scores, in verified order
    assert vlines[0][1] in (wfiles[1], wfiles[4]) and int(vlines[0][3]) >= 20


@pytest.mark.gpu
def test_cpp_detector_members(e2e, tmp_path):
    """tests/native/vocabulary_neighbours_keys.cpp: setVocabularyNeighbours, neighbours() and exportWords through hesaff.hpp hold what the
    Python path holds; the cells refusal throws"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, plain, vocab, want = e2e[:4]
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    exe = str(tmp_path / "vocabulary_neighbours_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, os.path.join(ROOT, "tests", "native", "vocabulary_neighbours_keys.cpp"),
                           "-L" + lib_dir, "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    out = str(tmp_path / "cpp.words")
    r = subprocess.run([exe, vfile, os.path.join(GOLD, "band_96x96.pgm"), out, "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "N 74 3 1", lines[0]
    assert lines[1:75] == ["B " + " ".join(str(v) for v in row.reshape(-1)) for row in want[1][:, :3]]
    assert lines[75:] == ["refused cells", "refused 0", "refused 9", "R 3"]
    three = _expected_files(e2e, 3, tmp_path, False)
    assert open(out, "rb").read() == _words_bytes(three[1][0], 300)
