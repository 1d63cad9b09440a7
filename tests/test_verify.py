"""GPU suite of spatial verification (hesaff_verify_matches, include/hesaff_amd.h; kernels_verify.h).  The reference is
tests/verify_ref.py: the definition in numpy float32.  Every comparison is bit for bit - out, hyp as uint32 bit patterns, order, the
pair lists and inl(h) of every hypothesis."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import WORDS_ROW_DTYPE as ROW
from tests import verify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
ARG = -2
F = np.float32
TILE, CHUNK = 256, 1024   # HS_VERIFY_TILE, HS_VERIFY_CHUNK of kernels_verify.h


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def vctx():
    with hesaff_amd.HesaffContext(_params(max_batch=4), device=0) as c:
        yield c


def _u32(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make_rows(rng, n, words, spread=200.0):
    """n live rows: ellipses with axes around 1 / 10 px and a little shear, anywhere in a spread x spread image"""
    rows = np.zeros(n, ROW)
    p = (0.05 + 0.1 * rng.rand(n)).astype(F); r = (0.05 + 0.1 * rng.rand(n)).astype(F); q = (0.04 * (rng.rand(n) - 0.5)).astype(F)
    rows["x"] = (rng.rand(n) * spread).astype(F); rows["y"] = (rng.rand(n) * spread).astype(F)
    rows["a"] = p * p + q * q; rows["b"] = q * r; rows["c"] = r * r
    rows["word"] = np.asarray(words, np.uint32)
    return rows


def moved(rng, rows, noise=2.0, scale=0.1):
    """the same keys seen in another image: shifted by (7, -3), jittered, the shapes scaled a little"""
    out = rows.copy()
    out["x"] = (rows["x"] + F(7) + (noise * rng.randn(len(rows))).astype(F)).astype(F)
    out["y"] = (rows["y"] - F(3) + (noise * rng.randn(len(rows))).astype(F)).astype(F)
    s = (1.0 + scale * (rng.rand(len(rows)) - 0.5)).astype(F)
    for f in "abc":
        out[f] = rows[f] * s
    return out


def make_corr(rng, m, noise=3.0):
    """m correspondences of live frames, float32 [m, 10], the candidate side a jittered copy of the query side"""
    c = np.zeros((m, 10), F)
    c[:, 0:2] = rng.rand(m, 2) * 300
    c[:, 5:7] = c[:, 0:2] + (noise * rng.randn(m, 2)).astype(F)
    for o in (2, 7):
        c[:, o] = 0.5 + rng.rand(m); c[:, o + 1] = 0.3 * (rng.rand(m) - 0.5); c[:, o + 2] = 0.5 + rng.rand(m)
    return c


def check_verify(ctx, q, cands, K, P, tol, what, device=False):
    want_out, want_hyp, want_order, want_lists, want_qinert = R.verify(q, cands, P, tol)
    if device:
        import torch
        flat = np.concatenate(cands) if sum(len(c) for c in cands) else np.zeros(1, ROW)
        tq = torch.from_numpy((q.copy() if len(q) else np.zeros(1, ROW)).view(np.uint8)).cuda()
        tc = torch.from_numpy(flat.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        out, hyp, order = ctx.verify_matches_device(tq.data_ptr(), len(q), tc.data_ptr(), [len(c) for c in cands], K, tol, P)
    else:
        out, hyp, order = ctx.verify_matches(q, cands, K, tol, P)
    assert out.dtype == np.int32 and hyp.dtype == np.float32 and order.dtype == np.int32
    bad = np.nonzero((out != want_out).any(axis=1))[0]
    assert len(bad) == 0, (what, "out", bad[:4].tolist(), out[bad[:4]].tolist(), want_out[bad[:4]].tolist())
    assert np.array_equal(_u32(hyp), _u32(want_hyp)), (what, "hyp")
    assert not np.isnan(hyp).any(), (what, "NaN in hyp")
    assert order.tolist() == want_order.tolist(), (what, "order")
    assert ctx.verify_query_inert == want_qinert, (what, "query inert")
    for r in sorted(set([0, len(cands) - 1] + np.argsort(-want_out[:, 1])[:3].tolist())):
        got = ctx.verify_pairs(r)
        assert got.shape == want_lists[r].shape and np.array_equal(got, want_lists[r]), (what, "pairs of candidate", r)
    return out, hyp, order


# ---------------------------------------------------------------- the hypothesis kernel alone

@pytest.mark.gpu
@pytest.mark.parametrize("m", [1, 2, 63, 64, 65, TILE - 1, TILE, TILE + 1, CHUNK - 1, CHUNK, CHUNK + 1, 4095, 4096])
def test_hypothesis_kernel_sizes(vctx, m):
    """random live frames through hesaff_stage_verify_pairs: inl(h) of every h and the best h, below, at and above a wavefront, the
    hypothesis tile (256) and the LDS chunk (1024), and at the cap"""
    corr = make_corr(np.random.RandomState(m), m)
    want_inl, want_best, _ = R.inliers(corr, 5.0)
    inl, best = vctx.stage_verify_pairs(corr, 5.0)
    assert np.array_equal(inl, want_inl), np.nonzero(inl != want_inl)[0][:8].tolist()
    assert best == want_best
    if m >= 64:
        assert 1 < want_inl.max() < m   # the tolerance divides the correspondences


@pytest.mark.gpu
def test_hypothesis_kernel_without_correspondences(vctx):
    inl, best = vctx.stage_verify_pairs(np.zeros((0, 10), F), 5.0)
    assert len(inl) == 0 and best == -1
    L, h = vctx.L, vctx.h
    c = make_corr(np.random.RandomState(1), 4)
    b = ctypes.c_int32(7)
    assert L.hesaff_stage_verify_pairs(h, 4097, c.ctypes.data, 5.0, None, ctypes.byref(b)) == ARG
    assert L.hesaff_stage_verify_pairs(h, -1, c.ctypes.data, 5.0, None, ctypes.byref(b)) == ARG
    assert L.hesaff_stage_verify_pairs(h, 4, None, 5.0, None, ctypes.byref(b)) == ARG
    for tol in (0.0, -1.0, float("nan"), float("inf"), 2.0 ** 20 * 1.5):
        assert L.hesaff_stage_verify_pairs(h, 4, c.ctypes.data, tol, None, ctypes.byref(b)) == ARG, tol
    assert b.value == 7
    assert L.hesaff_stage_verify_pairs(h, 4, c.ctypes.data, 2.0 ** 20, None, ctypes.byref(b)) == 0 and b.value == 0


def _identity_corr(points):
    c = np.zeros((len(points), 10), F)
    c[:, [2, 4, 7, 9]] = 1.0
    for k, (xq, yq, xd, yd) in enumerate(points):
        c[k, 0], c[k, 1], c[k, 5], c[k, 6] = xq, yq, xd, yd
    return c


@pytest.mark.gpu
def test_threshold_equality(vctx):
    """identity frames, integer coordinates: an error of exactly (3, 4) is an inlier at tol = 5 and none at the float below 5"""
    c = _identity_corr([(0, 0, 0, 0), (10, 0, 13, 4)])
    below = float(np.nextafter(F(5), F(0)))
    for tol, want in ((5.0, [2, 2]), (below, [1, 1])):
        inl, best = vctx.stage_verify_pairs(c, tol)
        assert inl.tolist() == want == R.inliers(c, tol)[0].tolist() and best == 0, tol   # equal counts: the lower h wins
    rows_q = np.zeros(2, ROW); rows_d = np.zeros(2, ROW)
    for rows, (k0, k1) in ((rows_q, ((0, 0), (10, 0))), (rows_d, ((0, 0), (13, 4)))):
        rows["x"] = [k0[0], k1[0]]; rows["y"] = [k0[1], k1[1]]; rows["a"] = 1; rows["c"] = 1; rows["word"] = [0, 1]
    for tol, want in ((5.0, 2), (below, 1)):
        out, hyp, order = check_verify(vctx, rows_q, [rows_d], 2, 1, tol, "threshold %r" % tol)
        assert out[0].tolist() == [want, 2, 2, 0, 0, 0] and hyp[0].tolist() == [1.0, 0.0, 1.0]


@pytest.mark.gpu
def test_ties(vctx):
    """two hypotheses with equal counts: the lower h; identical candidates at positions 2 and 5 keep their order; candidates without
    inliers rank by position"""
    c = _identity_corr([(0, 0, 50, 50), (1, 0, 0, 0), (2, 0, 1, 0), (100, 100, 150, 150)])   # h = 0 and 3 agree, h = 1 and 2 agree
    inl, best = vctx.stage_verify_pairs(c, 0.5)
    assert inl.tolist() == [2, 2, 2, 2] and best == 0
    rng = np.random.RandomState(9)
    q = make_rows(rng, 40, np.arange(40))
    same = moved(rng, q)
    other = make_rows(rng, 30, np.arange(40, 70))   # shares no word
    part = same[:10].copy()
    cands = [other, part, same, other[:5], np.zeros(0, ROW), same.copy(), other]
    out, hyp, order = check_verify(vctx, q, cands, 70, 1, 6.0, "ties")
    assert out[2].tolist() == out[5].tolist() and out[2, 0] > out[1, 0] > 0
    assert order.tolist() == [2, 5, 1, 0, 3, 4, 6]
    assert (out[[0, 3, 4, 6], :5] == [0, 0, 0, -1, -1]).all() and (hyp[[0, 3, 4, 6]] == 0).all()


@pytest.mark.gpu
def test_extremes(vctx):
    """p and r at 2^-20 against 2^20, coordinates at +-2^20: e2 overflows to +inf, the counts are the reference's, no NaN in hyp"""
    rng = np.random.RandomState(4)
    lo, hi = 2.0 ** -20, 2.0 ** 20
    m = 300
    c = np.zeros((m, 10), F)
    for o in (0, 1, 5, 6):
        c[:, o] = rng.choice([-hi, hi, 0.0, 1.0], m)
    for o in (2, 4, 7, 9):
        c[:, o] = rng.choice([lo, hi, 1.0], m)
    for o in (3, 8):
        c[:, o] = rng.choice([0.0, -(hi - 1), hi - 1, 0.5], m)
    want_inl, want_best, L = R.inliers(c, 2.0 ** 20)
    assert np.isfinite(L).all() and np.abs(L).max() > 2.0 ** 79
    inl, best = vctx.stage_verify_pairs(c, 2.0 ** 20)
    assert np.array_equal(inl, want_inl) and best == want_best and want_inl.min() >= 1
    # the same through rows: a = p^2 + q^2 and c = r^2 are exact for powers of two, and a = 2^40 is still live
    n = 64
    q = np.zeros(n, ROW); d = np.zeros(n, ROW)
    for rows in (q, d):
        p = rng.choice([lo, hi, 1.0], n).astype(F); r = rng.choice([lo, hi, 1.0], n).astype(F)
        rows["x"] = rng.choice([-hi, hi, 0.0], n); rows["y"] = rng.choice([-hi, hi, 0.0], n)
        rows["a"] = p * p; rows["c"] = r * r; rows["word"] = np.arange(n)
    assert R.frames(q)[1].all() and R.frames(d)[1].all()
    for tol in (1.0, 2.0 ** 20):
        out, hyp, order = check_verify(vctx, q, [d, q], n, 1, tol, "extreme rows")
        assert out[1].tolist() == [n, n, n, 0, 0, 0] and hyp[1].tolist() == [1.0, 0.0, 1.0]


# ---------------------------------------------------------------- pair construction

@pytest.mark.gpu
@pytest.mark.parametrize("P", [1, 2, 16])
def test_pairs_at_the_bound(vctx, P):
    """words with tfq * tf equal to P and to P + 1 (in both factorisations the bound has), inert keys on both sides, a candidate
    without keys and one that shares no word"""
    rng = np.random.RandomState(20 + P)
    K = 64
    shapes = []   # (tfq, tf) per word
    for a in range(1, P + 2):
        for b in range(1, P + 2):
            if a * b in (P, P + 1) or (a, b) == (1, 1):
                shapes.append((a, b))
    assert len(shapes) <= K - 4
    qw = np.concatenate([[w] * a for w, (a, b) in enumerate(shapes)] + [[K - 1, K - 2]])
    dw = np.concatenate([[w] * b for w, (a, b) in enumerate(shapes)] + [[K - 1, K - 3]])
    q = make_rows(rng, len(qw), rng.permutation(qw))
    d = make_rows(rng, len(dw), rng.permutation(dw))
    q["c"][q["word"] == K - 1] = -1.0            # inert: word K - 1 pairs with nothing
    d["a"][d["word"] == K - 1] = np.nan
    q2 = q.copy(); q2["x"][np.nonzero(q["word"] != K - 1)[0][0]] = np.inf
    empty = np.zeros(0, ROW)
    nothing = make_rows(rng, 9, np.full(9, K - 4))
    out, hyp, order = check_verify(vctx, q, [d, empty, nothing, moved(rng, q), d[::-1].copy()], K, P, 8.0, "P = %d" % P)
    want_found = sum(a * b for a, b in shapes if a * b <= P)
    assert out[0, 2] == want_found == out[4, 2] and out[0, 5] == 1 and out[1].tolist() == [0, 0, 0, -1, -1, 0] and out[2, 2] == 0
    assert vctx.verify_query_inert == 1
    check_verify(vctx, q2, [d], K, P, 8.0, "P = %d, an infinite x" % P)
    assert vctx.verify_query_inert == 2
    check_verify(vctx, empty, [d, empty], K, P, 8.0, "P = %d, empty query" % P)


@pytest.mark.gpu
@pytest.mark.parametrize("found", [4095, 4096, 4097])
def test_found_around_the_cap(vctx, found):
    """distinct words on both sides: found = n; above 4096 the dropped pair is the last of the (j, i) order"""
    rng = np.random.RandomState(found)
    q = make_rows(rng, found, rng.permutation(found) + 100, spread=2000.0)
    d = moved(rng, q)[rng.permutation(found)]
    out, hyp, order = check_verify(vctx, q, [d], 5000, 1, 6.0, "found %d" % found)
    assert out[0, 2] == found and out[0, 1] == min(found, 4096)
    pairs = vctx.verify_pairs(0)
    assert len(pairs) == min(found, 4096) and pairs[:, 1].tolist() == list(range(len(pairs)))   # j ascending: key 4096 is the one dropped


@pytest.mark.gpu
def test_order_inside_a_word(vctx):
    """tfq = 4, tf = 4, P = 16: sixteen pairs per word in the order (j, then i), whatever the order of arrival in the groups"""
    rng = np.random.RandomState(31)
    q = make_rows(rng, 4000, rng.permutation(np.repeat(np.arange(1000), 4)))
    d = make_rows(rng, 1200, rng.permutation(np.repeat(np.arange(300), 4)))
    out, hyp, order = check_verify(vctx, q, [d], 1000, 16, 6.0, "4 x 4")
    assert out[0, 2] == 4800 and out[0, 1] == 4096
    pairs = vctx.verify_pairs(0)
    assert (np.diff(pairs[:, 1]) >= 0).all() and (np.diff(pairs[:, 0])[np.diff(pairs[:, 1]) == 0] > 0).all()


@pytest.mark.gpu
def test_largest_vocabulary_and_candidate_counts(vctx):
    """word K - 1 at K = 2^20; R = 1 and R = 1024 tiny candidates"""
    rng = np.random.RandomState(41)
    K = 1 << 20
    words = np.array([K - 1, 0, K - 2, 12345, K // 2, 7, 8, 9])
    q = make_rows(rng, 8, words)
    check_verify(vctx, q, [moved(rng, q)], K, 1, 6.0, "R = 1")
    cands = []
    for r in range(1024):
        n = r % 5
        sel = rng.choice(8, n, replace=False)
        c = moved(rng, q[sel]) if n else np.zeros(0, ROW)
        if n and r % 7 == 0:
            c["c"][0] = 0.0   # an inert key
        cands.append(c)
    out, hyp, order = check_verify(vctx, q, cands, K, 2, 6.0, "R = 1024")
    assert sorted(order.tolist()) == list(range(1024)) and out[:, 0].max() >= 2
    with pytest.raises(hesaff_amd.HesaffError):
        vctx.verify_matches(q, cands + [q], K, 6.0, 2)   # R = 1025


@pytest.mark.gpu
def test_one_candidate_of_2_18_keys(vctx):
    rng = np.random.RandomState(43)
    K = 1 << 20
    n = 1 << 18
    d = make_rows(rng, n, rng.randint(0, K, n), spread=4000.0)
    d["a"][rng.choice(n, 100, replace=False)] = np.nan
    sel = np.sort(rng.choice(n, 3000, replace=False))
    q = moved(rng, d[sel], scale=0.0)
    q["word"][:50] = K - 1 - np.arange(50, dtype=np.uint32)
    for P in (1, 3):
        out, hyp, order = check_verify(vctx, q, [d, q[:7]], K, P, 6.0, "2^18 keys, P = %d" % P)
        assert out[0, 5] == 100 and 2000 < out[0, 1] <= 4096 and out[0, 0] > 2000
    with pytest.raises(hesaff_amd.HesaffError):
        vctx.verify_matches(q, [np.concatenate([d, d[:1]])], K, 6.0, 1)   # 2^18 + 1 keys


# ---------------------------------------------------------------- known answers

@pytest.mark.gpu
def test_known_answers(vctx):
    """the query against itself with distinct words: every hypothesis is exactly the identity, inliers == used == nq; and against
    itself moved by an integer offset, coordinates below 2^10, tol = 0.5"""
    rng = np.random.RandomState(51)
    n = 700
    q = make_rows(rng, n, rng.permutation(n))
    q["x"] = rng.randint(0, 900, n); q["y"] = rng.randint(0, 900, n)
    shifted = q.copy()
    shifted["x"] += F(37); shifted["y"] -= F(21)
    out, hyp, order = vctx.verify_matches(q, [q, shifted], n, 0.5, 1)
    assert out[:, :3].tolist() == [[n, n, n]] * 2 and out[:, 3:5].tolist() == [[0, 0]] * 2 and hyp.tolist() == [[1.0, 0.0, 1.0]] * 2
    assert order.tolist() == [0, 1]
    inl, best = vctx.stage_verify_pairs(np.concatenate([R.frames(q)[0], R.frames(shifted)[0]], axis=1), 0.5)
    assert (inl == n).all() and best == 0


@pytest.fixture(scope="module")
def shortlist():
    rng = np.random.RandomState(61)
    K = 500
    q = make_rows(rng, 400, rng.randint(0, K, 400))
    cands = []
    for r in range(9):
        sel = rng.choice(400, 40 * r, replace=False)
        c = np.concatenate([moved(rng, q[sel]), make_rows(rng, 60, rng.randint(0, K, 60))])
        cands.append(c[rng.permutation(len(c))])
    cands[4]["b"][::9] = np.nan
    for c in cands:
        c.setflags(write=False)
    q.setflags(write=False)
    return q, cands, K


@pytest.mark.gpu
def test_candidates_permuted_and_repeated_calls(vctx, shortlist):
    q, cands, K = shortlist
    out, hyp, order = check_verify(vctx, q, cands, K, 3, 6.0, "shortlist")
    assert len(set(out[:, 0].tolist())) > 4
    again = vctx.verify_matches(q, cands, K, 6.0, 3)
    assert again[0].tobytes() == out.tobytes() and again[1].tobytes() == hyp.tobytes() and again[2].tobytes() == order.tobytes()
    perm = np.random.RandomState(3).permutation(len(cands))
    out2, hyp2, order2 = check_verify(vctx, q, [cands[i] for i in perm], K, 3, 6.0, "shortlist, permuted")
    assert out2.tobytes() == out[perm].tobytes() and hyp2.tobytes() == hyp[perm].tobytes()
    assert (np.diff(out[perm[order2], 0]) <= 0).all()


@pytest.mark.gpu
def test_device_form_equals_host_form(vctx, shortlist):
    q, cands, K = shortlist
    host = check_verify(vctx, q, cands, K, 2, 6.0, "host")
    dev = check_verify(vctx, q, cands, K, 2, 6.0, "device", device=True)
    for a, b in zip(host, dev):
        assert a.tobytes() == b.tobytes()
    empty = np.zeros(0, ROW)
    check_verify(vctx, empty, [cands[0], empty], K, 2, 6.0, "device, empty query", device=True)
    check_verify(vctx, q, [empty, empty], K, 2, 6.0, "device, no candidate keys", device=True)


@pytest.mark.gpu
def test_verify_ms_are_event_times(vctx, shortlist):
    q, cands, K = shortlist
    vctx.set_profiling(1)
    try:
        vctx.verify_matches(q, cands, K, 6.0, 2)
        ms = vctx.verify_ms
        print("verify_ms (pairs, hypotheses) for 9 candidates:", ms)
        assert all(0.0 < v < 1000.0 for v in ms)
    finally:
        vctx.set_profiling(0)
    vctx.verify_matches(q, cands, K, 6.0, 2)
    assert vctx.verify_ms == (0.0, 0.0)


# ---------------------------------------------------------------- end to end

E2E_CROP = (8, 12, 112, 152)       # rows 8..111, columns 12..151 of band_160x120: a shifted crop of the query
E2E_KEYS = [221, 128, 74, 71]      # band_160x120, its crop, band_96x96, band_131x77
E2E_TOL = 5.0


@pytest.fixture(scope="module")
def e2e(vctx, tmp_path_factory):
    """the query image, a shifted crop of it and two unrelated images, detected under a vocabulary made of the query's own 221
    descriptors (all distinct: a copy of a key finds its own word), written as words files and read back as rows"""
    d = tmp_path_factory.mktemp("verify_e2e")
    img = hesaff_amd.read_pnm(os.path.join(GOLD, "band_160x120.pgm"))
    y0, x0, y1, x1 = E2E_CROP
    crop = np.ascontiguousarray(img[y0:y1, x0:x1])
    imgs = [img, crop, hesaff_amd.read_pnm(os.path.join(GOLD, "band_96x96.pgm")), hesaff_amd.read_pnm(os.path.join(GOLD, "band_131x77.pgm"))]
    image_paths = [os.path.join(GOLD, "band_160x120.pgm"), str(d / "crop.pgm"), os.path.join(GOLD, "band_96x96.pgm"), os.path.join(GOLD, "band_131x77.pgm")]
    with open(image_paths[1], "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (crop.shape[1], crop.shape[0]) + crop.tobytes())
    plain = vctx.detect_batch(imgs)
    vocab = np.ascontiguousarray(plain[0][1]["desc"])
    assert len(np.unique(vocab, axis=0)) == len(vocab) == 221
    vctx.set_vocabulary(vocab)
    try:
        res = vctx.detect_batch(imgs)
        words = [vctx.words(i) for i in range(len(imgs))]
    finally:
        vctx.set_vocabulary(None)
    assert [len(k) for _, k in res] == E2E_KEYS
    paths, rows = [], []
    for j, ((_, keys), w) in enumerate(zip(res, words)):
        paths.append(str(d / ("%d.pgm.hesaff.words" % j)))
        hesaff_amd.write_words(paths[-1], keys, w, vctx.params.mrSize, len(vocab))
        vs, r = hesaff_amd.read_words(paths[-1])
        assert vs == 221
        r.setflags(write=False)
        rows.append(r)
    return imgs, image_paths, plain, res, words, vocab, paths, rows


def _check_e2e(out, shortlist):
    """the ordering the numpy reference gives on the CPU oracle's keys: the query itself, its crop, the rest"""
    by_image = {int(i): out[r] for r, i in enumerate(shortlist)}
    assert by_image[0][0] == by_image[0][1] == 221          # the query against itself: every correspondence agrees
    assert by_image[1][0] > max(by_image[2][0], by_image[3][0])   # the crop above the unrelated images


@pytest.mark.gpu
def test_end_to_end_python(vctx, e2e):
    imgs, image_paths, plain, res, words, vocab, paths, rows = e2e
    vctx.build_index(words, 221)
    try:
        shortlist, scores = vctx.query_index(words[0], 4)
        assert sorted(shortlist.tolist()) == [0, 1, 2, 3] and shortlist[0] == 0
        out, hyp, order = check_verify(vctx, rows[0], [rows[i] for i in shortlist], 221, 1, E2E_TOL, "golden images")
        print("end to end (inliers, used, found) by shortlist position:", shortlist.tolist(), out[:, :3].tolist())
        _check_e2e(out, shortlist)
        assert [int(shortlist[r]) for r in order[:2]] == [0, 1]
        assert vctx.index_info[0] == 4   # the index is as it was
    finally:
        vctx.clear_index()


@pytest.mark.gpu
def test_end_to_end_cli_search_verify(vctx, e2e, tmp_path):
    """hesaff --search ... --verify prints rank, path, score and inliers in verified order; without --verify the three columns of the
    plain search, byte for byte what it printed before"""
    imgs, image_paths, plain, res, words, vocab, paths, rows = e2e
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    base = [EXE, "--search", str(lst), "--query", paths[0], "--top", "4"]
    r0 = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0, r0.stderr
    plain_lines = [l.split("\t") for l in r0.stdout.strip().split("\n")]
    assert all(len(l) == 3 for l in plain_lines) and len(plain_lines) == 4
    shortlist = [paths.index(l[1]) for l in plain_lines]
    want_out, _, want_order, _, _ = R.verify(rows[0], [rows[i] for i in shortlist], 1, E2E_TOL)
    for extra in (["--verify", "--tolerance", "5"], ["--tolerance", "5.0", "--pairs", "1", "--verify"]):
        r = subprocess.run(base + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        lines = [l.split("\t") for l in r.stdout.strip().split("\n")]
        assert [int(l[0]) for l in lines] == [1, 2, 3, 4]
        assert [l[1] for l in lines] == [paths[shortlist[c]] for c in want_order]
        assert [l[2] for l in lines] == [plain_lines[c][2] for c in want_order]
        assert [int(l[3]) for l in lines] == [int(want_out[c, 0]) for c in want_order]
    _check_e2e(want_out, shortlist)
    # the default tolerance and more pairs per word: still the reference's
    r = subprocess.run(base + ["--verify", "--pairs", "4"], capture_output=True, text=True, timeout=600)
    want_out, _, want_order, _, _ = R.verify(rows[0], [rows[i] for i in shortlist], 4, 8.0)
    assert r.returncode == 0 and [int(l.split("\t")[3]) for l in r.stdout.strip().split("\n")] == [int(want_out[c, 0]) for c in want_order]


@pytest.mark.gpu
def test_end_to_end_cpp_member(e2e, tmp_path):
    """tests/native/verify_keys.cpp: verifyMatches through hesaff.hpp holds what the Python path holds"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, image_paths, plain, res, words, vocab, paths, rows = e2e
    exe = str(tmp_path / "verify_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "verify_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    r = subprocess.run([exe, vfile, "5", "1", str(tmp_path), image_paths[0]] + image_paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out, _, order, _, _ = R.verify(rows[0], rows, 1, E2E_TOL)
    assert r.stdout.strip().split("\n") == ["V %d %d %d %d %d %d" % (j + 1, c, out[c, 0], out[c, 1], out[c, 2], out[c, 5]) for j, c in enumerate(order)] + ["C refused"]
    _check_e2e(out, [0, 1, 2, 3])


# ---------------------------------------------------------------- refusals and isolation

@pytest.mark.gpu
def test_refusals_leave_the_context_its_index_and_its_vocabulary_alone(e2e):
    import torch
    imgs, image_paths, plain, res, words, vocab, paths, rows = e2e
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        L, h = c.L, c.h
        out = np.full((3, 6), 7, np.int32); hyp = np.full((3, 3), 7, F); order = np.full(3, 7, np.int32)
        op, hp, dp = out.ctypes.data, hyp.ctypes.data, order.ctypes.data
        pp, n = ctypes.c_void_p(7), ctypes.c_int(7)
        # no verify call yet: the getters are refused
        assert L.hesaff_verify_get_pairs(h, 0, ctypes.byref(pp), ctypes.byref(n)) == ARG and L.hesaff_verify_get_query_inert(h, ctypes.byref(n)) == ARG
        with pytest.raises(hesaff_amd.HesaffError):
            c.verify_pairs(0)
        c.set_vocabulary(vocab)
        c.build_index(words, 221)
        want = c.verify_matches(rows[0], rows[:3], 221, E2E_TOL)
        want_pairs = c.verify_pairs(1)

        def still_works(what):
            assert c.vocabulary_size == 221 and c.index_info[0] == 4, what
            (nh, keys), = c.detect_batch(imgs[2:3])
            assert keys.tobytes() == res[2][1].tobytes() and np.array_equal(c.words(0), words[2]), what
            im, sc = c.query_index(words[0], 4)
            assert im[0] == 0, what
            assert np.array_equal(c.verify_pairs(1), want_pairs) and c.verify_query_inert == 0, what   # the last call's result is still there
            got = c.verify_matches(rows[0], rows[:3], 221, E2E_TOL)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want)), what
        still_works("before")
        q = rows[0].copy(); flat = np.concatenate(rows[:3]); counts = np.array([len(r) for r in rows[:3]], np.int32)
        tq = torch.from_numpy(q.view(np.uint8)).cuda(); tc = torch.from_numpy(flat.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        host = lambda nq=len(q), qp=q.ctypes.data, R=3, cp=counts.ctypes.data, rp=flat.ctypes.data, K=221, P=1, tol=5.0: \
            L.hesaff_verify_matches(h, nq, qp, R, cp, rp, K, P, tol, op, hp, dp)
        dev = lambda nq=len(q), qp=tq.data_ptr(), R=3, cp=counts.ctypes.data, rp=tc.data_ptr(), K=221, P=1, tol=5.0: \
            L.hesaff_verify_matches_device(h, nq, ctypes.c_void_p(qp), R, cp, ctypes.c_void_p(rp), K, P, tol, op, hp, dp)
        assert host() == 0 and dev() == 0 and out.tobytes() == want[0].tobytes()
        out[:] = 7; hyp[:] = 7; order[:] = 7
        for f in (host, dev):
            assert f(qp=None) == ARG and f(cp=None) == ARG and f(rp=None) == ARG
            for R_, K_ in ((0, 221), (-1, 221), (1025, 221), (3, 0), (3, -1), (3, (1 << 20) + 1)):
                big = np.zeros(max(R_, 3), np.int32)
                assert f(R=R_, cp=big.ctypes.data, K=K_) == ARG, (R_, K_)
            for bad in ([2, -1, 1], [2, (1 << 18) + 1, 1]):
                assert f(cp=np.array(bad, np.int32).ctypes.data) == ARG, bad
            assert f(nq=-1) == ARG and f(nq=(1 << 18) + 1) == ARG
            for P_ in (0, -1, 17):
                assert f(P=P_) == ARG
            for tol in (0.0, -5.0, float("nan"), float("inf"), 2.0 ** 20 + 1):
                assert f(tol=tol) == ARG, tol
            assert f(K=220) == ARG   # a word >= K: the host form finds it while staging, the device form by its check kernel
        assert host(R=1024, cp=np.full(1024, (1 << 18), np.int32).ctypes.data, nq=0, qp=None, rp=None) == ARG   # 2^28 keys and no rows
        assert dev(qp=tq.data_ptr() + 2) == ARG and dev(rp=tc.data_ptr() + 1) == ARG
        bad = flat.copy(); bad["word"][len(bad) - 1] = 221
        tb = torch.from_numpy(bad.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        assert host(rp=bad.ctypes.data) == ARG and dev(rp=tb.data_ptr()) == ARG
        bq = q.copy(); bq["word"][0] = 0xffffffff
        tbq = torch.from_numpy(bq.view(np.uint8)).cuda()
        torch.cuda.synchronize()
        assert host(qp=bq.ctypes.data) == ARG and dev(qp=tbq.data_ptr()) == ARG
        assert L.hesaff_verify_get_pairs(h, 3, ctypes.byref(pp), ctypes.byref(n)) == ARG and L.hesaff_verify_get_pairs(h, -1, ctypes.byref(pp), ctypes.byref(n)) == ARG
        assert L.hesaff_verify_get_pairs(h, 0, None, ctypes.byref(n)) == ARG and L.hesaff_verify_get_query_inert(h, None) == ARG
        ms = ctypes.c_float(7)
        assert L.hesaff_get_verify_ms(h, None, ctypes.byref(ms)) == ARG and L.hesaff_get_verify_ms(h, ctypes.byref(ms), None) == ARG
        assert (out == 7).all() and (hyp == 7).all() and (order == 7).all() and pp.value == 7 and n.value == 7 and ms.value == 7.0
        with pytest.raises(ValueError):
            c.verify_matches(np.zeros(3, np.int32), rows[:3], 221, 5.0)
        still_works("after the refusals")
        # each of out, hyp and order may be NULL
        assert L.hesaff_verify_matches(h, len(q), q.ctypes.data, 3, counts.ctypes.data, flat.ctypes.data, 221, 1, 5.0, None, None, None) == 0
        assert L.hesaff_verify_matches(h, len(q), q.ctypes.data, 3, counts.ctypes.data, flat.ctypes.data, 221, 1, 5.0, None, None, dp) == 0
        assert order.tolist() == want[2].tolist() and (out == 7).all()


@pytest.mark.gpu
def test_detection_is_untouched_by_a_verify_call(vctx, e2e):
    """the keys of a detecting call after a verify call are byte-equal to those before it"""
    imgs, image_paths, plain, res, words, vocab, paths, rows = e2e
    vctx.verify_matches(rows[0], rows, 221, E2E_TOL, 2)
    after = vctx.detect_batch(imgs)
    for (na, a), (nb, b) in zip(after, plain):
        assert na == nb and a.tobytes() == b.tobytes()
    assert len(vctx.verify_pairs(0)) == 221   # and the result of the verify call survives the detecting call
