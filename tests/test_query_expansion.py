"""GPU suite of query expansion (hesaff_expand_query, include/hesaff_amd.h; kernels_expand.h).  The reference is
tests/expand_ref.py: the definition in numpy float32.  Every comparison is bit for bit - the rows as bytes, the words, the
signatures, n_out and info."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import WORDS_ROW_DTYPE as ROW
from tests import expand_ref as X
from tests import verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
ARG = -2
F = np.float32
BIG = (-2.0 ** 20, -2.0 ** 20, 2.0 ** 20, 2.0 ** 20)
K = 1000


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def xctx():
    with hesaff_amd.HesaffContext(_params(max_batch=4), device=0) as c:
        yield c


def make_rows(rng, n, spread=200.0, k=K):
    """n live rows: ellipses with axes around 1 px and a little shear, anywhere in a spread x spread image"""
    rows = np.zeros(n, ROW)
    p = (0.5 + rng.rand(n)).astype(F); r = (0.5 + rng.rand(n)).astype(F); q = (0.4 * (rng.rand(n) - 0.5)).astype(F)
    rows["x"] = (rng.rand(n) * spread).astype(F); rows["y"] = (rng.rand(n) * spread).astype(F)
    rows["a"] = p * p + q * q; rows["b"] = q * r; rows["c"] = r * r
    rows["word"] = rng.randint(0, k, n)
    return rows


def unit_rows(xs, ys, words=None):
    """live rows with the unit circle for an ellipse at the given coordinates"""
    rows = np.zeros(len(xs), ROW)
    rows["x"] = np.asarray(xs, F); rows["y"] = np.asarray(ys, F); rows["a"] = 1; rows["c"] = 1
    rows["word"] = np.arange(len(xs)) % K if words is None else words
    return rows


def hypotheses(entries):
    """[(inliers, query_key, candidate_key, (L11, L21, L22))] -> (out int32 [R, 6], hyp float32 [R, 3])"""
    out = np.array([[e[0], max(e[0], 0), max(e[0], 0), e[1], e[2], 0] for e in entries], np.int32).reshape(-1, 6)
    hyp = np.array([e[3] for e in entries], F).reshape(-1, 3)
    return out, hyp


def expand_device(ctx, q, cands, out, hyp, min_inliers, max_images, roi, max_rows, qsigs, csigs, k):
    """the device form on torch buffers; the outputs lie in buffers filled with 0x7b, of which nothing past n_out may change"""
    import torch
    flat = np.concatenate(cands) if sum(len(c) for c in cands) else np.zeros(0, ROW)
    up = lambda a: torch.from_numpy(np.frombuffer((a.tobytes() if len(a) else b"") + b"\0" * 64, np.uint8).copy()).cuda()
    tq, tc = up(q), up(flat)
    cap = min(max_rows, len(q) + len(flat)) + 8
    t_rows = torch.full((cap * 24,), 0x7b, dtype=torch.uint8, device="cuda")
    t_words = torch.full((cap * 4,), 0x7b, dtype=torch.uint8, device="cuda")
    tqs = tcs = t_sigs = None
    if qsigs is not None:
        tqs, tcs = up(qsigs), up(np.concatenate(csigs) if len(flat) else np.zeros(0, np.uint64))
        t_sigs = torch.full((cap * 8,), 0x7b, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ptr = lambda t: None if t is None else t.data_ptr()
    n, info = ctx.expand_query_device(tq.data_ptr() if len(q) else None, len(q), tc.data_ptr() if len(flat) else None, [len(c) for c in cands], out, hyp, k,
                                      min_inliers, roi, t_rows.data_ptr(), t_words.data_ptr(), max_images=max_images, max_rows=max_rows,
                                      query_sigs_ptr=ptr(tqs) if len(q) else None, candidate_sigs_ptr=ptr(tcs) if len(flat) else None, sigs_out_ptr=ptr(t_sigs))
    torch.cuda.synchronize()
    b_rows, b_words = t_rows.cpu().numpy(), t_words.cpu().numpy()
    assert (b_rows[n * 24:] == 0x7b).all() and (b_words[n * 4:] == 0x7b).all(), "written past n_out"
    rows = np.frombuffer(b_rows[:n * 24].tobytes(), ROW)
    words = np.frombuffer(b_words[:n * 4].tobytes(), np.int32)
    sigs = None
    if t_sigs is not None:
        b_sigs = t_sigs.cpu().numpy()
        assert (b_sigs[n * 8:] == 0x7b).all(), "signatures written past n_out"
        sigs = np.frombuffer(b_sigs[:n * 8].tobytes(), np.uint64)
    return rows, words, sigs, info


def check_expand(ctx, q, cands, out, hyp, min_inliers, what, max_images=1024, roi=BIG, max_rows=2 ** 18, qsigs=None, csigs=None, forms=("host", "device"), k=K):
    want_rows, want_words, want_sigs, want_info = X.expand(q, cands, out, hyp, min_inliers, max_images, roi, max_rows, qsigs, csigs)
    for form in forms:
        if form == "host":
            got = ctx.expand_query(q, cands, out, hyp, k, min_inliers, max_images=max_images, roi=roi, max_rows=max_rows, query_signatures=qsigs,
                                   candidate_signatures=csigs)
            rows, info, sigs = got if qsigs is not None else got + (None,)
            words = None
        else:
            rows, words, sigs, info = expand_device(ctx, q, cands, out, hyp, min_inliers, max_images, roi, max_rows, qsigs, csigs, k)
        assert len(rows) == len(want_rows), (what, form, "n_out", len(rows), len(want_rows))
        assert info.tolist() == want_info.tolist(), (what, form, "info", info[(info != want_info).any(axis=1)][:4].tolist())
        bad = np.nonzero(rows.view(np.uint8).reshape(-1, 24) != want_rows.view(np.uint8).reshape(-1, 24))[0]
        assert len(bad) == 0, (what, form, "row", int(bad[0]), rows[bad[0]], want_rows[bad[0]])
        if words is not None:
            assert np.array_equal(words, want_words), (what, form, "words")
        if want_sigs is not None:
            assert np.array_equal(sigs, want_sigs), (what, form, "sigs")
    return want_rows, want_info


# ---------------------------------------------------------------- tiles

PATTERNS = {"all": lambda j: np.ones(len(j), bool), "none": lambda j: np.zeros(len(j), bool), "alternate": lambda j: j % 2 == 0,
            "lane 0": lambda j: j % 64 == 0, "lane 63": lambda j: j % 64 == 63}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 127, 128, 129, 4097])
def test_tile_edges(xctx, n):
    """one selected candidate of n rows under the identity, the kept rows chosen by where they lie: all, none, every other one, only
    lane 0 and only lane 63 of each tile (a candidate without rows cannot be eligible - it has no anchor: test_refusals)"""
    j = np.arange(n)
    out, hyp = hypotheses([(9, 0, 0, (1, 0, 1))])
    for name, keep in PATTERNS.items():
        kept = keep(j)
        cand = unit_rows(np.where(kept, 100 + j % 37, 5000 + j % 37), 50 + j % 11)
        q = unit_rows([cand["x"][0], 6, 7], [cand["y"][0], 8, 9])   # the anchors coincide: x' = x and y' = y, exactly
        rows, info = check_expand(xctx, q, [cand], out, hyp, 1, (n, name), roi=(-1000, -1000, 1000, 1000))
        assert info.tolist() == [[0, n, int(kept.sum()), int(kept.sum())]] and len(rows) == 3 + kept.sum(), (n, name)
        assert rows[3:].tobytes() == cand[kept].tobytes(), (n, name)


@pytest.mark.gpu
def test_many_candidates(xctx):
    """several selected candidates whose counts are no multiples of 64, with random maps; and R = 1024 with 0 .. 3 rows each, every
    candidate that has a row selected"""
    rng = np.random.RandomState(7)
    q = make_rows(rng, 300)
    counts = [70, 1, 129, 64, 0, 191, 333, 2, 65]
    cands = [make_rows(rng, n) for n in counts]
    entries = [(int(rng.randint(1, 6)), int(rng.randint(300)), int(rng.randint(max(n, 1))), (0.5 + rng.rand(), rng.rand() - 0.5, 0.5 + rng.rand())) for n in counts]
    entries[4] = (0, -1, -1, (0, 0, 0))
    out, hyp = hypotheses(entries)
    rows, info = check_expand(xctx, q, cands, out, hyp, 1, "nine candidates", roi=(-50, -50, 250, 250))
    assert (info[[0, 2, 3, 5, 6, 8], 2] > 0).all() and (info[:, 2] < info[:, 1]).any() and info[4].tolist() == [-1, 0, 0, 0]
    counts = [r % 4 for r in range(1024)]
    cands = [make_rows(rng, n) for n in counts]
    out, hyp = hypotheses([(1 + r % 7, r % 300, 0, (1, 0, 1)) if n else (0, -1, -1, (0, 0, 0)) for r, n in enumerate(counts)])
    rows, info = check_expand(xctx, q, cands, out, hyp, 1, "R = 1024", roi=(-500, -500, 500, 500))
    assert (info[:, 0] >= 0).sum() == 768 and sorted(info[info[:, 0] >= 0, 0].tolist()) == list(range(768)) and info[:, 2].sum() > 1000


# ---------------------------------------------------------------- the region, known answers

@pytest.mark.gpu
def test_region_edges(xctx):
    """identity map, anchors at the origin, so x' = x and y' = y exactly: a key exactly on x0, x1, y0 or y1 is kept, the next float
    outside is dropped"""
    up, down = lambda v: np.nextafter(F(v), F(np.inf)), lambda v: np.nextafter(F(v), F(-np.inf))
    q = unit_rows([0], [0])
    xs = [0, 2, 7, down(2), up(7), 2, 7, 4, 4, 4, 4]
    ys = [0, 3, 9, 5, 5, 9, 3, 3, 9, down(3), up(9)]
    cand = unit_rows(xs, ys)
    out, hyp = hypotheses([(3, 0, 0, (1, 0, 1))])
    rows, info = check_expand(xctx, q, [cand], out, hyp, 1, "region edges", roi=(2, 3, 7, 9))
    assert info.tolist() == [[0, 11, 6, 6]]
    assert rows["x"][1:].tolist() == [2, 7, 2, 7, 4, 4] and rows["y"][1:].tolist() == [3, 9, 9, 3, 3, 9]
    rows, info = check_expand(xctx, q, [cand], out, hyp, 1, "a region that is one point", roi=(2, 3, 2, 3))
    assert info.tolist() == [[0, 11, 1, 1]]


@pytest.mark.gpu
def test_shifted_copy_doubles_the_query(xctx):
    """a copy of the query shifted by an integer offset expands to q ++ q, bit for bit; the tf-idf query on the expanded words returns
    the same images with bit-identical scores: dot doubles, nq2 quadruples, and the powers of two pass the three binary64 operations"""
    rng = np.random.RandomState(11)
    n = 500
    q = make_rows(rng, n)
    q["x"] = rng.randint(0, 900, n); q["y"] = rng.randint(0, 900, n)
    shifted = q.copy()
    shifted["x"] += F(37); shifted["y"] -= F(21)
    out, hyp = hypotheses([(n, 17, 17, (1, 0, 1))])
    rows, info = check_expand(xctx, q, [shifted], out, hyp, 1, "shifted copy", roi=(0, 0, 899, 899))
    assert rows.tobytes() == q.tobytes() + q.tobytes() and info.tolist() == [[0, n, n, n]]
    images = [np.ascontiguousarray(make_rows(rng, 300)["word"].astype(np.int32)) for _ in range(20)]
    images[3] = np.ascontiguousarray(q["word"][:400].astype(np.int32))
    xctx.build_index(images, K)
    try:
        a = xctx.query_index(np.ascontiguousarray(q["word"].astype(np.int32)), 20)
        b = xctx.query_index(np.ascontiguousarray(rows["word"].astype(np.int32)), 20)
        assert a[0][0] == 3 and a[0].tolist() == b[0].tolist() and a[1].tobytes() == b[1].tobytes()
    finally:
        xctx.clear_index()


@pytest.mark.gpu
def test_dyadic_map_by_hand(xctx):
    """L = (0.5, 0.25, 2), query anchor (10.5, -3.25), candidate anchor (100, 200): every operation is exact.
    key (103, 205), E = [[4, 1], [1, 2]]: u = 3 / .5 = 6, t = .25 * 6 = 1.5, s = 5 - 1.5 = 3.5, v = 3.5 / 2 = 1.75 -> (16.5, -1.5);
    e00 = 4 * .5 + 1 * .25 = 2.25, e10 = 1 * .5 + 2 * .25 = 1, e01 = 1 * 2 = 2, e11 = 2 * 2 = 4;
    a' = .5 * 2.25 + .25 * 1 = 1.375, b' = .5 * 2 + .25 * 4 = 2, c' = 2 * 4 = 8"""
    q = unit_rows([1, 10.5], [1, -3.25])
    cand = np.zeros(3, ROW)
    cand["x"] = [103, 100, 96]; cand["y"] = [205, 200, 201]; cand["a"] = 4; cand["b"] = 1; cand["c"] = 2; cand["word"] = [5, 6, 7]
    out, hyp = hypotheses([(2, 1, 1, (0.5, 0.25, 2))])
    rows, info = check_expand(xctx, q, [cand], out, hyp, 2, "dyadic")
    assert info.tolist() == [[0, 3, 3, 3]]
    # key (96, 201): u = -8, t = -2, s = 3, v = 1.5 -> (2.5, -1.75)
    assert rows[2:].tolist() == [(16.5, -1.5, 1.375, 2.0, 8.0, 5), (10.5, -3.25, 1.375, 2.0, 8.0, 6), (2.5, -1.75, 1.375, 2.0, 8.0, 7)]


# ---------------------------------------------------------------- random maps, forms, signatures

@pytest.fixture(scope="module")
def verified():
    """a query of 400 keys and nine candidates with random maps, inert keys on both sides, and signatures"""
    rng = np.random.RandomState(61)
    q = make_rows(rng, 400)
    q["b"][::50] = np.nan
    counts = [40 * r + 60 for r in range(9)]
    cands = [make_rows(rng, n, spread=300.0) for n in counts]
    cands[4]["b"][::9] = np.nan; cands[6]["c"][5] = 0; cands[2]["x"][3] = -np.inf
    entries = []
    for n in counts:
        entries.append((int(rng.randint(3, 40)), int(rng.choice(np.nonzero(~np.isnan(q["b"]))[0])), 1, (0.5 + rng.rand(), 0.6 * (rng.rand() - 0.5), 0.5 + rng.rand())))
    entries[1] = entries[1][:3] + ((1, 0, 1),)
    entries[7] = (entries[3][0],) + entries[7][1:]   # a tie between candidates 3 and 7
    out, hyp = hypotheses(entries)
    qs = rng.randint(0, 2 ** 62, len(q)).astype(np.uint64)
    cs = [rng.randint(0, 2 ** 62, n).astype(np.uint64) for n in counts]
    for a in [q, out, hyp, qs] + cands + cs:
        a.setflags(write=False)
    return q, cands, out, hyp, qs, cs


@pytest.mark.gpu
def test_random_maps_both_forms_with_and_without_signatures(xctx, verified):
    q, cands, out, hyp, qs, cs = verified
    roi = (20, 10, 180, 190)
    rows, info = check_expand(xctx, q, cands, out, hyp, 3, "random", roi=roi)
    assert (info[:, 0] >= 0).all() and (info[:, 2] > 0).all() and (info[:, 2] < info[:, 1]).all() and info[4, 1] < len(cands[4])
    assert not np.isnan(rows[400:]["a"]).any() and V.frames(rows[400:])[1].all()   # an expanded row is a row the verifier accepts
    check_expand(xctx, q, cands, out, hyp, 3, "random, signatures", roi=roi, qsigs=qs, csigs=cs)
    # roi = None: the bounding box of the query's live keys
    live = V.frames(q)[1]
    box = (q["x"][live].min(), q["y"][live].min(), q["x"][live].max(), q["y"][live].max())
    got, got_info = xctx.expand_query(q, cands, out, hyp, K, 3)
    want = X.expand(q, cands, out, hyp, 3, 1024, box)
    assert got.tobytes() == want[0].tobytes() and got_info.tolist() == want[3].tolist()
    # an empty query; candidates without a row that is selected
    empty = np.zeros(0, ROW)
    rows, info = check_expand(xctx, empty, cands, out, hyp, 100, "empty query, nothing eligible", roi=roi)
    assert len(rows) == 0


@pytest.mark.gpu
def test_candidates_permuted_and_repeated_calls(xctx, verified):
    q, cands, out, hyp, qs, cs = verified
    roi = (20, 10, 180, 190)
    rows, info = check_expand(xctx, q, cands, out, hyp, 3, "as given", roi=roi, forms=("host",))
    again, again_info = xctx.expand_query(q, cands, out, hyp, K, 3, roi=roi)
    assert again.tobytes() == rows.tobytes() and again_info.tolist() == info.tolist()
    perm = np.random.RandomState(3).permutation(len(cands))
    rows2, info2 = check_expand(xctx, q, [cands[i] for i in perm], out[perm], hyp[perm], 3, "permuted", roi=roi, forms=("host",))
    assert info2[:, 1:].tolist() == info[perm, 1:].tolist()
    # the same rows per candidate, in rank order: the ranks differ only inside the tie
    start = 400 + np.concatenate([[0], np.cumsum(info[np.argsort(info[:, 0]), 3])])
    start2 = 400 + np.concatenate([[0], np.cumsum(info2[np.argsort(info2[:, 0]), 3])])
    for r in range(len(cands)):
        s, s2 = info[perm[r], 0], info2[r, 0]
        assert rows[start[s]:start[s + 1]].tobytes() == rows2[start2[s2]:start2[s2 + 1]].tobytes(), r


@pytest.mark.gpu
def test_selection(xctx, verified):
    """ties in the inlier count go to the lower r; max_images below the number eligible cuts the weakest; min_inliers equal to a count
    keeps it; nothing eligible: the query, and nothing written behind it"""
    q, cands, out, hyp, qs, cs = verified
    roi = (20, 10, 180, 190)
    inl = out[:, 0]
    assert inl[3] == inl[7]
    rows, info = check_expand(xctx, q, cands, out, hyp, 1, "all", roi=roi)
    assert info[3, 0] + 1 == info[7, 0]
    for m in (1, 4, 8):
        rows, info = check_expand(xctx, q, cands, out, hyp, 1, ("max_images", m), max_images=m, roi=roi)
        assert (info[:, 0] >= 0).sum() == m and sorted(inl[info[:, 0] >= 0].tolist()) == sorted(inl.tolist())[-m:]
    level = int(np.sort(inl)[4])
    rows, info = check_expand(xctx, q, cands, out, hyp, level, "min_inliers at a count", roi=roi)
    assert ((info[:, 0] >= 0) == (inl >= level)).all() and (info[:, 0] >= 0).any() and (info[:, 0] < 0).any()
    # candidates that are not eligible may hold anything but their count
    wild_out, wild_hyp = out.copy(), hyp.copy()
    wild_out[inl < level, 1:] = -77; wild_hyp[inl < level] = np.nan
    rows2, info2 = check_expand(xctx, q, cands, wild_out, wild_hyp, level, "wild hypotheses below min_inliers", roi=roi)
    assert rows2.tobytes() == rows.tobytes()
    rows, info = check_expand(xctx, q, cands, out, hyp, int(inl.max()) + 1, "nothing eligible", roi=roi, qsigs=qs, csigs=cs)
    assert rows.tobytes() == q.tobytes() and info.tolist() == [[-1, 0, 0, 0]] * len(cands)


# ---------------------------------------------------------------- extremes, inert keys

@pytest.mark.gpu
def test_extremes(xctx):
    """L11 = 2^-40 with |dx| = 2^21 and L21 = +-2^81: u = +-2^61, v infinite; an a' that is inf - inf; the largest ellipse under the
    largest scale.  Nothing is kept, no NaN reaches an output, every key counts as live"""
    B = 2.0 ** 20
    q = unit_rows([0, 1], [0, 1])
    far = unit_rows([B, -B, -B, B, 0], [-B, B, -B, B, 0])
    c2 = np.zeros(2, ROW); c2["a"] = 2.0 ** 40; c2["b"] = 1000; c2["c"] = 1e6
    c3 = np.zeros(2, ROW); c3["a"] = 2.0 ** 40; c3["c"] = 2.0 ** 40
    cands = [far, far.copy(), c2, c3]
    out, hyp = hypotheses([(5, 0, 1, (2.0 ** -40, 2.0 ** 81, 2.0 ** -40)), (5, 1, 0, (2.0 ** -40, -2.0 ** 81, 2.0 ** 40)), (5, 0, 0, (2.0 ** 40, -2.0 ** 81, 1)),
                           (5, 0, 0, (2.0 ** 40, 0, 2.0 ** 40))])
    for r, k in ((0, 1), (1, 0)):   # (even the anchor goes: it maps onto the query's anchor, but its a' overflows)
        new, live, kept = X.back_project(cands[r], q[out[r, 3]], cands[r][k], hyp[r], BIG)
        assert live.all() and not kept.any() and np.isinf(new["y"]).any() and not np.isnan(new["y"]).any() and np.abs(new["x"]).max() == 2.0 ** 61
    assert np.isnan(X.back_project(c2, q[0], c2[0], hyp[2], BIG)[0]["a"]).all()
    rows, info = check_expand(xctx, q, cands, out, hyp, 5, "extremes")
    assert info[:, 1:].tolist() == [[5, 0, 0], [5, 0, 0], [2, 0, 0], [2, 0, 0]]
    assert len(rows) == 2 and not np.isnan(rows.view(F).reshape(-1, 6)[:, :5]).any()


@pytest.mark.gpu
def test_inert_keys(xctx):
    """a NaN in each field of a candidate row: dropped and counted as not live; the same rows in the query: copied through"""
    rng = np.random.RandomState(19)
    q = make_rows(rng, 70)
    cand = make_rows(rng, 140)
    for i, f in enumerate("xyabc"):
        cand[f][10 + 20 * i] = np.nan
        q[f][3 + 5 * i] = np.nan
    q["a"][40] = -1; q["x"][41] = np.inf
    out, hyp = hypotheses([(4, 0, 0, (1.5, 0.25, 0.75))])
    rows, info = check_expand(xctx, q, [cand], out, hyp, 1, "inert keys")
    assert info[0, 1] == 135 and rows[:70].tobytes() == q.tobytes() and V.frames(rows[70:])[1].all()


# ---------------------------------------------------------------- truncation

@pytest.mark.gpu
def test_truncation(xctx):
    """kept_total one below, at and one above the room max_rows leaves; max_rows = nq; the written counts per candidate"""
    rng = np.random.RandomState(23)
    q = make_rows(rng, 100)
    cands = [make_rows(rng, n) for n in (150, 90, 200)]
    out, hyp = hypotheses([(5, 0, 0, (1, 0, 1)), (9, 1, 1, (1, 0.5, 1)), (7, 2, 2, (2, 0, 0.5))])
    roi = (0, 0, 250, 250)
    total = int(X.expand(q, cands, out, hyp, 1, 1024, roi)[3][:, 2].sum())
    assert 150 < total < 440
    for max_rows in (100 + total + 1, 100 + total, 100 + total - 1, 100 + 95, 101, 100):
        rows, info = check_expand(xctx, q, cands, out, hyp, 1, ("max_rows", max_rows), roi=roi, max_rows=max_rows)
        assert len(rows) == min(100 + total, max_rows) and info[:, 3].sum() == len(rows) - 100 and info[:, 2].sum() == total
    # the cut falls on the weakest candidate first: candidate 0 (5 inliers) loses its highest keys, then 2, then 1
    rows, info = check_expand(xctx, q, cands, out, hyp, 1, "cut inside candidate 2", roi=roi, max_rows=100 + info[1, 2] + 10, forms=("host",))
    assert info[1, 3] == info[1, 2] and info[2, 3] == 10 and info[0, 3] == 0


@pytest.mark.gpu
def test_one_candidate_of_2_18_rows(xctx):
    """nq = 1 and one candidate of 2^18 kept rows at max_rows = 2^18: all but one are written"""
    n = 1 << 18
    j = np.arange(n)
    q = unit_rows([3], [4])
    cand = unit_rows(j % 1024, j // 1024, words=j % K)
    out, hyp = hypotheses([(50, 0, 0, (1, 0, 1))])
    rows, info = check_expand(xctx, q, [cand], out, hyp, 1, "2^18 rows", roi=(0, 0, 2000, 2000))
    assert info.tolist() == [[0, n, n, n - 1]] and len(rows) == n


# ---------------------------------------------------------------- event times

@pytest.mark.gpu
def test_expand_ms_are_event_times(xctx, verified):
    q, cands, out, hyp, qs, cs = verified
    xctx.set_profiling(1)
    try:
        xctx.expand_query(q, cands, out, hyp, K, 3)
        ms = xctx.expand_ms
        print("expand_ms (flags, scatter) for 9 candidates:", ms)
        assert all(0.0 < v < 1000.0 for v in ms)
    finally:
        xctx.set_profiling(0)
    xctx.expand_query(q, cands, out, hyp, K, 3)
    assert xctx.expand_ms == (0.0, 0.0)


# ---------------------------------------------------------------- end to end

E2E_CROP = (8, 12, 112, 152)        # rows 8..111, columns 12..151 of band_160x120
E2E_ROI = (0.0, 0.0, 139.0, 103.0)  # the crop's extent: the query is the crop
E2E_KEYS = [221, 128, 74, 71]       # band_160x120, its crop, band_96x96, band_131x77
E2E_TOL = 5.0
# On the CPU oracle's keys with the numpy references, the crop as the query, P = 1, tol = 5:
E2E_INLIERS = {0: 128, 1: 128, 2: 3, 3: 5}   # by image: the two related images far above the unrelated ones
E2E_MIN_INLIERS = 20                          # anywhere in 6 .. 128 selects exactly images 0 and 1
E2E_KEPT = {0: 219, 1: 128}                   # of 221 and 128 live keys, inside the crop's extent
E2E_N_OUT = 128 + 219 + 128


@pytest.fixture(scope="module")
def e2e(xctx, tmp_path_factory):
    """band_160x120, a shifted crop of it and two unrelated images, detected under a vocabulary made of the first image's own 221
    descriptors (all distinct: a copy of a key finds its own word), written as words files and read back as rows"""
    d = tmp_path_factory.mktemp("expand_e2e")
    img = hesaff_amd.read_pnm(os.path.join(GOLD, "band_160x120.pgm"))
    y0, x0, y1, x1 = E2E_CROP
    crop = np.ascontiguousarray(img[y0:y1, x0:x1])
    imgs = [img, crop, hesaff_amd.read_pnm(os.path.join(GOLD, "band_96x96.pgm")), hesaff_amd.read_pnm(os.path.join(GOLD, "band_131x77.pgm"))]
    image_paths = [os.path.join(GOLD, "band_160x120.pgm"), str(d / "crop.pgm"), os.path.join(GOLD, "band_96x96.pgm"), os.path.join(GOLD, "band_131x77.pgm")]
    with open(image_paths[1], "wb") as f:
        f.write(b"P5\n%d %d\n255\n" % (crop.shape[1], crop.shape[0]) + crop.tobytes())
    plain = xctx.detect_batch(imgs)
    vocab = np.ascontiguousarray(plain[0][1]["desc"])
    assert len(np.unique(vocab, axis=0)) == len(vocab) == 221
    xctx.set_vocabulary(vocab)
    try:
        res = xctx.detect_batch(imgs)
        words = [xctx.words(i) for i in range(len(imgs))]
    finally:
        xctx.set_vocabulary(None)
    assert [len(k) for _, k in res] == E2E_KEYS
    paths, rows = [], []
    for j, ((_, keys), w) in enumerate(zip(res, words)):
        paths.append(str(d / ("%d.pgm.hesaff.words" % j)))
        hesaff_amd.write_words(paths[-1], keys, w, xctx.params.mrSize, len(vocab))
        vs, r = hesaff_amd.read_words(paths[-1])
        assert vs == 221
        r.setflags(write=False)
        rows.append(r)
    return imgs, image_paths, res, words, vocab, paths, rows


@pytest.mark.gpu
def test_end_to_end_python(xctx, e2e):
    imgs, image_paths, res, words, vocab, paths, rows = e2e
    xctx.build_index(words, 221)
    try:
        shortlist, scores = xctx.query_index(words[1], 4)
        assert sorted(shortlist.tolist()) == [0, 1, 2, 3]
        cands = [rows[i] for i in shortlist]
        out, hyp, order = xctx.verify_matches(rows[1], cands, 221, E2E_TOL, 1)
        print("end to end: shortlist", shortlist.tolist(), "inliers", out[:, 0].tolist())
        assert {int(i): int(out[r, 0]) for r, i in enumerate(shortlist)} == E2E_INLIERS
        got, info = check_expand(xctx, rows[1], cands, out, hyp, E2E_MIN_INLIERS, "golden images", roi=E2E_ROI, k=221)
        by_image = {int(i): info[r] for r, i in enumerate(shortlist)}
        print("end to end: n_out", len(got), "info by image", {i: v.tolist() for i, v in by_image.items()})
        assert len(got) == E2E_N_OUT and {i: int(v[2]) for i, v in by_image.items() if v[0] >= 0} == E2E_KEPT
        assert by_image[2].tolist() == by_image[3].tolist() == [-1, 0, 0, 0]
        second, scores2 = xctx.query_index(np.ascontiguousarray(got["word"].astype(np.int32)), 4)
        assert sorted(second[:2].tolist()) == [0, 1]
        # the same through the convenience, whose region is the bounding box of the query's live keys
        first, again, rows2, info2 = xctx.query_index_expanded(rows[1], rows, 4, E2E_TOL, E2E_MIN_INLIERS, roi=E2E_ROI)
        assert first[0].tolist() == shortlist.tolist() and first[2].tobytes() == out.tobytes() and first[3].tolist() == order.tolist()
        assert rows2.tobytes() == got.tobytes() and again[0].tolist() == second.tolist() and again[1].tobytes() == scores2.tobytes()
        assert xctx.index_info[0] == 4   # the index is as it was
    finally:
        xctx.clear_index()


@pytest.mark.gpu
def test_end_to_end_cli_search_verify_expand(e2e, tmp_path):
    """hesaff --search ... --verify --expand prints the verified list, "# expanded: <rows> rows from <images> images" and the verified
    list of the expanded query; the region is the bounding box of the query's live rows.  --index answers the same.
    The expanded query repeats the words of the related images (here three times: the crop, band_160x120 and the crop again), so at
    --pairs 1 the second verification finds hardly a pair - on the CPU oracle's keys 34, 0, 2 and 1 inliers - and the second list is
    held by its tf-idf scores; at --pairs 4 it gives 417 and 383 inliers for the related images against 10 and 15."""
    imgs, image_paths, res, words, vocab, paths, rows = e2e
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    plain = subprocess.run([EXE, "--search", str(lst), "--query", paths[1], "--top", "4"], capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr
    shortlist = [paths.index(l.split("\t")[1]) for l in plain.stdout.strip().split("\n")]   # the order the expansion sees the candidates in
    base = [EXE, "--search", str(lst), "--query", paths[1], "--top", "4", "--verify", "--tolerance", "5"]
    r0 = subprocess.run(base, capture_output=True, text=True, timeout=600)
    assert r0.returncode == 0, r0.stderr
    r = subprocess.run(base + ["--expand", "--min-inliers", str(E2E_MIN_INLIERS)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[:4] == r0.stdout.strip().split("\n") and len(lines) == 9
    first = [l.split("\t") for l in lines[:4]]
    assert {paths.index(l[1]): int(l[3]) for l in first} == E2E_INLIERS
    cands = [rows[i] for i in shortlist]
    out, hyp, _, _, _ = V.verify(rows[1], cands, 1, E2E_TOL)
    live = V.frames(rows[1])[1]
    box = (rows[1]["x"][live].min(), rows[1]["y"][live].min(), rows[1]["x"][live].max(), rows[1]["y"][live].max())
    want, _, _, info = X.expand(rows[1], cands, out, hyp, E2E_MIN_INLIERS, 10, box)
    assert lines[4] == "# expanded: %d rows from 2 images" % len(want) and sorted(shortlist[r] for r in np.nonzero(info[:, 0] >= 0)[0]) == [0, 1]
    second = [l.split("\t") for l in lines[5:]]
    assert [int(l[0]) for l in second] == [1, 2, 3, 4]
    by_score = sorted(second, key=lambda l: -float(l[2]))
    assert sorted(paths.index(l[1]) for l in by_score[:2]) == [0, 1]   # the second query still ranks the related images first
    out2 = V.verify(want, [rows[paths.index(l[1])] for l in second], 1, E2E_TOL)[0]
    assert [int(l[3]) for l in second] == out2[:, 0].tolist() and (np.diff(out2[:, 0]) <= 0).all()
    # more pairs per word: the repeated words of the expanded query verify, and the related images lead the verified list too
    r4 = subprocess.run(base + ["--pairs", "4", "--expand", "--min-inliers", str(E2E_MIN_INLIERS)], capture_output=True, text=True, timeout=600)
    assert r4.returncode == 0, r4.stderr
    lines4 = r4.stdout.strip().split("\n")
    out4, hyp4, _, _, _ = V.verify(rows[1], cands, 4, E2E_TOL)
    want4 = X.expand(rows[1], cands, out4, hyp4, E2E_MIN_INLIERS, 10, box)[0]
    assert len(lines4) == 9 and lines4[4] == "# expanded: %d rows from 2 images" % len(want4)
    second4 = [l.split("\t") for l in lines4[5:]]
    assert [paths.index(l[1]) for l in second4[:2]] == [0, 1]
    out5 = V.verify(want4, [rows[paths.index(l[1])] for l in second4], 4, E2E_TOL)[0]
    assert [int(l[3]) for l in second4] == out5[:, 0].tolist() and out5[1, 0] > 10 * out5[2, 0]
    # one image at most: the same first list, one image in the line
    r = subprocess.run(base + ["--expand", "--expand-images", "1", "--min-inliers", "1"], capture_output=True, text=True, timeout=600)
    want1 = X.expand(rows[1], cands, out, hyp, 1, 1, box)[0]
    assert r.returncode == 0 and r.stdout.split("\n")[4] == "# expanded: %d rows from 1 images" % len(want1)
    # a saved index
    idx = str(tmp_path / "four.index")
    assert subprocess.run([EXE, "--search", str(lst), "--save-index", idx], capture_output=True, text=True, timeout=600).returncode == 0
    r2 = subprocess.run([EXE, "--index", idx, "--query", paths[1], "--top", "4", "--verify", "--tolerance", "5", "--expand", "--min-inliers", str(E2E_MIN_INLIERS)],
                        capture_output=True, text=True, timeout=600)
    assert r2.returncode == 0 and r2.stdout.strip().split("\n") == lines, r2.stderr


@pytest.mark.gpu
def test_end_to_end_cpp_member(e2e, tmp_path):
    """tests/native/expand_keys.cpp: expandQuery through hesaff.hpp holds what the Python path holds"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, image_paths, res, words, vocab, paths, rows = e2e
    exe = str(tmp_path / "expand_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "expand_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    r = subprocess.run([exe, vfile, "5", str(E2E_MIN_INLIERS), str(tmp_path)] + ["%g" % v for v in E2E_ROI] + [image_paths[1]] + image_paths,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out, hyp, _, _, _ = V.verify(rows[1], rows, 1, E2E_TOL)
    want, want_words, _, info = X.expand(rows[1], rows, out, hyp, E2E_MIN_INLIERS, 1024, E2E_ROI)
    h = 1469598103934665603
    for b in want.tobytes():
        h = ((h ^ b) * 1099511628211) & (2 ** 64 - 1)
    live = V.frames(rows[1])[1]
    box = (rows[1]["x"][live].min(), rows[1]["y"][live].min(), rows[1]["x"][live].max(), rows[1]["y"][live].max())
    assert len(want) == E2E_N_OUT
    assert r.stdout.strip().split("\n") == ["N %d" % len(want)] + ["I %d %d %d %d %d" % ((c,) + tuple(info[c])) for c in range(4)] + \
        ["H %d" % h, "W %d" % int(want_words.sum()), "B %.9g %.9g %.9g %.9g" % box, "C refused"]


# ---------------------------------------------------------------- refusals and isolation

@pytest.mark.gpu
def test_refusals_leave_everything_as_it_was(e2e):
    import torch
    imgs, image_paths, res, words, vocab, paths, rows = e2e
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        L, h = c.L, c.h
        c.set_vocabulary(vocab)
        c.build_index(words, 221)
        cands = rows[:3]
        vout, vhyp, vorder = c.verify_matches(rows[1], cands, 221, E2E_TOL)
        want_pairs = c.verify_pairs(0)
        want = c.expand_query(rows[1], cands, vout, vhyp, 221, E2E_MIN_INLIERS, roi=E2E_ROI)

        def still_works(what):
            assert c.vocabulary_size == 221 and c.index_info[0] == 4, what
            (nh, keys), = c.detect_batch(imgs[2:3])
            assert keys.tobytes() == res[2][1].tobytes() and np.array_equal(c.words(0), words[2]), what
            im, sc = c.query_index(words[0], 4)
            assert im[0] == 0, what
            assert np.array_equal(c.verify_pairs(0), want_pairs), what   # the last verify call's result is still there
            got = c.expand_query(rows[1], cands, vout, vhyp, 221, E2E_MIN_INLIERS, roi=E2E_ROI)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tolist() == want[1].tolist(), what
        still_works("before")
        q = rows[1].copy(); flat = np.concatenate(cands); counts = np.array([len(r) for r in cands], np.int32)
        qs = np.arange(len(q), dtype=np.uint64); cs = np.arange(len(flat), dtype=np.uint64)
        roi = np.array(E2E_ROI, F)
        cap = len(q) + len(flat)
        o_rows = np.full(cap, 7, ROW); o_words = np.full(cap, 7, np.int32); o_sigs = np.full(cap, 7, np.uint64); o_info = np.full((3, 4), 7, np.int32); n = ctypes.c_int(7)
        up = lambda a: torch.from_numpy(np.frombuffer(a.tobytes(), np.uint8).copy()).cuda()
        tq, tc, tqs, tcs = up(q), up(flat), up(qs), up(cs)
        t_rows = torch.full((cap * 24,), 7, dtype=torch.uint8, device="cuda"); t_words = torch.full((cap * 4,), 7, dtype=torch.uint8, device="cuda")
        t_sigs = torch.full((cap * 8,), 7, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        P = ctypes.c_void_p

        def host(nq=len(q), qp=q.ctypes.data, qsp=None, R=3, cp=counts.ctypes.data, rp=flat.ctypes.data, csp=None, op=vout.ctypes.data, hp=vhyp.ctypes.data,
                 mi=E2E_MIN_INLIERS, images=1024, roi_p=roi.ctypes.data, k=221, max_rows=2 ** 18, ro=o_rows.ctypes.data, wo=o_words.ctypes.data, so=None):
            return L.hesaff_expand_query(h, nq, qp, qsp, R, cp, rp, csp, op, hp, mi, images, roi_p, k, max_rows, ro, wo, so, ctypes.byref(n), o_info.ctypes.data)

        def dev(nq=len(q), qp=tq.data_ptr(), qsp=None, R=3, cp=counts.ctypes.data, rp=tc.data_ptr(), csp=None, op=vout.ctypes.data, hp=vhyp.ctypes.data,
                mi=E2E_MIN_INLIERS, images=1024, roi_p=roi.ctypes.data, k=221, max_rows=2 ** 18, ro=t_rows.data_ptr(), wo=t_words.data_ptr(), so=None):
            z = lambda p: None if p is None else P(p)
            return L.hesaff_expand_query_device(h, nq, z(qp), z(qsp), R, cp, z(rp), z(csp), op, hp, mi, images, roi_p, k, max_rows, z(ro), z(wo), z(so), ctypes.byref(n),
                                                o_info.ctypes.data)
        assert host() == 0 and n.value == len(want[0]) and o_rows[:n.value].tobytes() == want[0].tobytes() and dev() == 0 and n.value == len(want[0])
        o_rows[:] = 7; o_words[:] = 7; o_info[:] = 7; n.value = 7
        t_rows.fill_(7); t_words.fill_(7)
        sig_args = ((host, dict(qsp=qs.ctypes.data, csp=cs.ctypes.data, so=o_sigs.ctypes.data)), (dev, dict(qsp=tqs.data_ptr(), csp=tcs.data_ptr(), so=t_sigs.data_ptr())))
        for f, sg in sig_args:
            assert f(qp=None) == ARG and f(cp=None) == ARG and f(rp=None) == ARG and f(op=None) == ARG and f(hp=None) == ARG and f(roi_p=None) == ARG
            assert f(ro=None) == ARG and f(wo=None) == ARG
            for R_, k_ in ((0, 221), (-1, 221), (1025, 221), (3, 0), (3, (1 << 20) + 1)):
                big = np.zeros(max(R_, 3), np.int32)
                assert f(R=R_, cp=big.ctypes.data, k=k_) == ARG, (R_, k_)
            for bad in ([2, -1, 1], [2, (1 << 18) + 1, 1]):
                assert f(cp=np.array(bad, np.int32).ctypes.data) == ARG, bad
            assert f(nq=-1) == ARG and f(nq=(1 << 18) + 1) == ARG
            assert f(mi=0) == ARG and f(mi=-3) == ARG and f(images=0) == ARG and f(images=1025) == ARG
            assert f(max_rows=len(q) - 1) == ARG and f(max_rows=(1 << 18) + 1) == ARG and f(max_rows=-1) == ARG
            for bad in ((np.nan, 0, 1, 1), (0, 0, np.inf, 1), (0, -np.inf, 1, 1), (2, 0, 1, 1), (0, 2, 1, 1), (0, 0, 1, 2.0 ** 20 + 1), (-2.0 ** 21, 0, 1, 1)):
                assert f(roi_p=np.array(bad, F).ctypes.data) == ARG, bad
            assert f(k=220) == ARG   # a word >= K: the host form finds it while staging, the device form by its check kernel
            # signatures on one side only, or without an output for them
            assert f(qsp=sg["qsp"]) == ARG and f(csp=sg["csp"]) == ARG and f(so=sg["so"]) == ARG and f(qsp=sg["qsp"], csp=sg["csp"]) == ARG
            assert f(qsp=sg["qsp"], so=sg["so"]) == ARG and f(csp=sg["csp"], so=sg["so"]) == ARG
            # an eligible candidate that is broken: its keys, its map, its anchor rows - named
            for field, value in ((3, -1), (3, len(q)), (4, -1), (4, int(counts[0]))):
                bo = vout.copy(); bo[0, field] = value
                assert f(op=bo.ctypes.data) == ARG and "candidate 0" in c.L.hesaff_last_error(h).decode(), (field, value)
            for col, value in ((0, np.nan), (0, 0.0), (0, 2.0 ** 41), (1, -2.0 ** 82), (2, 2.0 ** -41), (2, -1.0)):
                bh = vhyp.copy(); bh[1, col] = value
                assert f(hp=bh.ctypes.data) == ARG and "candidate 1" in c.L.hesaff_last_error(h).decode(), (col, value)
            # ... and the same breakage below min_inliers is nobody's business
            bo = vout.copy(); bo[2, 3:5] = -9
            bh = vhyp.copy(); bh[2] = np.nan
            assert vout[2, 0] < E2E_MIN_INLIERS and f(op=bo.ctypes.data, hp=bh.ctypes.data) == 0 and n.value == len(want[0])
            o_rows[:] = 7; o_words[:] = 7; o_info[:] = 7; n.value = 7
            t_rows.fill_(7); t_words.fill_(7)
        # an anchor row that is not live
        dead = flat.copy(); dead["c"][vout[0, 4]] = np.nan
        td = up(dead)
        dq = q.copy(); dq["a"][vout[1, 3]] = -1.0
        tdq = up(dq)
        torch.cuda.synchronize()
        assert host(rp=dead.ctypes.data) == ARG and dev(rp=td.data_ptr()) == ARG and "candidate 0" in c.L.hesaff_last_error(h).decode()
        assert host(qp=dq.ctypes.data) == ARG and dev(qp=tdq.data_ptr()) == ARG
        assert dev(qp=tq.data_ptr() + 2) == ARG and dev(rp=tc.data_ptr() + 1) == ARG and dev(ro=t_rows.data_ptr() + 2) == ARG and dev(wo=t_words.data_ptr() + 1) == ARG
        assert dev(qsp=tqs.data_ptr() + 4, csp=tcs.data_ptr(), so=t_sigs.data_ptr()) == ARG
        bad = flat.copy(); bad["word"][len(bad) - 1] = 221
        tb = up(bad)
        torch.cuda.synchronize()
        assert host(rp=bad.ctypes.data) == ARG and dev(rp=tb.data_ptr()) == ARG   # (a word of a candidate that is not selected: still checked)
        ms = ctypes.c_float(7)
        assert L.hesaff_get_expand_ms(h, None, ctypes.byref(ms)) == ARG and L.hesaff_get_expand_ms(h, ctypes.byref(ms), None) == ARG and ms.value == 7.0
        torch.cuda.synchronize()
        assert o_rows.tobytes() == np.full(cap, 7, ROW).tobytes() and (o_words == 7).all() and (o_info == 7).all() and n.value == 7 and (o_sigs == 7).all()
        assert (t_rows.cpu().numpy() == 7).all() and (t_words.cpu().numpy() == 7).all() and (t_sigs.cpu().numpy() == 7).all()
        with pytest.raises(ValueError):
            c.expand_query(np.zeros(3, np.int32), cands, vout, vhyp, 221, 3)
        with pytest.raises(ValueError):
            c.expand_query(rows[1], cands, vout, vhyp, 221, 3, query_signatures=qs)
        with pytest.raises(hesaff_amd.HesaffError):
            c.expand_query(rows[1], cands, vout, vhyp, 221, 0)
        still_works("after the refusals")
        # info_out may be NULL; with signatures the third output is written
        assert L.hesaff_expand_query(h, len(q), q.ctypes.data, qs.ctypes.data, 3, counts.ctypes.data, flat.ctypes.data, cs.ctypes.data, vout.ctypes.data, vhyp.ctypes.data,
                                     E2E_MIN_INLIERS, 1024, roi.ctypes.data, 221, 2 ** 18, o_rows.ctypes.data, o_words.ctypes.data, o_sigs.ctypes.data, ctypes.byref(n),
                                     None) == 0
        assert n.value == len(want[0]) and o_rows[:n.value].tobytes() == want[0].tobytes() and o_sigs[:len(q)].tolist() == qs.tolist() and (o_info == 7).all()


@pytest.mark.gpu
def test_detection_is_untouched_by_an_expand_call(xctx, e2e, verified):
    """the keys of a detecting call after an expand call are byte-equal to those before it"""
    imgs, image_paths, res, words, vocab, paths, rows = e2e
    q, cands, out, hyp, qs, cs = verified
    before = xctx.detect_batch(imgs)
    xctx.expand_query(q, cands, out, hyp, K, 3)
    after = xctx.detect_batch(imgs)
    for (na, a), (nb, b) in zip(after, before):
        assert na == nb and a.tobytes() == b.tobytes()
