"""The detection chain - k_extrema_march -> k_localize -> k_dedupe -> scan / k_scatter_ordered / k_hess_deal - on constructed response
planes at the edges of its domain (tests/detect_inputs.py).

CPU half (no mark): the oracle's trace of localizeKeypoint alone proves that every site takes the branch it was built for - candidate
or not, the centre of every iteration, the exit, the bits of b / val / edgeScore where a site claims them - and that every claim shows
in the kept list, so that a GPU error at that site changes the output.
GPU half (pytest.mark.gpu): hesaff_stage_detect_planes, which runs the production launches on caller-supplied planes, against the
oracle's kept list: count, order, (type, octave, level, r0, c0) and the bits of x, y, s, pixelDistance and response.  All
comparisons are equalities.
"""
import functools

import numpy as np
import pytest

from tests import detect_inputs as di

F = np.float32
gpu = pytest.mark.gpu
PSETS = list(di.PSETS)
SINGLE = [n for n in di.SCENES if n != "all262"]   # all262 has the band test to itself


def _params(pset):
    import hesaff_amd
    p = hesaff_amd.default_params()
    for k, v in di.PSETS[pset].items():
        setattr(p, k, v)
    return p


@functools.lru_cache(maxsize=None)
def _planes(name, pset, garbage_seed=1):
    L, R, sites = di.planes(name, pset, garbage_seed)
    L.setflags(write=False); R.setflags(write=False)
    return L, R, sites


@functools.lru_cache(maxsize=None)
def _oracle_run(name, pset, garbage_seed=1):
    """the oracle's scans of a scene's planes: kept list and trace; computed once and shared"""
    from tests import _oracle
    L, R, _ = _planes(name, pset, garbage_seed)
    run = _oracle.PlanesRun(L, R, params=_params(pset))
    for a in (run.f, run.i, run.trace_i, run.trace_u):
        a.setflags(write=False)
    return run


def _kept_set(run):
    return {(int(l), int(r), int(c)): (int(t), k) for k, (t, _, l, r, c) in enumerate(run.i)}


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the inputs reach what they claim
# ----------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pset", PSETS)
def test_thresholds_are_the_oracles(oracle, pset):
    assert [di.bits(v) for v in di.thresholds(pset)] == [di.bits(v) for v in oracle.thresholds(_params(pset))]
    if pset == "ratio4":
        assert di.thresholds(pset)[2] == F(6.25)


def _check_site(oracle, run, kept, L, R, rows, cols, s):
    """every claim of one site against the trace and the kept list -> the exits it claimed"""
    st = s.stencil
    seen = []
    for n, (level, r0, c0, claim) in enumerate(s.claims(rows, cols)):
        t = run.trace_at(level, r0, c0)
        what = (repr(s), level, r0, c0, claim)
        if claim is None:
            assert t is None and (level, r0, c0) not in kept, what
            continue
        assert t is not None, what
        ti, tu = t
        if claim == ():
            continue
        iters, final, exit_, path = claim
        got_path = [(int(ti[7 + 2 * k]), int(ti[8 + 2 * k])) for k in range(int(ti[3]))]
        assert (int(ti[3]), (int(ti[4]), int(ti[5])), int(ti[6]), got_path) == (iters, final, exit_, path), (what, ti, [hex(x) for x in tu])
        # a kept claim and a dropped claim both show in the output
        assert ((level, r0, c0) in kept) == (exit_ == di.KEPT), what
        seen.append(exit_)
        if n == 0 and len(path) == len(st.path):   # (not cut short by a border)
            for key, u in st.bits.items():
                assert int(tu[{"b0": 0, "b1": 1, "b2": 2, "val": 3, "edge": 4}[key]]) == u, (what, key, hex(u), [hex(x) for x in tu])
            if st.bits_at is not None:
                (dr, dc), k, u = st.bits_at
                assert (s.r0 + dr, s.c0 + dc) in path, what
                A, b = di.local_system(R, level, s.r0 + dr, s.c0 + dc)
                oracle.lib().ho_solve_linear3x3(A, b)
                assert di.bits(b[k]) == u, (what, hex(di.bits(b[k])), hex(u))
            if st.type is not None and exit_ == di.KEPT:
                assert kept[(level, r0, c0)][0] == st.type == di.l_type(L, level, *final), (what, kept[(level, r0, c0)])
                if final != (r0, c0):   # a moved site: L at the first centre gives the other type
                    assert di.l_type(L, level, r0, c0) == 1 - st.type, what
    return seen


@pytest.mark.parametrize("pset", PSETS)
def test_every_site_reaches_what_it_claims(oracle, pset):
    """Kind by kind and position by position: candidate or not, iterations, every centre, the exit, the claimed bits, the type, and
    kept <=> present in the kept list.  Over all scenes every exit of localizeKeypoint occurs, claimed by some site."""
    exits = set(); kinds = {}
    for name in di.SCENES:
        L, R, sites = _planes(name, pset)
        run = _oracle_run(name, pset)
        kept = _kept_set(run)
        for s in sites:
            exits |= set(_check_site(oracle, run, kept, L, R, R.shape[1], R.shape[2], s))
            kinds.setdefault(s.kind, set()).add(s.stencil.name)
    assert exits == set(range(11)), sorted(exits)
    assert set(kinds) == {"threshold", "edge", "ties", "pivot", "move", "shift06", "shift15", "type", "collision", "comb", "position", "border"}


def test_moves_cover_every_direction_and_length(oracle):
    """one move in each of the four directions, a diagonal one (both indices change in one iteration), chains of 2, 3 and 4 moves, and a
    site that still asks to move at the fifth iteration"""
    run = _oracle_run("catalogue70", "default")
    steps = set(); lengths = set(); fifth = False
    for ti, tu in zip(run.trace_i, run.trace_u):
        pth = [(int(ti[7 + 2 * k]), int(ti[8 + 2 * k])) for k in range(int(ti[3]))]
        steps |= {(b[0] - a[0], b[1] - a[1]) for a, b in zip(pth, pth[1:])}
        if ti[6] == di.KEPT:
            lengths.add(len(pth) - 1)
            b0, b1 = di.from_bits(tu[0]), di.from_bits(tu[1])
            fifth |= len(pth) == 5 and (abs(float(b0)) > 0.6 or abs(float(b1)) > 0.6)
    assert {(0, 1), (0, -1), (1, 0), (-1, 0), (1, 1)} <= steps and {0, 1, 2, 3, 4} <= lengths and fifth


def test_shift_sites_sit_on_the_comparisons(oracle):
    """The 0.6 sites' b is the float32 adjacent to the double 0.6 on either side (16 steps were allowed; every site reached step 1 in
    REACHED's count), the 1.5 sites' b is 1.5 and the float32 above it, the near crosses' edgeScore is the float32 adjacent to 6.25."""
    below, above = 0x3f199999, 0x3f19999a
    assert float(di.from_bits(below)) < 0.6 < float(di.from_bits(above)) and above - below == 1
    for k in ("b0", "b1"):
        assert di.REACHED[k + "_06_below"] == (below, 1) and di.REACHED[k + "_06_above"] == (above, 1)
    for k in ("b0", "b1", "b2"):
        assert di.REACHED[k + "_15_above"] == (di.bits(F(1.5)) + 1, 1)
    assert di.SEARCHED["b0_15"]["bits"]["b0"] == di.bits(F(1.5)) and di.SEARCHED["b2_15"]["bits"]["b2"] == di.bits(F(1.5))
    assert di.bits(di.edge_score(di.cross(16.0, 64.0))) == di.bits(F(6.25))
    for side, d in (("below", -1), ("above", 1)):
        assert di.bits(di.cross_near(side)[1]) - di.bits(F(6.25)) == d, side


def test_solve_replica_is_the_oracles(oracle):
    """detect_inputs.solve3x3 without a flip is solveLinear3x3: on the system of every candidate's first centre of the catalogue"""
    L, R, _ = _planes("catalogue70", "default")
    n = 0
    for ti in _oracle_run("catalogue70", "default").trace_i[::3]:
        A, b = di.local_system(R, int(ti[0]), int(ti[1]), int(ti[2]))
        want = b.copy(); A2 = A.copy()
        oracle.lib().ho_solve_linear3x3(A2, want)
        got = di.solve3x3(A, b)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (ti[:3], got, want)
        n += 1
    assert n > 200


def test_pivot_sites_tie_where_they_claim(oracle):
    """Each pivot site's first system has its tie, and is regular; the reference's solve gives the b the site claims (which the trace
    confirms: test_every_site_reaches_what_it_claims) and the solve that takes the other pivot at the tie gives other bits, so an
    implementation that decides the tie differently shows in x, y or s of a kept keypoint."""
    edge_thr = di.thresholds("default")[2]
    for which in ("xy", "xs", "ys_gt", "a47"):
        st = di.pivot(which, edge_thr)
        assert st.exit == di.KEPT and set(st.bits) == {"b0", "b1", "b2"}, which   # under the defaults every one reaches the solve
        L, R = di.build(13, 13, [di.Site("pivot", st, 0, 6, 6)], 1)
        A, b = di.local_system(R, 0, 6, 6)
        dxx, dxy, dxs = abs(A[0]), abs(A[1]), abs(A[2])
        if which == "xy": assert dxx == dxy > dxs
        if which == "xs": assert dxx == dxs > dxy
        if which == "ys_gt": assert dxy == dxs > dxx
        if which == "a47":
            assert dxx != dxy and dxs != max(dxx, dxy)
            i = 2 if dxs > max(dxx, dxy) else 1 if dxy > dxx else 0
            M = A.reshape(3, 3).copy(); M[[0, i]] = M[[i, 0]]
            a4 = F(M[1, 1] - F(F(M[1, 0] / M[0, 0]) * M[0, 1])); a7 = F(M[2, 1] - F(F(M[2, 0] / M[0, 0]) * M[0, 1]))
            assert abs(a4) == abs(a7) != 0
        ref = di.solve3x3(A, b); alt = di.solve3x3(A, b, di.PIVOT_FLIP[which])
        assert [di.bits(x) for x in ref] == [st.bits["b0"], st.bits["b1"], st.bits["b2"]], which
        assert np.isfinite(alt).all() and [di.bits(x) for x in alt] != [di.bits(x) for x in ref], which
        for other in ("first", "second", "third"):   # the other comparisons are no ties: deciding them the other way changes nothing
            if other != di.PIVOT_FLIP[which]:
                assert np.array_equal(di.solve3x3(A, b, other).view(np.uint32), ref.view(np.uint32)), (which, other)


def test_comb_overfills_a_block(oracle):
    """more than 64 candidates per level in one strip's row: a wavefront's block of 64 slots cannot hold the row"""
    for name, row in (("catalogue70", 62), ("all262", 110)):
        t = _oracle_run(name, "default").trace_i
        for level in (0, 1):
            for strip in (0, 1):
                n = int(((t[:, 0] == level) & (t[:, 1] == row) & (t[:, 2] // 248 == strip)).sum())
                assert n > 64, (name, level, strip, n)


@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("name", di.SCENES)
def test_frame_values_reach_nothing(oracle, name, pset):
    """other garbage on the frame of the response planes: the same trace and the same kept list, bit for bit"""
    a = _oracle_run(name, pset, 1); b = _oracle_run(name, pset, 2)
    assert not np.array_equal(_planes(name, pset, 1)[1], _planes(name, pset, 2)[1])
    for x, y in ((a.f, b.f), (a.i, b.i), (a.trace_i, b.trace_i), (a.trace_u, b.trace_u)):
        assert np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the production chain on the same planes
# ----------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def contexts(ctx):
    """one context per parameter set: the session's for the defaults, one of this module's for the other"""
    import hesaff_amd
    other = hesaff_amd.HesaffContext(_params("ratio4"), device=0)
    yield {"default": ctx, "ratio4": other}
    other.close()


def _assert_equals_oracle(got, runs, what):
    """got = detect_planes' (f, i, image, count); runs = the oracle's run of every image, in order"""
    f, i, image, count = got
    want_f = np.concatenate([r.f[:, :5] for r in runs]); want_i = np.concatenate([r.i for r in runs])
    want_img = np.concatenate([np.full(len(r.i), b, np.int32) for b, r in enumerate(runs)])
    print("%s: %d keypoints (oracle %d), %d candidates" % (what, count, len(want_i), sum(r.n_candidates for r in runs)))
    assert count == len(want_i) == len(i), (what, count, len(want_i))
    assert np.array_equal(image, want_img), what
    assert np.array_equal(i, want_i), (what, np.argwhere((i != want_i).any(axis=1))[:5].tolist())
    ne = np.ascontiguousarray(f).view(np.uint32) != np.ascontiguousarray(want_f).view(np.uint32)
    assert not ne.any(), (what, "rows", np.argwhere(ne.any(axis=1))[:5].reshape(-1).tolist(), f[ne.any(axis=1)][:3], want_f[ne.any(axis=1)][:3],
                          want_i[ne.any(axis=1)][:3])


@gpu
@pytest.mark.parametrize("pset", PSETS)
@pytest.mark.parametrize("name", SINGLE)
def test_detect_planes_equals_the_oracle(contexts, pset, name):
    L, R, _ = _planes(name, pset)
    run = _oracle_run(name, pset)
    assert len(run.i) > 0
    _assert_equals_oracle(contexts[pset].detect_planes(L, R), [run], "%s/%s" % (name, pset))


@gpu
@pytest.mark.parametrize("pset", PSETS)
def test_band_heights_agree(contexts, pset):
    """262 x 510 with bands of 32, 64 and 128 rows (and the plan's own choice): the same sites give the same records"""
    L, R, _ = _planes("all262", pset)
    run = _oracle_run("all262", pset)
    for band in (32, 64, 128, 0):
        _assert_equals_oracle(contexts[pset].detect_planes(L, R, band=band), [run], "all262/%s band %d" % (pset, band))


@gpu
@pytest.mark.parametrize("pset", PSETS)
def test_three_images_are_three_oracle_runs(contexts, pset):
    """images 0 and 2 carry the collisions and the comb, image 1 the positions: the octaveMap is per image and the order image-major"""
    names = ["catalogue70", "positions70", "catalogue70b"]
    L = np.stack([_planes(n, pset)[0] for n in names]); R = np.stack([_planes(n, pset)[1] for n in names])
    runs = [_oracle_run(n, pset) for n in names]
    for band in (0, 32):
        _assert_equals_oracle(contexts[pset].detect_planes(L, R, band=band), runs, "three images/%s band %d" % (pset, band))


@gpu
def test_detect_planes_is_the_image_path(ctx):
    """The planes hesaff_stage_pyramid makes of an image, fed back octave by octave, give hesaff_stage_hessian_keypoints' records of
    that octave: r0, c0, level, type and response as they are, x, y and s once the octave's pixelDistance is divided out (the stage
    takes every set of planes for octave 0)."""
    from hesaff_amd.synth import band_noise_image
    img = band_noise_image(150, 210, seed=11)
    f0, i0, n0 = ctx.hessian_keypoints(img)
    assert n0 == len(i0) > 100
    octaves = ctx.pyramid(img)
    total = 0
    for o, (Ls, Rs) in enumerate(octaves):
        if min(Rs.shape[1:]) <= 2 * di.BORDER + 2:
            continue
        f, i, image, count = ctx.detect_planes(Ls, Rs)
        m = i0[:, 1] == o
        assert count == int(m.sum()), (o, count, int(m.sum()))
        assert not image.any() and not i[:, 1].any()
        assert np.array_equal(i[:, [0, 2, 3, 4]], i0[m][:, [0, 2, 3, 4]]), o
        pd = f0[m][:, 3]
        assert np.all(pd == F(2.0 ** o)) and np.all(f[:, 3] == F(1.0))
        for col in (0, 1, 2):   # pd is a power of two: the division is exact
            assert np.array_equal((f0[m][:, col] / pd).view(np.uint32), f[:, col].view(np.uint32)), (o, col)
        assert np.array_equal(f0[m][:, 4].view(np.uint32), f[:, 4].view(np.uint32)), o
        total += count
    assert total == n0 and (i0[:, 1] > 0).any()


@gpu
def test_detect_planes_argument_errors(ctx):
    import ctypes as C
    import hesaff_amd
    z = np.zeros((5, 13, 13), F)
    for shape in ((5, 12, 13), (5, 13, 12)):
        with pytest.raises(hesaff_amd.HesaffError):
            ctx.detect_planes(np.zeros(shape, F), np.zeros(shape, F))
    for band in (1, 16, 33, 256, -32):
        with pytest.raises(hesaff_amd.HesaffError):
            ctx.detect_planes(z, z, band=band)
    cnt = C.c_int()
    assert ctx.L.hesaff_stage_detect_planes(ctx.h, 1, 13, 13, None, z.ctypes.data, 0, 0, None, None, None, C.byref(cnt)) == -2
    assert ctx.L.hesaff_stage_detect_planes(ctx.h, 1, 13, 13, z.ctypes.data, None, 0, 0, None, None, None, C.byref(cnt)) == -2
    f, i, image, count = ctx.detect_planes(z, z)   # nothing fires on zero planes
    assert count == 0 and len(f) == 0
