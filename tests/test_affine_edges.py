"""The affine shape iteration (hs_affine_groups behind k_affine / k_affine_stage, hs_affine_tail, hs_inv_sqrt, hs_eigenvalues,
hs_rectify) on constructed inputs at the edges of its domain (tests/affine_inputs.py).

CPU half (no GPU): the oracle's trace of findAffineShape proves that every input takes the exit it was built for, that the trace
ends in findAffineShape's own result, that the scaled and threshold families are what they claim, and that the parameter sets change
what they were chosen to change; the production records are pinned to the compiled reference.
GPU half (marked): pure equalities.  Every row - converged or not - against the trace's U at the exit, bit for bit (+0 and -0 alike;
where the oracle's U is NaN the same elements are NaN and nothing more is asserted), one context per parameter set; the tail and
rectify on operands; the same positions through hesaff_describe_regions."""
import numpy as np
import pytest

import hesaff_amd
from tests import affine_inputs as A

F = np.float32
FROM_POINTS = 1


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _differs(got, want):
    """elementwise: not the same float32 - other bits, unless both are zeros (+0 / -0 are the same value for every later operation)
    or both are NaN (nothing is claimed about a NaN's bits)"""
    got = np.ascontiguousarray(got, F); want = np.ascontiguousarray(want, F)
    assert got.shape == want.shape
    return (_bits(got) != _bits(want)) & ~((got == 0) & (want == 0)) & ~(np.isnan(got) & np.isnan(want))


@pytest.fixture(scope="module")
def traces(oracle):
    """pset -> case name -> the oracle's trace under that parameter set: computed once, left unchanged"""
    P = A.planes()
    out = {}
    for pset, kw in A.PSETS.items():
        h = oracle.OracleHandle(_params(**kw))
        out[pset] = {c.name: h.affine_trace(P[c.plane], *c.kp) for c in A.cases()}
    return out


# ------------------------------------------------------------------ CPU ------------------------------------------------------------------

def test_claims_hold_in_the_trace(oracle, traces):
    """Every case leaves findAffineShape the way it claims, after the iterations it claims, with the taps outside, the exact U or the
    NaN U it claims; and every finite tap coordinate of every trace, under every parameter set, is below 2^31 in magnitude - beyond
    that the reference's (int) floor(w) is undefined and the oracle would stop being a reference."""
    assert 100 <= len(A.cases()) <= 400 and max(p.size for p in A.planes().values()) <= 64 * 64
    for c in A.cases():
        t = traces["default"][c.name]
        assert (t.kind, t.n_iter) == (c.kind, c.n_iter), (c, oracle.AX_NAMES[t.kind], t.n_iter)
        assert len(t.state) == t.n_iter
        if c.outside is not None:
            assert tuple(t.outside.tolist()) == tuple(c.outside), (c, t.outside)
        if c.U is not None:
            assert np.array_equal(_bits(t.U), _bits(np.array(c.U, F))), (c, t.U)
        assert bool(np.isnan(t.U).all()) == c.nan_U and bool(np.isnan(t.U).any()) == c.nan_U, (c, t.U)
        if c.family == "nonfinite":
            assert (t.outside == 361).all()
    for pset in A.PSETS:
        for c in A.cases():
            assert traces[pset][c.name].max_coord.max() < 2.0 ** 31, (pset, c)


def test_trace_ends_in_find_affine_shape(oracle, traces):
    """The trace is a restatement, not a second opinion: under every parameter set it ends in ho_h_find_affine_shape's result."""
    P = A.planes()
    for pset, kw in A.PSETS.items():
        h = oracle.OracleHandle(_params(**kw))
        for c in A.cases():
            conv, U, it = h.find_affine_shape(P[c.plane], *c.kp)
            wc, wU, wi = traces[pset][c.name].result()
            assert (conv, it) == (wc, wi) and np.array_equal(_bits(U), _bits(wU)), (pset, c)


def test_scaled_family(traces):
    t = traces["default"]
    t0 = t["scaled/0"]
    assert t0.kind == A.CONVERGED and len(A.SCALED_SAME) >= 6
    for k in A.SCALED_SAME:
        assert np.array_equal(_bits(t["scaled/%d" % k].U), _bits(t0.U)), k
        assert t["scaled/%d" % k].n_iter == t0.n_iter
    # the denormal range: the sums of iteration 0 are within 2^6 of the smallest normal number or below it (the terms a weight of
    # the Gaussian mask makes 2^-7 of the largest are denormal), no two results alike, none like k = 0
    seen = {tuple(_bits(t0.U).tolist())}
    for k in A.SCALED_DENORMAL:
        tk = t["scaled/%d" % k]
        assert 0 < tk.abc_in[0].max() < 2.0 ** -120 and np.isfinite(tk.U).all(), k
        seen.add(tuple(_bits(tk.U).tolist()))
    assert len(A.SCALED_DENORMAL) >= 4 and len(seen) == 1 + len(A.SCALED_DENORMAL)
    # both ends: the sums are zero (or, upwards, infinite), NaN from invSqrt on
    assert min(A.SCALED_GONE) < min(A.SCALED_DENORMAL) and max(A.SCALED_GONE) > max(A.SCALED_SAME)
    for k in A.SCALED_GONE:
        tk = t["scaled/%d" % k]
        assert tk.kind == A.MAX_ITER and np.isnan(tk.U).all()
        assert ((tk.abc_in[0] == 0).all() if k <= -100 else (tk.abc_in[0] == 0).any()) if k < 0 else not np.isfinite(tk.abc_in[0]).all(), k
    # the first k beyond each end of the finite range
    assert min(A.SCALED_DENORMAL) - 1 in A.SCALED_GONE and max(A.SCALED_SAME) + 1 in A.SCALED_GONE


def test_threshold_pairs(traces):
    """The two planes of a pair come from adjacent float32 values of the family's parameter; up to the deciding iteration both take
    the same decisions, there the deciding quantity lies on either side of its threshold."""
    t = traces["default"]
    assert set(A.THRESHOLD) == set(A.THRESHOLD_AT) and {k[0] for k in A.THRESHOLD} == {"a", "b", "c"}
    for key, (theta, sx, kp, lo, claims) in A.THRESHOLD.items():
        p0, p1 = A.from_bits(lo), A.from_bits(lo + 1)
        assert p0 < p1 and np.nextafter(p0, F(np.inf)) == p1
        assert not np.array_equal(A.blob(p0, theta, sx), A.blob(p1, theta, sx))
        below, above = t["threshold/%s/0" % key], t["threshold/%s/1" % key]
        assert ((below.kind, below.n_iter), (above.kind, above.n_iter)) == claims and claims[0] != claims[1]
        at, what = A.THRESHOLD_AT[key]
        assert np.array_equal(below.state[:at], above.state[:at]) and (below.state[:at] == 0).all()
        if what == "ratio":
            assert below.ratio[at] < A.THR <= above.ratio[at], (key, below.ratio[at], above.ratio[at])
            assert above.ratio[at] - below.ratio[at] < 2e-6
            # below: converged in this iteration (l = 0: eigen_ratio_bef is 0), else in the next one (this ratio is then the one before)
            assert below.kind == A.CONVERGED and below.n_iter - 1 == (at if at == 0 else at + 1)
            assert not (above.kind == A.CONVERGED and above.n_iter <= below.n_iter)
        else:
            qb, qa = below.ev[at, 0] / below.ev[at, 1], above.ev[at, 0] / above.ev[at, 1]
            assert qb <= F(6) < qa and qa - qb < 1e-4, (key, qb, qa)
            assert below.state[at] == 0 and above.state[at] == 2
    # (a) converged or one more iteration; (c) converged in the last iteration allowed, or never
    assert t["threshold/a/l=3/1"].n_iter == t["threshold/a/l=3/0"].n_iter + 1
    assert t["threshold/c/0"].n_iter == A.MAX_ITERATIONS and t["threshold/c/0"].kind == A.CONVERGED and t["threshold/c/1"].kind == A.MAX_ITER


def test_exact_operands(traces):
    t = traces["default"]
    a, b, c = t["exact/spike"].abc_in[0]
    assert b == 0 and a == c and a > 0
    a, b, c = t["exact/spike/off"].abc_in[0]
    assert b == 0 and a != c and a > 0 and c > 0
    a, b, c = t["limits/s=2^20"].abc_in[0]
    assert b == 0 and a == c and a > 0
    for name in ("flat/ramp_x/2", "flat/ramp_x/3"):
        a, b, c = t[name].abc_in[0]
        assert a > 0 and b == 0 and c == 0, name
    for name in ("flat/const/0", "flat/zero/1", "flat/unreached/4", "flat/unreached/5", "limits/pos/x+", "limits/s=0"):
        assert (t[name].abc_in[0] == 0).all(), name
    assert np.array_equal(t["anisotropic/6"].abc_in[0][:2], np.zeros(2, F)) and t["anisotropic/6"].abc_in[0][2] > 0
    assert 0 < abs(t["exact/paraboloid"].abc_in[0][1]) < 1e-6


def test_every_exit_occurs(oracle, traces):
    kinds = [t.kind for t in traces["default"].values()]
    assert all(kinds.count(k) >= 4 for k in (A.CONVERGED, A.NO_REAL_EIGEN, A.ANISOTROPY, A.MAX_ITER))
    an = sorted(t.n_iter for n, t in traces["default"].items() if n.startswith("anisotropic/") and t.kind == A.ANISOTROPY)
    assert an[:2] == [1, 2] and an[-1] > 2
    # MAX_ITER with a finite U as well as through the NaN flow
    assert any(t.kind == A.MAX_ITER and np.isfinite(t.U).all() for t in traces["default"].values())
    # the scan that found the NO_REAL_EIGEN blobs: its budget and its yield
    h = oracle.OracleHandle()
    scan = list(A.no_real_eigen_scan())
    found = [(theta, sx, float(p), kp) for theta, sx, p, kp in scan if h.affine_trace(A.blob(p, theta, sx), *kp).kind == A.NO_REAL_EIGEN]
    assert len(scan) == 1800 and len(found) == 9
    for theta, sx, p, kp, claim in A.NO_REAL_EIGEN_BLOBS:
        assert any(f[0] == theta and f[1] == sx and F(f[2]) == F(p) and f[3] == kp for f in found), (theta, sx, p, kp)


def test_parameter_sets_change_what_they_were_chosen_to_change(traces):
    d = traces["default"]
    names = [c.name for c in A.cases()]
    finite0 = [n for n in names if np.isfinite(d[n].ratio[0])]
    assert len(finite0) > 60
    # maxIterations = 1, 2: nothing enters more iterations; what converged at l = 0 still does, everything that went on is cut short
    for pset, m in (("maxit1", 1), ("maxit2", 2)):
        t = traces[pset]
        assert all(t[n].n_iter == min(d[n].n_iter, m) for n in names)
        assert all((t[n].kind == d[n].kind) if d[n].n_iter <= m else (t[n].kind == A.MAX_ITER) for n in names)
        assert sum(t[n].kind == A.MAX_ITER and np.isfinite(t[n].U).all() for n in names) > 30
    assert sum(traces["maxit1"][n].kind == A.CONVERGED for n in names) >= 8
    # (no keypoint converges at l = 1: eigen_ratio_bef would have let it converge at l = 0)
    assert not any(t.kind == A.CONVERGED and t.n_iter == 2 for ps in traces.values() for t in ps.values())
    # maxIterations = 40: the same up to sixteen iterations; of those that ran out of iterations with a finite U, some now converge
    t = traces["maxit40"]
    ran_out = [n for n in names if d[n].kind == A.MAX_ITER and np.isfinite(d[n].U).all()]
    assert all(t[n].n_iter > 16 for n in ran_out) and any(t[n].kind == A.CONVERGED for n in ran_out)
    assert all((t[n].kind, t[n].n_iter) == (d[n].kind, d[n].n_iter) for n in names if d[n].kind != A.MAX_ITER)
    assert max(t[n].n_iter for n in names) == 40
    # convergenceThreshold = 0: nothing converges; every keypoint runs out of iterations or takes one of the two other exits
    t = traces["thr0"]
    assert not any(t[n].kind == A.CONVERGED for n in names)
    assert {t[n].kind for n in names} == {A.MAX_ITER, A.ANISOTROPY, A.NO_REAL_EIGEN}
    # convergenceThreshold = 1: 1 - l2 / l1 < 1 for every finite l1 >= l2 > 0, so whatever is finite leaves in iteration 0
    t = traces["thr1"]
    for n in names:
        if n in finite0:
            assert t[n].n_iter == 1 and t[n].kind in (A.CONVERGED, A.ANISOTROPY), n
            assert (t[n].kind == A.ANISOTROPY) == (d[n].state[0] == 2)
        else:
            assert t[n].kind == A.MAX_ITER and np.isnan(t[n].U).all(), n
    assert sum(t[n].kind == A.CONVERGED for n in names) > 60


def test_mixed_lists_are_what_they_say(traces):
    d = traces["default"]
    L = A.mixed_lists()
    odd, ordinary = set(A.ODD), {"ordinary/%d" % j for j in range(len(A.ORDINARY))}
    assert all(A.case(n).plane == "blobs*2^0" for n in odd | ordinary)
    assert all(d[n].kind == A.CONVERGED for n in ordinary) and all(d[n].kind == A.MAX_ITER and np.isnan(d[n].U).all() for n in odd)
    assert len({d[n].n_iter for n in ordinary}) >= 2
    for j in range(4):
        rows = L["batch/%d" % j]
        assert len(rows) == A.SLOTS
        for q in range(4):
            four = rows[4 * q:4 * q + 4]
            assert [n in odd for n in four] == [t == j for t in range(4)], (j, q)
        assert L["batch/%d/short" % j] == rows[:-2]
    rows = L["refill"]
    assert len(rows) == A.BIG_ROWS == 2 * A.SLOTS * A.STAGE_BLOCKS and A.STAGE_BLOCKS % 8 == 0
    pos = np.array([A.big_position(r) for r in range(len(rows))])
    is_odd = np.array([n in odd for n in rows])
    assert pos.max() == 2 * A.SLOTS - 1 and (np.bincount(pos) == A.STAGE_BLOCKS).all()
    assert not is_odd[pos < A.SLOTS].any() and is_odd[pos == A.SLOTS].all()
    assert set(np.unique(pos[is_odd]).tolist()) == {16, 20, 24, 28}
    assert {n for n in rows} == odd | ordinary


# ---- the tail and rectify on operands: the rows of the GPU half, and what the oracle makes of them ----

def tail_operands():
    """abc[n,3], U[n,4], ratio_bef[n]: about 10^5 seeded random rows, then the constructed ones"""
    rng = np.random.default_rng(20260)
    n = 100000
    # symmetric positive definite [a b; b c] over forty orders of magnitude, b on either side; a tenth indefinite
    a = np.exp(rng.uniform(np.log(1e-20), np.log(1e20), n)); c = a * np.exp(rng.uniform(-4, 4, n))
    b = np.sqrt(a * c) * rng.uniform(-0.999, 0.999, n) * np.where(rng.uniform(size=n) < 0.1, 1.2, 1.0)
    th = rng.uniform(0, 2 * np.pi, n); r = rng.uniform(1.0, 7.0, n); f = np.exp(rng.uniform(-1, 1, n))
    U = np.stack([f * np.cos(th), -f * np.sin(th) / r, f * np.sin(th), f * np.cos(th) / r], 1)
    U[: n // 2] = np.stack([f, 0.1 * np.sin(th), 0.1 * np.cos(th), f / r], 1)[: n // 2]    # the iteration's own: near a positive diagonal
    abc = [np.stack([a, b, c], 1).astype(F)]; Us = [U.astype(F)]; ratio = [rng.uniform(0.0, 0.1, n).astype(F)]
    # any bit pattern at all (NaN, infinities, denormals)
    m = 20000
    abc.append(rng.integers(0, 2 ** 32, (m, 3), dtype=np.uint64).astype(np.uint32).view(F))
    Us.append(rng.integers(0, 2 ** 32, (m, 4), dtype=np.uint64).astype(np.uint32).view(F))
    ratio.append(rng.integers(0, 2 ** 32, m, dtype=np.uint64).astype(np.uint32).view(F))
    rows = []
    I = (1.0, 0.0, 0.0, 1.0)
    rot = lambda t: (np.cos(t), -np.sin(t), np.sin(t), np.cos(t))
    den = A.from_bits(1)   # the smallest denormal
    thr_lo, thr_hi = A.from_bits(A.bits(A.THR) - 1), A.from_bits(A.bits(A.THR) + 1)
    for rb in (0.0, thr_lo, A.THR, thr_hi, 0.04, 0.06):
        for u in (I, (1.2, -0.17, -0.17, 0.85)):
            rows += [((1.0, 0.0, 1.0), u, rb), ((1.0, 0.0, 1.0005), u, rb), ((1.0, 0.0, 1.2), u, rb)]            # b = 0: r = 1, t = 0
            rows += [((1.0, den, 1.0005), u, rb), ((1.0, -den, 1.0005), u, rb), ((1.0, den, 1.0), u, rb)]        # b = +- the smallest denormal
            rows += [((2.0, 0.5, 2.0), u, rb), ((2.0, -0.5, 2.0), u, rb), ((3.0, 1e-3, 3.0), u, rb)]            # c == a: r = 0
            rows += [((0.0, 0.5, 0.0), u, rb), ((0.0, 0.0, 0.0), u, rb), ((0.0, 0.0, 1.0), u, rb), ((1.0, 0.0, 0.0), u, rb), ((-0.0, -0.0, -0.0), u, rb)]
            rows += [((1.0, A.from_bits(A.bits(F(1)) + 1), 1.0), u, rb), ((1.0, A.from_bits(A.bits(F(1)) - 1), 1.0), u, rb), ((1.0, 1.0, 1.0), u, rb)]
            rows += [((4.0, -A.from_bits(A.bits(F(2)) + 1), 1.0), u, rb), ((-1.0, 0.0, 1.0), u, rb), ((1.0, 0.0, -1.0), u, rb)]
    for e in range(-149, 43):                                   # the denormal range up to 2^42, the largest a 2^20 image gives
        for q in (1.0, 1.0005, 1.7):
            a_ = 2.0 ** e; c_ = min(a_ * q, 2.0 ** 42)
            rows += [((a_, 0.3 * np.sqrt(a_ * c_), c_), I, 0.0), ((a_, 0.0, c_), I, 0.04), ((a_, -0.9 * np.sqrt(a_ * c_), c_), (1.1, 0.1, 0.1, 0.9), 0.0)]
    for k in range(0, 360, 15):                                 # rotations: 90 degrees gives delta1 < 0 directly
        rows += [((1.0, 0.0, 1.0), rot(np.radians(k)), 0.0), ((1.3, 0.2, 0.8), rot(np.radians(k)), 0.01)]
    for k in range(-6, 7):                                      # l1 / l2 of U within a few float32 steps of 6, on both sides
        d = A.from_bits(A.bits(F(6)) + k)
        rows += [((1.0, 0.0, 1.0), (d, 0.0, 0.0, 1.0), 0.0), ((1.0, 0.0, 1.0), (1.0, 0.0, 0.0, d), 0.0), ((1.0, 0.0, 1.0), (2 * d, 0.0, 0.0, 2.0), 0.04),
                 ((1.0, 0.0, 1.0), (1.0 / d, 0.0, 0.0, 1.0), 0.0)]
    abc.append(np.array([r[0] for r in rows], np.float64).astype(F)); Us.append(np.array([r[1] for r in rows], np.float64).astype(F))
    ratio.append(np.array([r[2] for r in rows], np.float64).astype(F))
    return np.concatenate(abc), np.concatenate(Us), np.concatenate(ratio)


def rectify_operands(traces):
    rng = np.random.default_rng(20261)
    n = 100000
    th = rng.uniform(0, 2 * np.pi, n); r = rng.uniform(1.0, 7.0, n); f = np.exp(rng.uniform(-3, 3, n)); sgn = np.where(rng.uniform(size=n) < 0.3, -1.0, 1.0)
    th2 = rng.uniform(0, 2 * np.pi, n)
    c1, s1, c2, s2 = np.cos(th), np.sin(th), np.cos(th2), np.sin(th2)
    d1, d2 = f, sgn * f / r
    Us = [np.stack([c1 * d1 * c2 - s1 * d2 * s2, -c1 * d1 * s2 - s1 * d2 * c2, s1 * d1 * c2 + c1 * d2 * s2, -s1 * d1 * s2 + c1 * d2 * c2], 1).astype(F)]
    Us.append(rng.integers(0, 2 ** 32, (20000, 4), dtype=np.uint64).astype(np.uint32).view(F))
    rows = []
    for k in range(0, 360, 5):
        t = np.radians(k)
        rows += [(np.cos(t), -np.sin(t), np.sin(t), np.cos(t)), (np.cos(t), np.sin(t), np.sin(t), -np.cos(t)), (2 * np.cos(t), -np.sin(t), 2 * np.sin(t), np.cos(t))]
    T, den = 2.0 ** 20, float(A.from_bits(1))
    rows += [(T, T, -T, T), (T, 0, 0, T), (T, -T, T, T), (T, T, T, -T), (T, 0, 0, den), (den, 0, 0, T), (0, T, -T, 0), (T, T, T, T), (T, T, T, float(np.nextafter(F(T), F(0))))]
    # a11^2 + a12^2 and the determinant at the smallest values hesaff_describe_regions accepts (non-zero in double), and at zero
    rows += [(den, 0, 0, den), (den, 0, 0, 1), (1, 0, 0, den), (0, den, den, 0), (0, den, -den, 0), (den, den, -den, den), (den, 0, 1, 1), (0, den, 1, 0),
             (1, 1, 1, float(np.nextafter(F(1), F(2)))), (0, 0, 0, 0), (0, 0, 1, 1), (1, 2, 2, 4), (1, 0, 0, 0), (-0.0, 0, 0, 1)]
    Us.append(np.array(rows, np.float64).astype(F))
    # every U the constructed cases converged to, under every parameter set
    Us.append(np.array([t.U for ps in traces.values() for t in ps.values() if t.kind == A.CONVERGED], F))
    return np.concatenate(Us)


def test_operand_rows_cover_their_branches(oracle, traces):
    """the tail's operands reach every state and both branches of invSqrt; the oracle's tail agrees with its trace on every iteration
    of every case, so ho_affine_tail is the loop's own tail"""
    abc, U, rb = tail_operands()
    o = oracle.affine_tail(abc, U, rb, A.THR)
    assert 1.2e5 < len(abc) < 1.4e5
    assert all((o[4] == s).sum() > 200 for s in range(4)), np.bincount(o[4])
    assert (abc[:, 1] == 0).sum() > 200 and (np.abs(abc[:, 1]) == A.from_bits(1)).sum() >= 30 and ((abc[:, 0] == abc[:, 2]) & (abc[:, 1] != 0)).sum() >= 30
    assert np.isnan(o[0]).any(axis=1).sum() > 1000 and np.isfinite(o[0]).all(axis=1).sum() > 90000
    with np.errstate(all="ignore"):
        q = o[3][:, 2] / o[3][:, 3]
    near6 = np.abs(q - 6) < 1e-5
    assert (near6 & (o[4] == oracle.AT_ANISOTROPY)).sum() >= 6 and (near6 & (o[4] != oracle.AT_ANISOTROPY)).sum() >= 6
    # the comparisons are strict: l1 / l2 == 6 exactly goes on, eigen_ratio_bef == convergenceThreshold exactly does not converge
    assert ((q == 6) & (o[4] != oracle.AT_ANISOTROPY)).sum() >= 3
    assert ((rb == A.THR) & (o[2] < A.THR) & (o[4] == oracle.AT_CONTINUE)).sum() >= 3
    for pset, kw in A.PSETS.items():
        thr = F(kw.get("convergenceThreshold", A.THR))
        rows = [(t, i) for t in traces[pset].values() for i in range(len(t.state))]
        abc = np.array([t.abc_in[i] for t, i in rows], F)
        Ub = np.array([t.Us[i - 1] if i else (1, 0, 0, 1) for t, i in rows], F)
        rbef = np.array([t.ratio[i - 1] if i else 0 for t, i in rows], F)
        a2, U2, r2, l2, st = oracle.affine_tail(abc, Ub, rbef, thr)
        assert not _differs(a2, np.array([t.abc[i] for t, i in rows], F)).any()
        assert not _differs(U2, np.array([t.Us[i] for t, i in rows], F)).any()
        assert not _differs(r2, np.array([t.ratio[i] for t, i in rows], F)).any()
        assert not _differs(l2[:, :2], np.array([t.l[i] for t, i in rows], F)).any() and not _differs(l2[:, 2:], np.array([t.ev[i] for t, i in rows], F)).any()
        assert np.array_equal(st, np.array([t.state[i] for t, i in rows]))
    R = rectify_operands(traces)
    with np.errstate(all="ignore"):
        det = R[:, 0].astype(np.float64) * R[:, 3] - R[:, 1].astype(np.float64) * R[:, 2]
    assert (det < 0).sum() > 20000 and (det > 0).sum() > 60000 and (np.abs(R) == 2.0 ** 20).any(axis=1).sum() >= 8


# ---- the production path: the same positions as FROM_POINTS records ----

PROD_H, PROD_W, PROD_OCTAVES = 96, 128, 3


def production_plane():
    """96 x 128: the two blobs, the integer plane beside them (border-exact windows), a ridge and a flat quarter; values 0..255"""
    P = A.planes()
    img = np.zeros((PROD_H, PROD_W), F)
    img[:64, :64] = P["blobs*2^0"]
    img[:64, 64:] = P["integers"]
    img[64:, :64] = A.ridge(0.0, 1.0, 0.1)[16:48, :]
    img[64:, 64:] = 77.0
    return img


def production_records():
    """FROM_POINTS records on every (octave, level): ordinary and border-exact positions, a ridge, the flat quarter, far outside
    (+-2^20), s = 2^20 and the smallest s accepted, in image coordinates (position = plane position * pixelDistance)"""
    REGION = hesaff_amd._binding.REGION_DTYPE
    T = 2.0 ** 20
    rows = []
    for o in range(PROD_OCTAVES):
        pd = 2.0 ** o
        for l in range(3):
            s0 = 1.6 * pd * 2.0 ** (l / 3.0)
            pts = [(x * pd, y * pd, s / 4.0 * s0) for x, y, s, _ in A.ORDINARY]                                       # ordinary, in the blobs
            pts += [(x, y, 1.6 * pd) for x in (9 * pd, 8 * pd, PROD_W - 1 - 9 * pd, PROD_W - 10 * pd) for y in (40.0, 9 * pd)]   # the window on the border
            pts += [(95.0, 30.0, s0), (70.5, 20.25, 1.2 * s0), (100.0, 50.0, 0.8 * s0), (80.0, 40.0, 2.0 * s0)]            # ordinary, in the integer plane
            pts += [(32.3, 79.2, s0), (31.0, 80.5, 1.5 * s0), (96.0, 80.0, s0), (100.3, 84.1, 2 * s0), (127.0, 95.0, s0), (0.0, 0.0, s0), (-0.0, -0.0, s0)]
            pts += [(T, 32.0, s0), (-T, 32.0, s0), (32.0, T, s0), (32.0, -T, s0), (T, -T, s0), (-T, T, s0)]                # far outside: every tap zero
            pts += [(32.3, 31.2, T), (95.0, 30.0, T), (17.0, 40.0, T), (64.0, 48.0, T), (T, T, T)]                       # s = 2^20: the centre tap alone
            pts += [(32.3, 31.2, float(A.from_bits(1))), (32.3, 31.2, 2.0 ** -21), (95.0, 30.0, 0.25 * pd)]
            rows += [(o, l) + p for p in pts]
    rec = np.zeros(len(rows), REGION)
    for k, (o, l, x, y, s) in enumerate(rows):
        rec[k]["x"], rec[k]["y"], rec[k]["s"], rec[k]["octave"], rec[k]["level"] = x, y, s, o, l
        rec[k]["response"], rec[k]["type"] = 10.0 + k, k % 3
    return rec


def test_production_records_against_the_reference(oracle):
    """The production records through the compiled reference's findAffineShape / normalizeAffine / SIFT (ref_driver's points= path)
    against the oracle's stage functions, as tests/test_reference.py::test_foreign_records pins its records: every field.  All
    coordinates stay far below 2^31 (|x|, |y|, s <= 2^20: at most 9 * 2^20 / 1.6 + 2^20)."""
    from tests import _reference as R
    from tests.test_reference import oracle_foreign
    driver = R.binary("ref_driver")
    grey = production_plane()
    rec = production_records()
    _, labels = R.oracle_records(oracle, grey, {})
    index = {ol: k for k, ol in enumerate(labels)}
    assert len(index) >= 4, labels
    reg = rec[[ol in index for ol in zip(rec["octave"].tolist(), rec["level"].tolist())]]
    points = np.zeros(len(reg), np.dtype(R.POINT_IN.descr + [("octave", "<i4"), ("level", "<i4")]))
    for k in ("x", "y", "s", "octave", "level"):
        points[k] = reg[k]
    points["plane"] = [index[ol] for ol in zip(reg["octave"].tolist(), reg["level"].tolist())]
    pin = np.zeros(len(points), R.POINT_IN)
    for k in R.POINT_IN.names:
        pin[k] = points[k]
    got = R.run_driver(driver, grey, {}, points=pin)
    R.same_records(got, oracle_foreign(oracle, grey, {}, points=points), "production records")
    n = np.bincount(got["fate"], minlength=3)
    print("reference on %d production records: not converged %d, rejected %d, described %d" % (len(got), n[0], n[1], n[2]))
    assert len(got) >= 100 and n.min() >= 10, n


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

def _check_rows(c, plane, kp, want, what):
    """kp rows on one plane through k_affine_stage; want: the trace of every row.  converged, iters and U of EVERY row."""
    conv, U, it = c.find_affine_shape(plane, np.array(kp, F).reshape(-1, 4))
    wc = np.array([t.kind == A.CONVERGED for t in want], np.int32)
    wi = np.array([t.n_iter - 1 if t.kind == A.CONVERGED else 0 for t in want], np.int32)
    wU = np.array([t.U for t in want], F)
    assert np.array_equal(conv, wc), (what, "converged differs, first rows", np.flatnonzero(conv != wc)[:8])
    assert np.array_equal(it, wi), (what, "iters differs, first rows", np.flatnonzero(it != wi)[:8])
    ne = _differs(U, wU).any(axis=1)
    assert not ne.any(), (what, "U differs in %d of %d rows, first %d: %r vs %r" % (ne.sum(), len(ne), np.argmax(ne), U[np.argmax(ne)], wU[np.argmax(ne)]))
    return len(want)


@pytest.mark.gpu
@pytest.mark.parametrize("pset", list(A.PSETS))
def test_every_row_against_the_trace(ctx, traces, pset):
    """One context per parameter set; every case, grouped by plane; no row is left out of the comparison."""
    P = A.planes()
    by_plane = {}
    for c in A.cases():
        by_plane.setdefault(c.plane, []).append(c)
    assert sum(len(v) for v in by_plane.values()) == len(A.cases())
    c2 = ctx if pset == "default" else hesaff_amd.HesaffContext(_params(**A.PSETS[pset]), device=0)
    try:
        done = 0
        for plane, cs in by_plane.items():
            done += _check_rows(c2, P[plane], [c.kp for c in cs], [traces[pset][c.name] for c in cs], "%s on %s: %s" % (pset, plane, [c.name for c in cs]))
        assert done == len(A.cases())
    finally:
        if c2 is not ctx:
            c2.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(A.mixed_lists()))
def test_mixed_orders(ctx, traces, name):
    """A NaN-flow or far-outside keypoint in each position of every batch of four slots, and refilled into slots whose keypoint
    converged: every row is the trace's of the case it repeats."""
    rows = A.mixed_lists()[name]
    kp = {n: A.case(n).kp for n in set(rows)}
    assert _check_rows(ctx, A.planes()["blobs*2^0"], [kp[n] for n in rows], [traces["default"][n] for n in rows], name) == len(rows)


@pytest.mark.gpu
def test_affine_tail_on_operands(ctx, oracle):
    abc, U, rb = tail_operands()
    want = oracle.affine_tail(abc, U, rb, A.THR)
    got = ctx.affine_tail(abc, U, rb)
    for g, w, what in zip(got[:4], want[:4], ("a, b, c", "U", "eigen_ratio_act", "l1, l2")):
        ne = _differs(g.reshape(len(abc), -1), w.reshape(len(abc), -1)).any(axis=1)
        i = int(np.argmax(ne))
        assert not ne.any(), "%s differs in %d rows, first %d: abc %r U %r ratio_bef %r -> %r, expected %r" % (what, ne.sum(), i, abc[i], U[i], rb[i], g[i], w[i])
    # 0 continue, 1 break (either exit), 2 converged
    ws = np.array([0, 1, 1, 2], np.int32)[want[4]]
    assert np.array_equal(got[4], ws), np.flatnonzero(got[4] != ws)[:8]


@pytest.mark.gpu
def test_rectify_on_operands(ctx, oracle, traces):
    R = rectify_operands(traces)
    want = R.copy()
    for k in range(len(want)):
        oracle.lib().ho_rectify(want[k])
    got = ctx.rectify(R)
    ne = _differs(got, want).any(axis=1)
    i = int(np.argmax(ne))
    assert not ne.any(), "rectify differs in %d of %d rows, first %d: %r -> %r, expected %r" % (ne.sum(), len(R), i, R[i], got[i], want[i])


@pytest.mark.gpu
@pytest.mark.parametrize("dim", [0, -66], ids=["plain", "times2^-66"])
def test_production_path(ctx, oracle, dim):
    """The same positions as FROM_POINTS records through hesaff_describe_regions_f32 on a float image, and on the image times 2^-66,
    which takes the pyramid kernels into the denormal range as well: every field of every record is the oracle's."""
    from tests.test_describe_regions import _same_records, check_foreign, oracle_describe, outcome_counts
    plane = A.scaled(production_plane(), dim)
    rec = production_records()
    assert set(zip(rec["octave"].tolist(), rec["level"].tolist())) == {(o, l) for o in range(PROD_OCTAVES) for l in range(3)}
    describe = lambda r: ctx.describe_regions_f32([plane], [r], FROM_POINTS)[0]
    if dim == 0:
        check_foreign(describe, oracle, plane, rec, FROM_POINTS, "production records")   # (at least 20 of each outcome)
    else:
        # (the dim image: by the oracle fewer keypoints converge; the comparison is check_foreign's without its counts)
        want_r, want_k = oracle_describe(oracle, plane, rec, FROM_POINTS)
        got_r, got_k = describe(rec)
        print("production records, image * 2^%d: %d records, by the oracle %s" % (dim, len(rec), outcome_counts(want_r)))
        _same_records(got_r, want_r, "dim production records: regions")
        _same_records(got_k, want_k, "dim production records: keys")
