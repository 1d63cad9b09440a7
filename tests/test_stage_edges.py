"""Descriptor and patch kernels on constructed inputs at the edges of their domains (tests/stage_inputs.py).

CPU half (no mark): the oracle alone proves that every input hits what it claims -- which body of k_sift_grad a patch
takes, which operands reach atan2f, which window kernel a record selects -- so that the inputs cannot rot.
GPU half (pytest.mark.gpu): the same inputs through hesaff_stage_sift_parts, hesaff_stage_math_sift_general and
hesaff_stage_normalize_affine, bit for bit against the oracle: mean / variance and the un-normalised histogram as well as
the descriptor bytes, because a one-ulp error in the former almost never moves a byte.
"""
import functools

import numpy as np
import pytest

from tests import stage_inputs as si

F = np.float32
gpu = pytest.mark.gpu
FAMILIES = ("flat", "threshold", "saturating", "ordinary")


def _bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def assert_same_bits(got, want, what, zero_signs=True):
    """Bit equality of float32 arrays; zero_signs=False lets +0 equal -0 (the same value for every later operation)."""
    got = np.ascontiguousarray(got, F); want = np.ascontiguousarray(want, F)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = _bits(got) != _bits(want)
    if not zero_signs:
        ne &= ~((got == 0) & (want == 0))
    if ne.any():
        idx = np.argwhere(ne)[:5]
        raise AssertionError("%s: %d of %d floats differ, first at %s: %r (%08x) vs %r (%08x)" % (
            what, int(ne.sum()), got.size, idx.tolist(), got[tuple(idx[0])], _bits(got)[tuple(idx[0])],
            want[tuple(idx[0])], _bits(want)[tuple(idx[0])]))


def _family(name):
    return getattr(si, name)()


@functools.lru_cache(maxsize=None)
def _oracle_parts_of(name):
    """The oracle's (meanvar [k][2], hist [k][128], desc [k][128]) of a family or of 'interleaved:<n>'; computed once."""
    from tests import _oracle
    oh = _oracle.OracleHandle()
    patches = si.interleaved(int(name.split(":")[1])) if name.startswith("interleaved:") else _family(name)
    res = [oh.sift_parts(p) for p in patches]
    out = tuple(np.stack([r[j] for r in res]) for j in range(3))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _oracle_windows():
    """The oracle's normalizeAffine of every record of the window list: (rejected [n], patches [n][41][41])."""
    from tests import _oracle
    oh = _oracle.OracleHandle()
    gray = _oracle.gray_from_u8(si.window_image())
    kp, A, _, _ = si.windows()
    res = [oh.normalize_affine(gray, kp[k, 0], kp[k, 1], kp[k, 2], A[k]) for k in range(len(kp))]
    rej = np.array([r for r, _ in res]); patches = np.stack([p for _, p in res])
    rej.setflags(write=False); patches.setflags(write=False)
    return rej, patches


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the inputs hit what they claim
# ----------------------------------------------------------------------------------------------------------------------

def test_oracle_parts_end_in_the_descriptor_of_compute_sift_descriptor(oracle):
    """ho_h_sift_parts restates computeSiftDescriptor to expose its intermediate values: on every constructed patch its
    final vector is ho_h_sift's, and its mean / var are numpy's of the same sequential float32 sums."""
    oh = oracle.OracleHandle()
    m = si.circular_mask().reshape(-1)
    for name in FAMILIES:
        mv, hist, desc = _oracle_parts_of(name)
        for k, p in enumerate(_family(name)):
            assert np.array_equal(desc[k], oh.sift(p)), (name, k)
        assert np.isfinite(hist).all() and (hist >= 0).all(), name
    # mean and var by hand for a few patches of each body
    for p, (mean, var) in [(si.flat()[0], _oracle_parts_of("flat")[0][0]), (si.ordinary()[3], _oracle_parts_of("ordinary")[0][3])]:
        v = p.reshape(-1)[m]
        s = F(0)
        for x in v:
            s = F(s + x)
        mu = F(s / F(len(v)))
        q = F(0)
        for x in v:
            d = F(mu - x); q = F(q + F(d * d))
        assert mu == mean and np.sqrt(F(q / F(len(v)))) == var


def test_families_take_the_body_they_claim():
    """var < 1e-4 (helpers.cpp:270, the float32 var against the double constant) for every patch of `flat`, var >= 1e-4 for
    `saturating` and `ordinary`, both sides for `threshold`: bisection over the scale's bit pattern reaches var within 3
    float32 steps of fl(1e-4) on either side (64 allowed)."""
    assert all(si.is_flat_var(v) for v in _oracle_parts_of("flat")[0][:, 1])
    for name in ("saturating", "ordinary"):
        assert not any(si.is_flat_var(v) for v in _oracle_parts_of(name)[0][:, 1]), name
    assert len(si.ordinary()) == 200
    names = si.threshold_names(); var = _oracle_parts_of("threshold")[0][:, 1]
    assert np.array_equal(var, si.threshold_vars())
    below = [si.is_flat_var(v) for v in var]
    assert below == [nm.split(":")[1] == "below" for nm in names] and sum(below) == 2 and len(below) == 4
    steps = np.abs(_bits(var).astype(np.int64) - int(si.THRESHOLD_VAR.view(np.uint32)))
    assert steps.max() <= 64, steps
    # fl(1e-4) itself is below the double constant: a var equal to it is still flat
    assert si.is_flat_var(si.THRESHOLD_VAR) and not si.is_flat_var(np.nextafter(si.THRESHOLD_VAR, F(1)))


def test_flat_patches_by_group():
    """What the flat body produces, by the oracle: a full descriptor down to 2^-70 (and for the offsets whose pattern
    survives the rounding at the offset), a different one where the squared gradients underflow (2^-74 .. 2^-76),
    nothing from 2^-100 down, from constants and from content that no masked pixel's stencil reaches."""
    names = si.flat_names(); desc = _oracle_parts_of("flat")[2]
    by = dict(zip(names, desc))
    for nm, d in by.items():
        kind = nm.split(":")
        if kind[0] == "scale":
            e = int(kind[1])
            if e >= -70:
                assert (d > 0).sum() >= 100, nm
            if e in (-74, -75, -76):
                assert not np.array_equal(d, by["scale:-70:" + kind[2]]), nm
            if e <= -100:
                assert not d.any(), nm
        elif kind[0] == "offset":
            # ulp(100) = 2^-17 and ulp(255) = 2^-16 swallow a 2^-20 pattern whole: constants; every other offset keeps >= 100 bytes
            if kind[1] in ("100", "255") and kind[2] == "-20":
                assert not d.any(), nm
            else:
                assert (d > 0).sum() >= 100, nm
        elif kind[0] == "const" or kind[:2] == ["outside", "silent"] or nm.startswith("outside:spike:21"):
            assert not d.any(), nm
        elif kind[0] == "gap" or nm in ("outside:frame", "outside:spike:20:x", "outside:spike:20:y"):
            assert d.any(), nm
        else:
            raise AssertionError("unclassified flat patch " + nm)
    assert sorted({int(nm.split(":")[1]) for nm in names if nm.startswith("scale")}) == sorted(si.FLAT_EXPONENTS)
    assert sum(nm.startswith("const") for nm in names) == len(si.FLAT_CONSTANTS)
    # the checkerboard of period 1 has 0/0 at every interior pixel: an all-zero histogram, 0 * inf = NaN -> 0 in the quantiser
    k = si.saturating_names().index("checker:1")
    assert not _oracle_parts_of("saturating")[1][k].any() and not _oracle_parts_of("saturating")[2][k].any()


def _exponent(v):
    return ((_bits(v) >> 23) & 0xff).astype(np.int64)


def test_gradient_operands_cover_the_special_cases():
    """The gap patches hold masked pixels whose gy and gx lie more than 60 binades apart (hm_atan2f_rare) in both
    directions and with gx == 0; the saturating patches hold every exact case of atan2f."""
    names = si.flat_names()
    gaps = si.flat()[[i for i, nm in enumerate(names) if nm.startswith("gap")]]
    assert len(gaps) == 4
    for p in gaps:
        gy, gx = si.masked_gradients(p)
        both = (gy != 0) & (gx != 0)
        k = _exponent(gy) - _exponent(gx)
        assert (both & (k > 60)).any() and (both & (k < -60)).any()
        assert ((np.abs(gy) == F(2.0 ** -9)) & (gx == 0)).any()
        assert ((np.abs(gx) == F(2.0 ** -9)) & (gy != 0) & (np.abs(gy) < F(2.0 ** -90))).any()
    gy, gx = si.masked_gradients(si.saturating())
    assert ((gx == 0) & (gy == 0)).any()
    assert ((gx == 0) & (gy > 0)).any() and ((gx == 0) & (gy < 0)).any()
    assert ((gy == 0) & (gx < 0)).any() and ((gy == 0) & (gx > 0)).any()
    for sy in (1, -1):
        for sx in (1, -1):
            assert ((np.abs(gy) == np.abs(gx)) & (sy * gy > 0) & (sx * gx > 0)).any(), (sy, sx)
    # gy = +0 with gx < 0 is atan2f = +pi, the top of the orientation coordinate's range: o = 12 exactly
    assert F((8.0 * (float(F(np.pi)) + 2 * np.pi)) / (2 * np.pi)) == F(12.0)


def test_window_list_reaches_every_kernel_and_remainder():
    kp, A, P0, P = si.windows()
    rej, patches = _oracle_windows()
    assert not rej.any(), P[rej != 0]
    for k in range(len(kp)):
        assert si.window_side(kp[k, 2]) == (P0[k], P0[k] + 2)
    direct = P0 / 41.0 <= 0.4
    assert sorted(P0[direct]) == [13, 15] and 17 in P0 and P[list(P0).index(17)] == 19
    have = set(P[~direct].tolist())
    for lo, hi in si.WINDOW_P_RANGES:
        assert set(range(lo, hi + 1, 2)) <= have, (lo, hi)
    iso = (A == np.array([1, 0, 0, 1], F)).all(axis=1)
    assert have == set(P[iso & ~direct].tolist()) and (~iso).sum() >= len(have) // 4
    # on each side of each cut between two kernels (odd sides only: 41|43, 63|65, 127|129, 511|513, 1279|1281)
    assert {41, 43, 63, 65, 127, 129, 511, 513, 1279, 1281} <= have
    large3 = {p for p in have if 513 <= p <= 1279}; large1 = {p for p in have if p >= 1281}
    # k_patch_large_rows takes 18-row tasks with two-row and one-row remainders; a window side is odd, so P mod 18 is
    # one of the nine odd residues: all of them, in each form
    odd = set(range(1, 18, 2))
    assert {p % 18 for p in large3} == odd and {p % 18 for p in large1} == odd
    for lo, hi in ((65, 127), (129, 511)):
        assert {p % 3 for p in have if lo <= p <= hi} == {0, 1, 2}
    # noise, not a smooth blob: neighbouring patch pixels are unrelated
    assert all(np.unique(p).size > 1000 for p in patches[::10])


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------

def _gradient_operands():
    """(gy, gx) pairs, finite: see test_general_gradient_forms_on_the_device."""
    ys, xs = [], []
    for fam in (si.flat(), si.saturating()):
        gy, gx = si.masked_gradients(fam)
        ys.append(gy); xs.append(gx)
    tiny = np.array(1, np.uint32).view(F); maxsub = np.array(0x007fffff, np.uint32).view(F)
    sp = np.array([0.0, tiny, maxsub, np.finfo(F).tiny, 1.0, np.finfo(F).max], F)
    sp = np.concatenate([sp, -sp])
    ys.append(np.repeat(sp, len(sp))); xs.append(np.tile(sp, len(sp)))
    # quotients on and one ulp either side of fdlibm's interval thresholds and of 2^25
    for t in (0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** 25):
        for x in (1.0, 2.0 ** -100, 2.0 ** 100, 2.0 ** -140, 3.0, 7.0, 1.2345678, 2.0 ** -126):
            x = F(x); y = F(F(t) * x)
            for yy in (np.nextafter(y, F(0)), y, np.nextafter(y, F(np.inf))):
                for sy in (1, -1):
                    for sx in (1, -1):
                        ys.append(np.array([sy * yy], F)); xs.append(np.array([sx * x], F))
    # exponent gaps 59, 60, 61 in both directions, mantissas at both ends of the binade
    lo, hi = F(1.0), np.nextafter(F(2.0), F(0))
    for gap in (59, 60, 61):
        for base in (0, 60, -20, 30, -66):
            for ma in (lo, hi):
                for mb in (lo, hi):
                    a = F(ma * F(2.0) ** F(base)); b = F(mb * F(2.0) ** F(base - gap))
                    for u, v in ((a, b), (b, a)):
                        for sy in (1, -1):
                            for sx in (1, -1):
                                ys.append(np.array([sy * u], F)); xs.append(np.array([sx * v], F))
    gy = np.concatenate(ys).astype(F); gx = np.concatenate(xs).astype(F)
    assert np.isfinite(gy).all() and np.isfinite(gx).all()
    # each distinct pair once (the constants alone give six thousand (0, 0))
    key = (_bits(gy).astype(np.uint64) << np.uint64(32)) | _bits(gx).astype(np.uint64)
    _, first = np.unique(key, return_index=True)
    first.sort()
    return gy[first].copy(), gx[first].copy()


@gpu
def test_general_gradient_forms_on_the_device(ctx, oracle):
    """The forms k_sift_grad takes for a flat patch -- hm_atan2f_tab through the LDS table, sqrtf, hm_sift_orient_coord -- as
    hipcc compiles them, on the (gy, gx) of every masked pixel of the flat and saturating families (numpy float32, the
    reference's stencil), the cross product of +-0, the smallest and largest subnormal, the smallest normal, 1 and the
    largest finite float, quotients on and next to the interval thresholds of atanf and 2^25, and exponent gaps of 59, 60
    and 61 binades.  Orientation: the bits of libm's atan2f including the sign of zero; magnitude: numpy's float32 sqrt of
    the float32 sum of float32 squares; coordinate: siftdesc.cpp:65 in double."""
    gy, gx = _gradient_operands()
    assert gy.size > 40000
    k = _exponent(gy) - _exponent(gx)
    assert ((gy != 0) & (gx != 0) & (np.abs(k) > 60)).sum() > 100   # the out-of-line path is in
    ori, grad, coord = ctx.math_sift_general(gy, gx)
    L = oracle.lib()
    want_ori = np.array([L.ho_atan2f(float(a), float(b)) for a, b in zip(gy, gx)], F)
    with np.errstate(over="ignore", under="ignore"):
        want_grad = np.sqrt((gx * gx + gy * gy).astype(F)).astype(F)
    want_coord = ((8.0 * (want_ori.astype(np.float64) + 2 * np.pi)) / (2 * np.pi)).astype(F)
    assert_same_bits(ori, want_ori, "atan2f, general tabled form")
    assert_same_bits(grad, want_grad, "gradient magnitude")
    assert_same_bits(coord, want_coord, "orientation coordinate")
    assert coord.min() >= 4.0 and coord.max() <= 12.0 and (coord == 12.0).any()   # the range k_sift_hist relies on


@gpu
@pytest.mark.parametrize("name", FAMILIES)
def test_descriptor_parts_per_family(ctx, name):
    """One hesaff_stage_sift_parts call per family: mean and var as bits, the un-normalised histogram as bits (+0 == -0),
    the bytes, and the same bytes from hesaff_stage_sift."""
    patches = _family(name)
    want_mv, want_hist, want_desc = _oracle_parts_of(name)
    mv, hist, desc = ctx.sift_parts(patches)
    assert_same_bits(mv, want_mv, name + ": mean, var")
    assert_same_bits(hist, want_hist, name + ": histogram", zero_signs=False)
    bad = np.flatnonzero((desc != want_desc).any(axis=1))
    assert bad.size == 0, (name, bad[:10].tolist())
    assert np.array_equal(ctx.sift(patches), want_desc), name


COUNTS = (1, 2, 3, 4, 5, 15, 16, 17, 63, 64, 65)


@gpu
def test_descriptor_parts_for_every_group_remainder(ctx):
    """The first n patches of the interleaving for n around the kernels' group sizes (4 keypoints per wavefront of
    k_sift_hist, 16 of k_sift_meanvar, 64 of k_sift_quantize): a patch's results do not depend on its neighbours or on
    the padding of the last group."""
    want_mv, want_hist, want_desc = _oracle_parts_of("interleaved:%d" % max(COUNTS))
    patches = si.interleaved(max(COUNTS))
    for n in COUNTS:
        mv, hist, desc = ctx.sift_parts(patches[:n])
        assert_same_bits(mv, want_mv[:n], "n=%d: mean, var" % n)
        assert_same_bits(hist, want_hist[:n], "n=%d: histogram" % n, zero_signs=False)
        assert np.array_equal(desc, want_desc[:n]), n
        assert np.array_equal(ctx.sift(patches[:n]), want_desc[:n]), n


POOL = 600


@gpu
def test_descriptor_parts_when_every_persistent_block_takes_several_keypoints(ctx):
    """n = 4 * 32 * CUs + 3 patches tiled from a pool of 600: k_sift_grad's grid is 32 blocks per CU, so every block walks
    at least four keypoints, three blocks five.  Patch j is pool[(j + j // G) % 600] with G the grid size: neighbours
    differ in family, and so do the keypoints k, k + G, ... of one block, whose block-uniform normalised / flat switch
    therefore flips while the next keypoint's mean and var are already in registers."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    G = 32 * cus
    n = 4 * G + 3
    pool = si.interleaved(POOL)
    want_mv, want_hist, want_desc = _oracle_parts_of("interleaved:%d" % POOL)
    j = np.arange(n)
    idx = (j + j // G) % POOL
    flat_body = np.array([si.is_flat_var(v) for v in want_mv[:, 1]])
    assert 0.3 < flat_body.mean() < 0.7
    assert (flat_body[idx[:-G]] != flat_body[idx[G:]]).mean() > 0.9 and (flat_body[idx[:-1]] != flat_body[idx[1:]]).mean() > 0.9
    mv, hist, desc = ctx.sift_parts(pool[idx])
    assert_same_bits(mv, want_mv[idx], "mean, var")
    assert_same_bits(hist, want_hist[idx], "histogram", zero_signs=False)
    bad = np.flatnonzero((desc != want_desc[idx]).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:10].tolist(), idx[bad[:10]].tolist())


CLIP_PATCHES = (17, 18, 19)   # of stage_inputs.ordinary()
CLIP_BIN_BITS = 0x3d932b7d    # the value of the first normalizeVec of patch 17 that is taken as maxBinValue


def _first_normalize_vec(hist):
    """siftdesc.cpp:83-96 in float32: sequential sum of squares, 1.0f / sqrt, product."""
    s = F(0)
    for x in hist:
        s = F(s + F(x * x))
    fac = F(F(1) / np.sqrt(s))
    return (hist * fac).astype(F)


@gpu
def test_descriptor_clip_at_equality(oracle):
    """k_sift_quantize's `x > maxBinValue` with maxBinValue equal to a bin of the normalised vector, and one float32 step
    below and above it.  maxBinValue is a float in hesaff_params and in the oracle's parameters: it carries x exactly.
    A bin value strictly inside the vector's range changes nothing by itself at equality (clipping x to x), so the value is
    one -- found by a search over the ordinary patches' bins with the oracle -- at which the one-step change of the
    clipped bins' value does move a byte: the three results are not all equal, and each equals the oracle's."""
    import hesaff_amd
    patches = si.ordinary()[list(CLIP_PATCHES)]
    hist = _oracle_parts_of("ordinary")[1][CLIP_PATCHES[0]]
    v = _first_normalize_vec(hist)
    x = np.array(CLIP_BIN_BITS, np.uint32).view(F)
    assert (v == x).any() and v.min() < x < v.max()
    results = []
    for mbv in (np.nextafter(x, F(0)), x, np.nextafter(x, F(1))):
        p = hesaff_amd.default_params(); p.maxBinValue = float(mbv)
        assert F(p.maxBinValue) == mbv
        oh = oracle.OracleHandle(p)
        want = np.stack([oh.sift(pp) for pp in patches])
        with hesaff_amd.HesaffContext(p, device=0) as c2:
            got = c2.sift(patches)
        assert np.array_equal(got, want), float(mbv)
        results.append(want)
    assert not (np.array_equal(results[0], results[1]) and np.array_equal(results[1], results[2]))


@gpu
def test_window_sweep_through_every_patch_kernel(ctx, oracle):
    """normalizeAffine on noise for every window side next to a cut between two patch kernels and every row remainder of
    the mid and large kernels (stage_inputs.windows), in three calls: the windows up to 1279 (one launch of
    k_patch_large_rows, three-row form), all of them (split launches), and those from 1281 alone.  Patches as bits against
    the oracle, none rejected, a window's patch the same in every call; then the sweep's patches through the descriptor
    kernels against the oracle, parts and bytes."""
    kp, A, P0, P = si.windows()
    want_rej, want = _oracle_windows()
    assert not want_rej.any()
    gray = oracle.gray_from_u8(si.window_image())
    sel3 = np.flatnonzero(P <= 1279); sel1 = np.flatnonzero(P >= 1281)
    assert len(sel3) + len(sel1) == len(P) and len(sel1) >= 18
    got = {}
    for what, sel in (("P <= 1279", sel3), ("all", np.arange(len(P))), ("P >= 1281", sel1)):
        rej, patches = ctx.normalize_affine(gray, kp[sel], A[sel])
        assert not rej.any(), (what, P[sel][rej != 0])
        ne = (_bits(patches) != _bits(want[sel])).reshape(len(sel), -1).any(axis=1)
        assert not ne.any(), "%s: the patches of the windows with P = %s differ from the oracle's" % (what, P[sel][ne].tolist())
        got[what] = patches
    assert np.array_equal(_bits(got["all"][sel3]), _bits(got["P <= 1279"])) and np.array_equal(_bits(got["all"][sel1]), _bits(got["P >= 1281"]))
    oh = oracle.OracleHandle()
    res = [oh.sift_parts(p) for p in want]
    mv, hist, desc = ctx.sift_parts(got["all"])
    assert_same_bits(mv, np.stack([r[0] for r in res]), "sweep: mean, var")
    assert_same_bits(hist, np.stack([r[1] for r in res]), "sweep: histogram", zero_signs=False)
    assert np.array_equal(desc, np.stack([r[2] for r in res]))
