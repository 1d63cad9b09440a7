"""GPU suite of the dominant-orientation mode (hesaff_set_orientation, include/hesaff_amd.h).  The reference is the oracle chain of
tests/orientation_ref.py: ho_rectify -> normalizeAffine -> the estimator in numpy float32 with the oracle's atan2f and circular mask
-> A' = A R(theta) in numpy float32 -> normalizeAffine -> SIFT.  Everything is held bit for bit; the one inequality is the purpose
test's (descriptors of a rotated image are closer with the mode on than with it off)."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import FROM_SHAPES, ORI_DOMINANT, ORI_UP, _binding
from hesaff_amd.synth import band_noise_image
from tests import orientation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REGION = _binding.REGION_DTYPE
KEY = _binding.KEYPOINT_DTYPE
E2E_IMAGES = ["band_160x120", "band_96x96", "tiny_20x15", "thin_12x40"]


def _u32(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _same_records(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    for name in got.dtype.names:
        g, w = np.ascontiguousarray(got[name]), np.ascontiguousarray(want[name])
        same = (_u32(g) == _u32(w)) if g.dtype == np.float32 else (g == w)
        if same.ndim > 1:
            same = same.all(axis=1)
        assert same.all(), "%s: field %s differs at records %s" % (what, name, np.nonzero(~same)[0][:8].tolist())


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def octx():
    """a context of its own with the mode on (the session's context stays in mode 0)"""
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_orientation(ORI_DOMINANT)
        assert c.orientation == ORI_DOMINANT
        yield c


_golden = {}


def golden(oracle, name):
    """image, float grey plane and the reference chain's (regions, keys, n_hessian) of a golden image: computed once"""
    if name not in _golden:
        img = hesaff_amd.read_pnm(os.path.join(GOLD, name + ".pgm"))
        gray = oracle.gray_from_u8(img)
        _golden[name] = (img, gray) + R.oriented_run(oracle, gray)
    return _golden[name]


# ---------------------------------------------------------------- the stage operator

def oracle_patches(oracle, name, limit):
    img, gray = golden(oracle, name)[:2]
    run = oracle.OracleRun(gray)
    hf, _ = run.hessian()
    U, ai = run.affine()
    handle = oracle.OracleHandle()
    out = []
    for k in range(run.n_hessian):
        if not ai[k, 0]:
            continue
        A = U[k].copy()
        oracle.lib().ho_rectify(A)
        rej, p = handle.normalize_affine(gray, hf[k, 0], hf[k, 1], hf[k, 2], A)
        if not rej:
            out.append(p)
        if len(out) == limit:
            break
    return np.stack(out)


def check_stage(ctx, oracle, patches, what, counts=()):
    """counts: the operator on the first n patches alone as well, for every n of it, against the same reference"""
    want = [R.estimate(oracle, p) for p in patches]
    for n in tuple(counts) + (len(patches),):
        theta, hist, cs = ctx.orientation_of(patches[:n], parts=True)
        assert np.array_equal(_u32(ctx.orientation_of(patches[:n])), _u32(theta))
        for k in range(n):
            t, h, (c, s), flat = want[k]
            assert np.array_equal(_u32(hist[k]), _u32(h)), "%s, first %d: histogram of patch %d" % (what, n, k)
            assert _u32(theta[k:k + 1])[0] == _u32(np.array([t], np.float32))[0], "%s, first %d: theta of patch %d: %r, reference %r" % (what, n, k, theta[k], t)
            assert _u32(cs[k])[0] == _u32(np.array([c], np.float32))[0] and _u32(cs[k])[1] == _u32(np.array([s], np.float32))[0], \
                "%s, first %d: (cos, sin) of patch %d: %r, reference %r" % (what, n, k, cs[k], (c, s))
    return theta, hist, cs, np.array([w[3] for w in want])


@pytest.mark.gpu
def test_stage_on_oracle_patches(ctx, oracle):
    """hesaff_stage_orientation on 100 patches normalizeAffine made on band_160x120: theta, the smoothed histogram, cos and sin are
    the reference's bits - and of the first 1, 3 and 65 of them alone, sizes at which the operator's arrays are multiples of nothing.
    The property `orientation`, called, is the same operator."""
    patches = oracle_patches(oracle, "band_160x120", 100)
    assert len(patches) == 100
    theta, _, _, flats = check_stage(ctx, oracle, patches, "oracle patches", counts=(1, 3, 65))
    assert not flats.any() and len(np.unique(theta)) > 90 and theta.min() < -2.0 and theta.max() > 2.0
    assert ctx.orientation == ORI_UP   # the operator neither needs nor changes the mode
    assert np.array_equal(_u32(ctx.orientation(patches[:3])), _u32(theta[:3]))


def constructed_patches():
    f32 = np.float32
    c = np.tile(np.arange(41, dtype=f32), (41, 1))
    r = c.T.copy()
    rng = np.random.default_rng(17)

    def one(i, j):
        z = np.zeros((41, 41), f32)
        z[i, j] = 200.0
        return z

    return {
        "constant": np.full((41, 41), 93.0, f32),
        "ramp_x": c, "ramp_y": r, "ramp_45": c + r,
        "ramp_pi": -c,                       # every gradient (gx, gy) = (-2, 0): atan2f = pi, t = 36, the wrap to bin 0
        "pixel_1_1": one(1, 1), "pixel_39_39": one(39, 39),
        "pm_2_20": ((rng.integers(0, 2, (41, 41)) * 2 - 1) * 2.0 ** 20).astype(f32),
        "tie": one(20, 20),                  # four gradients of one weight at 0, 90, 180, 270 degrees: bins 18, 27, 0 (wrapped) and 9 tie
        "noise": rng.uniform(0, 255, (41, 41)).astype(f32),
    }


@pytest.mark.gpu
def test_stage_on_constructed_patches(ctx, oracle):
    """The estimator's edges: a flat patch (theta = 0), ramps, a single bright pixel where the mask is zero, values of +-2^20, an
    exact tie of the best bins (the lowest index wins) and gradients of angle exactly pi (b = 36 wraps to 0): the reference's bits."""
    cases = constructed_patches()
    names = list(cases)
    patches = np.stack([cases[n] for n in names])
    theta, hist, cs, flats = check_stage(ctx, oracle, patches, "constructed")
    at = {n: i for i, n in enumerate(names)}
    for n in ("constant", "pixel_1_1", "pixel_39_39"):   # no gradient, or none under the mask: theta = 0, cos = 1, sin = 0
        i = at[n]
        assert flats[i] and not hist[i].any() and _u32(theta[i:i + 1])[0] == 0 and cs[i, 0] == 1.0 and _u32(cs[i])[1] == 0, n
    assert R.mask(oracle)[1, 1] == 0 and R.mask(oracle)[39, 39] == 0
    for n in ("ramp_x", "ramp_y", "ramp_45", "ramp_pi", "pm_2_20", "tie", "noise"):
        assert not flats[at[n]] and np.isfinite(hist[at[n]]).all(), n
    # the wrap: the reference's own bins reach 36 before it, and everything lands in bin 0
    _, b, raw = R.bins_of(oracle, cases["ramp_pi"])
    assert (raw == 36).all() and (b == 0).all() and int(np.argmax(hist[at["ramp_pi"]])) == 0
    # the tie: four equal maxima nine bins apart, bin 0 among them through the wrap; theta is bin 0's
    h = hist[at["tie"]]
    tied = np.nonzero(h == h.max())[0].tolist()
    assert tied == [0, 9, 18, 27], tied
    assert (R.bins_of(oracle, cases["tie"])[2] == 36).sum() == 1
    assert abs(float(theta[at["tie"]]) - (0.5 * 2 * np.pi / 36 - np.pi)) < 0.05
    assert abs(float(theta[at["ramp_x"]]) - (18.5 * 2 * np.pi / 36 - np.pi)) < 0.1


# ---------------------------------------------------------------- end to end

@pytest.mark.gpu
@pytest.mark.parametrize("name", E2E_IMAGES)
def test_end_to_end_equals_the_reference_chain(ctx, octx, oracle, name):
    """detect_regions and detect_batch with the mode on: counts, every field of every region (outcome and key included), every key
    field - A' included - and all 128 descriptor bytes are the reference chain's over the oracle's regions; what the mode must not
    touch (x, y, s, response, type, U, iters) is the mode-0 run's."""
    img, gray, want_r, want_k, n_hess = golden(oracle, name)
    (got_r, got_k), = octx.detect_regions([img])
    (nh, keys_b), = octx.detect_batch([img])
    print("%s: %d Hessian keypoints, %d oriented keys, %d rejected in either pass" % (name, n_hess, len(want_k), int((want_r["outcome"] == 1).sum())))
    assert nh == n_hess == len(got_r)
    _same_records(got_r, want_r, name + ": regions")
    _same_records(got_k, want_k, name + ": keys")
    assert keys_b.tobytes() == got_k.tobytes()
    (up_r, up_k), = ctx.detect_regions([img])
    for f in ("x", "y", "s", "pixelDistance", "response", "type", "octave", "level", "a11", "a12", "a21", "a22", "iters"):
        assert np.array_equal(_u32(got_r[f]), _u32(up_r[f])), f
    assert ((got_r["outcome"] == 0) == (up_r["outcome"] == 0)).all() and (got_r["outcome"] <= up_r["outcome"]).all()
    if name.startswith("band"):
        assert len(want_k) > 20
        # the frames were turned: A' differs from the upright A, its ellipse does not (A' A'^T = A A^T up to rounding)
        both = np.nonzero((got_r["outcome"] == 2) & (up_r["outcome"] == 2))[0]
        ko, ku = got_k[got_r["key"][both]], up_k[up_r["key"][both]]
        assert (ko["a12"] != 0).mean() > 0.9 and (ku["a12"] == 0).all()
        so = ko["a11"].astype(np.float64) ** 2 + ko["a12"].astype(np.float64) ** 2
        su = ku["a11"].astype(np.float64) ** 2 + ku["a12"].astype(np.float64) ** 2
        assert np.allclose(so, su, rtol=1e-5)


@pytest.mark.gpu
def test_mode_0_is_untouched(oracle):
    """set 1, set 0, detect: the bytes are a fresh context's."""
    imgs = [golden(oracle, "band_160x120")[0], golden(oracle, "band_96x96")[0]]
    with hesaff_amd.HesaffContext(device=0) as fresh:
        want = fresh.detect_regions(imgs)
    with hesaff_amd.HesaffContext(device=0) as c:
        assert c.orientation == ORI_UP
        c.set_orientation("dominant")
        assert c.orientation == ORI_DOMINANT
        turned = c.detect_regions(imgs)
        c.orientation = ORI_UP
        assert c.orientation == ORI_UP
        got = c.detect_regions(imgs)
        with pytest.raises(hesaff_amd.HesaffError):
            c.set_orientation(2)
        with pytest.raises(ValueError):
            c.set_orientation("sideways")
        assert c.orientation == ORI_UP
    for (gr, gk), (wr, wk), (tr, tk) in zip(got, want, turned):
        assert gr.tobytes() == wr.tobytes() and gk.tobytes() == wk.tobytes()
        assert tk.tobytes() != wk.tobytes()


# ---------------------------------------------------------------- a general A in every window bin

BIN_SCALES = [2.0, 5.5, 11.0, 40.0, 55.0, 125.0]   # windows of 25, 61, 119, 419, 575 and 1303 pixels: the five bins, and one above the three-row split
BIN_H = BIN_W = 2000


def _window(s, mr_size):
    p0 = 2 * int(np.ceil(np.float32(s) * np.float32(mr_size))) + 1
    return p0 + 2


def _shape(k):
    """an anisotropic U per scale; nearly isotropic for the largest, whose turned 1303-pixel window must still fit 2000 pixels"""
    th, r = 0.4 + 0.9 * k, (1.3 + 0.25 * k if k < 5 else 1.1)
    Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    return (Rm @ np.diag([1.0, 1.0 / r]) @ Rm.T).astype(np.float32)


def bin_records(oracle, gray):
    """-> (centred records, records at the right border that pass one accepts and whose turned window leaves the image)"""
    handle = oracle.OracleHandle()
    centred = np.zeros(len(BIN_SCALES), REGION)
    edge = np.zeros(len(BIN_SCALES), REGION)
    for k, s in enumerate(BIN_SCALES):
        U = _shape(k)
        for rec in (centred, edge):
            rec[k]["x"], rec[k]["y"], rec[k]["s"] = BIN_W / 2 + 3.25 * k, BIN_H / 2 - 2.5 * k, s
            rec[k]["a11"], rec[k]["a12"], rec[k]["a21"], rec[k]["a22"] = U.reshape(-1)
            rec[k]["response"], rec[k]["type"] = 10.0 + k, k % 3
        A = U.reshape(-1).copy()
        oracle.lib().ho_rectify(A)
        # the smallest distance d from the right border (to 1/8 pixel) at which normalizeAffine accepts the upright frame: the turned
        # frame's window is wider in x by |cos| + |sin| there (the rectified a12 is 0)
        lo, hi = 0.0, BIN_W / 2.0   # rejected, accepted
        y = float(centred[k]["y"])
        while hi - lo > 0.125:
            mid = 0.5 * (lo + hi)
            rej, _ = handle.normalize_affine(gray, BIN_W - 1 - mid, y, s, A)
            lo, hi = (mid, hi) if rej else (lo, mid)
        edge[k]["x"] = BIN_W - 1 - hi
    return centred, edge


@pytest.mark.gpu
def test_general_frames_in_every_window_bin(octx, oracle):
    """describe_regions(HESAFF_FROM_SHAPES) with the mode on, 2000 x 2000: a keypoint per window-size bin and one above the 1280-pixel
    three-row split, whose second pass runs the patch kernels on a frame with a12 != 0 - the reference chain's bits; and the same
    keypoints at the border, where pass one accepts and the turned window leaves the image - outcome 1, no key."""
    mr = octx.params.mrSize
    assert [_window(s, mr) for s in BIN_SCALES] == [25, 61, 119, 419, 575, 1303]
    img = band_noise_image(BIN_H, BIN_W, 5)
    gray = oracle.gray_from_u8(img)
    centred, edge = bin_records(oracle, gray)
    want_c, keys_c = R.oriented_from_shapes(oracle, gray, centred)
    want_e, keys_e = R.oriented_from_shapes(oracle, gray, edge)
    assert (want_c["outcome"] == 2).all() and len(keys_c) == len(BIN_SCALES) and (keys_c["a12"] != 0).all()
    assert (want_e["outcome"] == 1).all() and len(keys_e) == 0
    handle = oracle.OracleHandle()
    for r in edge:   # ... and pass one did accept them
        A = np.array([r["a11"], r["a12"], r["a21"], r["a22"]], np.float32)
        oracle.lib().ho_rectify(A)
        assert handle.normalize_affine(gray, r["x"], r["y"], r["s"], A)[0] == 0
    (got_c, gk_c), = octx.describe_regions([img], [centred], FROM_SHAPES)
    _same_records(got_c, want_c, "centred: regions")
    _same_records(gk_c, keys_c, "centred: keys")
    (got_e, gk_e), = octx.describe_regions([img], [edge], FROM_SHAPES)
    _same_records(got_e, want_e, "border: regions")
    assert len(gk_e) == 0 and (got_e["key"] == -1).all()
    # both sets in one call, interleaved: a rejected neighbour changes nothing
    mixed = np.stack([centred, edge], axis=1).reshape(-1)
    (got_m, gk_m), = octx.describe_regions([img], [mixed], FROM_SHAPES)
    assert gk_m.tobytes() == gk_c.tobytes() and got_m["outcome"].tolist() == [2, 1] * len(BIN_SCALES)


@pytest.mark.gpu
def test_describe_from_points_equals_the_oriented_detect_run(octx, oracle):
    """describe_regions(HESAFF_FROM_POINTS) with the mode on, over detect_regions' own records: findAffineShape runs again, and the
    regions and keys are the oriented detecting run's (which the end-to-end test holds to the reference chain)."""
    imgs = [golden(oracle, "band_160x120")[0], golden(oracle, "band_96x96")[0]]
    detected = octx.detect_regions(imgs)
    described = octx.describe_regions(imgs, [r for r, _ in detected], hesaff_amd.FROM_POINTS)
    for (dr, dk), (pr, pk) in zip(detected, described):
        assert len(dk) > 20 and (dk["a12"] != 0).any()
        _same_records(pr, dr, "FROM_POINTS: regions")
        _same_records(pk, dk, "FROM_POINTS: keys")


# ---------------------------------------------------------------- composition

def _identity(keys):
    return [tuple(_u32(np.array([k[f] for f in ("x", "y", "s", "response")], np.float32)).tolist()) for k in keys]


@pytest.mark.gpu
def test_composes_with_limit_and_mask(octx, oracle):
    """set_keypoint_limit(N) and a half-image mask with the mode on: the kept keys' bytes are those of the same keypoints in the
    unlimited, unmasked oriented run."""
    img, _, want_r, want_k, n_hess = golden(oracle, "band_160x120")
    mask = np.zeros(img.shape, np.uint8)
    mask[:, : img.shape[1] // 2] = 1
    octx.set_keypoint_limit(40)
    try:
        (nh, kept), = octx.detect_batch([img], masks=[mask])
    finally:
        octx.set_keypoint_limit(0)
    full = {ident: k.tobytes() for ident, k in zip(_identity(want_k), want_k)}
    assert len(full) == len(want_k)
    assert nh == 40 < n_hess and 5 < len(kept) < len(want_k)
    assert (kept["x"] < img.shape[1] // 2 + 1).all()
    for ident, k in zip(_identity(kept), kept):
        assert full.get(ident) == k.tobytes(), ident


@pytest.mark.gpu
def test_fast_mode_small_windows_equal_parity_mode(octx, oracle):
    """fast = 2 with the mode on: both passes of a window of at most 41 pixels run the parity kernel, so those keys are the parity
    mode's oriented keys."""
    img = golden(oracle, "band_160x120")[0]
    (_, parity), = octx.detect_batch([img])
    with hesaff_amd.HesaffContext(_params(fast=2), device=0) as cf:
        cf.set_orientation(ORI_DOMINANT)
        (_, fast), = cf.detect_batch([img])
        mr = cf.params.mrSize
    want = {ident: k.tobytes() for ident, k in zip(_identity(parity), parity)}
    small = [i for i, k in enumerate(fast) if _window(k["s"], mr) <= 41]
    assert len(small) > 20 and len(small) < len(fast)
    for i, ident in zip(small, [_identity(fast)[i] for i in small]):
        assert want.get(ident) == fast[i].tobytes(), ident


@pytest.mark.gpu
def test_process_files_text_is_the_oriented_keys(octx, oracle, tmp_path):
    img, _, _, want_k, _ = golden(oracle, "band_160x120")
    src = os.path.join(GOLD, "band_160x120.pgm")
    path = str(tmp_path / "band.pgm")
    shutil.copyfile(src, path)
    st = octx.process_files([path])
    assert st[0][0] == 0 and st[0][3] == len(want_k), st
    text = open(path + ".hesaff.sift", "rb").read()
    assert text == hesaff_amd.format_sift(want_k, octx.params.mrSize)


@pytest.mark.gpu
def test_cpp_detector_with_orientation(oracle, tmp_path):
    """tests/native/orientation_keys.cpp: AffineHessianDetector::setOrientation(HESAFF_ORI_DOMINANT) holds the reference chain's keys."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    _, _, want_r, want_k, n_hess = golden(oracle, "band_96x96")
    exe = str(tmp_path / "orientation_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "orientation_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, "1", os.path.join(GOLD, "band_96x96.pgm")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "N %d %d %d" % (n_hess, len(want_k), len(want_k)), lines[0]
    assert [ln[2:] for ln in lines[1:]] == [k.tobytes().hex() for k in want_k]


# ---------------------------------------------------------------- what the mode is for

@pytest.mark.gpu
def test_descriptors_follow_a_rotation_of_the_image(ctx, octx):
    """band_noise_image(240, 320, seed=7) and its np.rot90: the first 300 converged keypoints of the image, carried over by
    (x, y) -> (y, W - 1 - x), U -> [[0, 1], [-1, 0]] U, described in both images through describe_regions_f32(FROM_SHAPES).  The
    median L2 distance between the paired descriptors is smaller with the mode on than with it off (the CPU prototype of the
    definition: 11.7 against 531)."""
    img = band_noise_image(240, 320, seed=7)
    H, W = img.shape
    (reg, _), = ctx.detect_regions([img])
    rec = reg[reg["outcome"] >= 1][:300].copy()
    assert len(rec) == 300
    rot = rec.copy()
    rot["x"], rot["y"] = rec["y"], np.float32(W - 1) - rec["x"]
    rot["a11"], rot["a12"], rot["a21"], rot["a22"] = rec["a21"], rec["a22"], -rec["a11"], -rec["a12"]
    planes = [img.astype(np.float32), np.ascontiguousarray(np.rot90(img)).astype(np.float32)]
    assert planes[1].shape == (W, H) and planes[1][W - 1 - 17, 5] == planes[0][5, 17]
    medians = {}
    for name, c in (("up", ctx), ("dominant", octx)):
        (r0, k0), (r1, k1) = c.describe_regions_f32(planes, [rec, rot], FROM_SHAPES)
        both = np.nonzero((r0["outcome"] == 2) & (r1["outcome"] == 2))[0]
        assert len(both) > 200, (name, len(both))
        d0 = k0["desc"][r0["key"][both]].astype(np.float64)
        d1 = k1["desc"][r1["key"][both]].astype(np.float64)
        dist = np.sqrt(((d0 - d1) ** 2).sum(axis=1))
        medians[name] = float(np.median(dist))
        if name == "up":
            up_dist, up_both = dist, both
        else:
            common, iu, io = np.intersect1d(up_both, both, return_indices=True)
            closer = float((dist[io] < up_dist[iu]).mean())
    print("median paired L2 distance: upright %.1f, dominant orientation %.1f; the oriented one is the smaller in %.1f %% of %d pairs"
          % (medians["up"], medians["dominant"], 100.0 * closer, len(common)))
    assert medians["dominant"] < medians["up"], medians
