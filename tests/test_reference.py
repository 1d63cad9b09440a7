"""The compiled reference against the oracle (CPU) and against the HIP path (GPU).

oracle/_ref/ holds the reference's own sources, compiled unmodified against the OpenCV stand-in oracle/cvshim/ (`make -C oracle
ref`, called by __graft_entry__.build()); tests/golden/ref_*.npz hold what it wrote for small inputs.

CPU tests run the binaries live and compare every float as bits with tests/_oracle, and check that the oracle reproduces the
committed fixtures (that part needs no binary).  GPU tests compare the library with the committed fixtures directly: the oracle is
not in that loop.
"""
import hashlib
import os
import subprocess

import numpy as np
import pytest

from hesaff_amd.synth import band_noise_image
from tests import _reference as R

SMALL_BANDS = R.SMALL_BANDS
SET_NAMES = list(R.PARAM_SETS)


def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def driver():
    return R.binary("ref_driver")


@pytest.fixture(scope="module")
def hesaff_ref():
    return R.binary("hesaff_ref")


@pytest.fixture(scope="module")
def parameter_images(oracle):
    return [("300x420", oracle.gray_from_u8(band_noise_image(300, 420, 91))),
            ("200x260", oracle.gray_from_u8(band_noise_image(200, 260, 92, SMALL_BANDS)))]


def check_driver_against_oracle(driver, oracle, grey, kw, what):
    rec = R.run_driver(driver, grey, kw)
    want, _ = R.oracle_records(oracle, grey, kw)
    R.same_records(rec, want, what)
    return rec


# ------------------------------------------------------------------ CPU, live ------------------------------------------------------------------

def test_binaries_are_static(driver, hesaff_ref):
    """-static: the binaries carry the libm they were built with, so they give the same bits on every machine of this kind"""
    for exe in (driver, hesaff_ref):
        head = open(exe, "rb").read(1 << 16)
        assert head[:4] == b"\x7fELF" and b"/ld-linux" not in head and b"ld-musl" not in head, exe + " names a dynamic loader"


def test_driver_refuses_upscale_and_unknown_parameters(driver, tmp_path):
    """doubleImage (helpers.cpp:297-329) steps through float rows with the byte step and reads outside its input: it must not run"""
    src = tmp_path / "in.f32"
    np.zeros((20, 20), np.float32).tofile(src)
    for arg, word in (("upscaleInputImage=1", "doubleImage"), ("numberOfScales=4", "unknown parameter")):
        r = subprocess.run([driver, str(src), "20", "20", str(tmp_path / "out.rec"), arg], capture_output=True, text=True)
        assert r.returncode == 2 and word in r.stderr, (arg, r.returncode, r.stderr)
        assert not (tmp_path / "out.rec").exists()


@pytest.mark.parametrize("name", R.GOLDEN_PGMS + ["probe_vga"])
def test_whole_files(hesaff_ref, oracle, name):
    """The reference's own main: its counts are the oracle's and its .hesaff.sift is the oracle's text byte for byte, a, b and c
    included (the stand-in's SVD reproduces the survey's md5 on probe_vga, DESIGN.md section 2, so no tolerance is needed)."""
    import hesaff_amd
    path = os.path.join(R.GOLD, name + ".pgm")
    n_hess, n_desc, text = R.run_hesaff_ref(hesaff_ref, path)
    o = oracle.OracleRun(oracle.gray_from_u8(hesaff_amd.read_pnm(path)))
    assert (n_hess, n_desc) == (o.n_hessian, o.n_keys)
    m = R.manifest()[name]
    assert (n_hess, n_desc) == (m["hessian"], m["descriptors"])
    want = o.export_text()
    if text != want:
        a, b = text.split(b"\n"), want.split(b"\n")
        assert len(a) == len(b), (len(a), len(b))
        row = next(i for i in range(len(a)) if a[i] != b[i])
        raise AssertionError("%s: row %d differs:\n%r\n%r" % (name, row, a[row][:80], b[row][:80]))
    assert hashlib.md5(text).hexdigest() == m["sift_md5"]
    if name == "probe_vga":
        assert hashlib.md5(text).hexdigest().startswith("e004ba88") and (n_hess, n_desc) == (4763, 4183)
    else:
        assert text == open(os.path.join(R.GOLD, name + ".hesaff.sift"), "rb").read()


@pytest.mark.parametrize("name", SET_NAMES)
def test_parameter_sets(driver, oracle, parameter_images, name):
    """ref_driver against OracleRun(params=...), every field of every record as bits, on the two images of
    test_gpu_parity.test_non_default_parameters"""
    kw = R.PARAM_SETS[name]
    described = 0
    for tag, grey in parameter_images:
        rec = check_driver_against_oracle(driver, oracle, grey, kw, "%s on %s" % (name, tag))
        described += int((rec["fate"] == R.DESCRIBED).sum())
    assert described > 30


def test_structured_ragged_images(driver, oracle):
    """the forty images of test_gpu_parity.test_fuzz_ragged_sizes_and_structured_content"""
    from tests.test_gpu_parity import _structured_image
    rng = np.random.default_rng(20261001)
    kinds = ["checker", "blobs", "lines", "saturated", "ramp"]
    described = 0
    for i in range(40):
        h, w = int(rng.integers(13, 260)), int(rng.integers(13, 330))
        img = _structured_image(kinds[i % len(kinds)], h, w, rng)
        rec = check_driver_against_oracle(driver, oracle, oracle.gray_from_u8(img), {}, "image %d (%s %s)" % (i, kinds[i % 5], img.shape))
        described += int((rec["fate"] == R.DESCRIBED).sum())
    assert described > 3000


# float planes of a 131 x 177 image, all in float32.  pm2^20: the 8-bit range stretched to -2^20 .. +2^20 (253/255 of it)
FLOAT_TRANSFORMS = {
    "affine": lambda u: u * np.float32(0.37) + np.float32(12.25),
    "x257": lambda u: u * np.float32(257.0),
    "negative": lambda u: u * np.float32(1.37) - np.float32(300.75),
    "x2^-140": lambda u: u * np.float32(2.0 ** -140),
    "x4096": lambda u: u * np.float32(4096.0),
    "pm2^20": lambda u: (u - np.float32(128.0)) * np.float32(8192.0),
}


@pytest.mark.parametrize("name", list(FLOAT_TRANSFORMS))
def test_float_planes(driver, oracle, name):
    u = band_noise_image(131, 177, 93, SMALL_BANDS).astype(np.float32)
    plane = FLOAT_TRANSFORMS[name](u)
    assert plane.dtype == np.float32
    rec = check_driver_against_oracle(driver, oracle, plane, {}, name)
    if name == "x2^-140":
        assert plane.max() < np.finfo(np.float32).tiny and len(rec) == 0   # all subnormal: no response reaches the threshold
    else:
        assert (rec["fate"] == R.DESCRIBED).sum() >= 30 and set(np.unique(rec["fate"]).tolist()) == {0, 1, 2}   # (x0.37 leaves 40)


@pytest.mark.parametrize("h,w", [(12, 13), (13, 13), (13, 200), (25, 25), (26, 27), (51, 53)])
def test_small_sizes(driver, oracle, h, w):
    """around the octave limit (rows and cols > 12, pyramid.cpp:283-284): no octave, one octave, one and two and three"""
    grey = oracle.gray_from_u8(band_noise_image(h, w, 94, SMALL_BANDS))
    rec = check_driver_against_oracle(driver, oracle, grey, {}, "%dx%d" % (h, w))
    if min(h, w) <= 12:
        assert len(rec) == 0
    if (h, w) == (51, 53):
        assert len(rec) > 10 and len(set(rec["pixelDistance"].tolist())) >= 2


def test_probe_vga_and_fhd(driver, oracle):
    """the survey's photograph-like VGA image, and 1080 x 1920 for seven octaves and windows of several hundred pixels"""
    import hesaff_amd
    rec = check_driver_against_oracle(driver, oracle, oracle.gray_from_u8(hesaff_amd.read_pnm(os.path.join(R.GOLD, "probe_vga.pgm"))), {},
                                      "probe_vga")
    assert (len(rec), int((rec["fate"] == R.DESCRIBED).sum())) == (4763, 4183)
    rec = check_driver_against_oracle(driver, oracle, oracle.gray_from_u8(band_noise_image(1080, 1920, 77)), {}, "fhd")
    assert rec["pixelDistance"].max() >= 32.0 and len(rec) > 20000   # (seven octaves run; the coarsest keypoints are in the sixth)
    assert (2 * np.ceil(rec["s"][rec["fate"] == R.DESCRIBED] * np.float32(R.DEFAULTS["mrSize"])) + 3).max() > 256


def test_initial_sigma_belongs_to_the_pyramid(driver, oracle, parameter_images):
    """hesaff_params.initialSigma is PyramidParams::initialSigma (pyramid.h:36) and nothing else: AffineShapeParams::initialSigma
    (affine.h:40) stays 1.6, as in the reference's main, which never sets either.  With the affine value changed as well the
    reference gives other fates, so the two readings are told apart and the library's is the tested one."""
    tag, grey = parameter_images[0]
    pyramid_only = check_driver_against_oracle(driver, oracle, grey, dict(initialSigma=1.0), "initialSigma=1.0")
    both = R.run_driver(driver, grey, dict(initialSigma=1.0, affineInitialSigma=1.0))
    R.same_records(both, pyramid_only, "the Hessian stage does not see the affine value", fields=["x", "y", "s", "pixelDistance", "response", "type", "plane"])
    changed = int((both["fate"] != pyramid_only["fate"]).sum())
    print("initialSigma = 1.0 on %s: %d of %d keypoints change fate when the affine stage uses it too" % (tag, changed, len(both)))
    assert changed > 0


@pytest.mark.parametrize("kw", [{}, dict(initialSigma=1.0), dict(initialSigma=3.1)], ids=["default", "sigma1.0", "sigma3.1"])
def test_planes(driver, oracle, parameter_images, kw):
    """Every plane the detector hands to onHessianKeypointDetected is the oracle's blur plane of that (octave, level), bit for bit,
    and every (octave, level) that holds a keypoint was handed over."""
    matched = set()
    for tag, grey in parameter_images:
        rec, planes = R.run_driver(driver, grey, kw, planes=True)
        o = oracle.OracleRun(grey, keep_planes=True, params=R.params_of(kw))
        want, labels = R.oracle_records(oracle, grey, run=o)
        R.same_records(rec, want, tag)
        assert len(planes) == len(labels) == len(set(labels)) == rec["plane"].max() + 1
        for (octave, level), (pd, plane) in zip(labels, planes):
            assert pd == 2.0 ** octave
            mine = o.plane(octave, 0, level)
            assert plane.shape == mine.shape and np.array_equal(_u32(plane), _u32(mine)), (tag, octave, level)
            matched.add((octave, level))
        hf, hi = o.hessian()
        assert set(zip(hi[:, 1].tolist(), hi[:, 2].tolist())) == set(labels)
    assert len(matched) >= 9 and {l for _, l in matched} == {0, 1, 2}


def oracle_foreign(oracle, grey, kw, points=None, shapes=None):
    """The reference's stages on caller-supplied records, from the oracle library: -> records[RECORD]"""
    handle = oracle.OracleHandle(R.params_of(kw))
    n = len(points) if points is not None else len(shapes)
    out = np.zeros(n, R.RECORD)
    planes = {}
    if points is not None:
        run = oracle.OracleRun(grey, keep_planes=True, detect_only=True, params=R.params_of(kw))
    for k in range(n):
        q = points[k] if points is not None else shapes[k]
        r = out[k]
        r["x"], r["y"], r["s"] = q["x"], q["y"], q["s"]
        if points is not None:
            ol = (int(q["octave"]), int(q["level"]))
            if ol not in planes:
                planes[ol] = run.plane(ol[0], 0, ol[1])
            r["plane"], r["pixelDistance"] = q["plane"], 2.0 ** ol[0]
            conv, U, it = handle.find_affine_shape(planes[ol], q["x"], q["y"], q["s"], r["pixelDistance"])
            if not conv:
                continue
            r["iters"] = it
        else:
            r["plane"], U = -1, q["U"]
        r["U"] = U
        r["fate"] = R.REJECTED
        A = np.array(U, np.float32)
        oracle.lib().ho_rectify(A)
        rej, patch = handle.normalize_affine(grey, q["x"], q["y"], q["s"], A)
        if rej:
            continue
        r["fate"], r["A"], r["desc"] = R.DESCRIBED, A, handle.sift(patch)
    return out


@pytest.mark.parametrize("kw", [{}, dict(mrSize=8.0, maxIterations=10)], ids=["default", "mrSize8_maxIter10"])
def test_foreign_records(driver, oracle, parameter_images, kw):
    """findAffineShape / rectifyAffineTransformationUpIsUp / normalizeAffine / computeSiftDescriptor of the reference on points and
    shapes that no detector produced (near the border, determinant away from 1, both branches of normalizeAffine), against
    OracleHandle's stage functions."""
    from tests.test_describe_regions import foreign_records, patch_window
    tag, grey = parameter_images[0]
    H, W = grey.shape
    _, labels = R.oracle_records(oracle, grey, kw)
    index = {ol: k for k, ol in enumerate(labels)}
    n_oct = 1 + max(o for o, _ in labels)
    assert n_oct == 5

    reg = foreign_records(H, W, n_oct, 1.0, 53, per_plane=16)
    reg = reg[[ol in index for ol in zip(reg["octave"].tolist(), reg["level"].tolist())]]
    points = np.zeros(len(reg), np.dtype(R.POINT_IN.descr + [("octave", "<i4"), ("level", "<i4")]))
    for k in ("x", "y", "s", "octave", "level"):
        points[k] = reg[k]
    points["plane"] = [index[ol] for ol in zip(reg["octave"].tolist(), reg["level"].tolist())]
    pin = np.zeros(len(points), R.POINT_IN)
    for k in R.POINT_IN.names:
        pin[k] = points[k]
    got = R.run_driver(driver, grey, kw, points=pin)
    R.same_records(got, oracle_foreign(oracle, grey, kw, points=points), "points")
    n = np.bincount(got["fate"], minlength=3)
    assert len(got) > 300 and n.min() >= 20, n

    reg = foreign_records(H, W, n_oct, 1.0, 54, per_plane=16, shapes=True)
    shapes = np.zeros(len(reg), R.SHAPE_IN)
    for k in ("x", "y", "s"):
        shapes[k] = reg[k]
    shapes["U"] = np.stack([reg[k] for k in ("a11", "a12", "a21", "a22")], 1)
    got = R.run_driver(driver, grey, kw, shapes=shapes)
    R.same_records(got, oracle_foreign(oracle, grey, kw, shapes=shapes), "shapes")
    n = np.bincount(got["fate"], minlength=3)
    assert len(got) > 300 and n[0] == 0 and n[1:].min() >= 20, n
    branches = {patch_window(s, R.params_of(kw).mrSize)[1] for s in got["s"][got["fate"] == R.DESCRIBED]}
    assert branches == {False, True}, branches


def test_poisoned_twins(driver, hesaff_ref, oracle):
    """Built with -DSHIM_POISON every fresh Mat buffer starts as 0xFF bytes (NaN as float).  The same output means that no value
    the reference never wrote reaches a result: the 1-pixel response border, the patch and workspace buffers."""
    import hesaff_amd
    poisoned_driver, poisoned_main = R.binary("ref_driver_poison"), R.binary("hesaff_ref_poison")
    for name in ("band_160x120", "probe_vga"):
        path = os.path.join(R.GOLD, name + ".pgm")
        assert R.run_hesaff_ref(hesaff_ref, path) == R.run_hesaff_ref(poisoned_main, path), name
        grey = oracle.gray_from_u8(hesaff_amd.read_pnm(path))
        for kw in ({}, dict(mrSize=1.0)):   # (mrSize = 1: the direct branch of normalizeAffine as well)
            a, pa = R.run_driver(driver, grey, kw, planes=True)
            b, pb = R.run_driver(poisoned_driver, grey, kw, planes=True)
            assert a.tobytes() == b.tobytes() and len(a) > 300, (name, kw)
            assert len(pa) == len(pb) and all(x[1].tobytes() == y[1].tobytes() for x, y in zip(pa, pb)), (name, kw)


# ------------------------------------------------------------------ fixtures ------------------------------------------------------------------

def fixture_grey(name):
    """the float32 plane a fixture of records was made on"""
    if name == "float":
        return R.float_fixture_plane()
    image = R.manifest()["reference"]["fixtures"]["ref_%s.npz" % name]["image"]
    return R.grey_of(R.fixture_image() if image == "band_160x120" else R.sparse_image())


@pytest.mark.parametrize("name", SET_NAMES + ["float"])
def test_oracle_reproduces_record_fixtures(oracle, name):
    """needs no reference binary: the committed records are the oracle's, every field as bits"""
    want = R.load_fixture(name)["records"]
    entry = R.manifest()["reference"]["fixtures"]["ref_%s.npz" % name]
    assert R.records_md5(want) == entry["records_md5"] and len(want) == entry["records"]
    assert int((want["fate"] == R.DESCRIBED).sum()) == entry["described"] >= 30
    got, _ = R.oracle_records(oracle, fixture_grey(name), R.PARAM_SETS.get(name, {}))
    R.same_records(got, want, name)


def test_oracle_reproduces_plane_and_foreign_fixtures(oracle):
    grey = R.grey_of(R.fixture_image())
    o = oracle.OracleRun(grey, keep_planes=True)
    _, labels = R.oracle_records(oracle, grey, run=o)
    seen = []
    for octave in range(3):
        z = R.load_fixture("planes_o%d" % octave)
        assert float(z["pixelDistance"]) == 2.0 ** octave
        for level in z["levels"].tolist():
            assert np.array_equal(_u32(z["L%d" % level]), _u32(o.plane(octave, 0, level))), (octave, level)
            seen.append((octave, level))
    assert seen == labels and len(seen) == 8
    z = R.load_fixture("foreign")
    assert [labels[k] for k in z["points"]["plane"].tolist()] == list(zip(z["points"]["octave"].tolist(), z["points"]["level"].tolist()))
    R.same_records(oracle_foreign(oracle, grey, {}, points=z["points"]), z["point_records"], "foreign points")
    R.same_records(oracle_foreign(oracle, grey, {}, shapes=z["shapes"]), z["shape_records"], "foreign shapes")
    for rec, fates in ((z["point_records"], (0, 1, 2)), (z["shape_records"], (1, 2))):
        assert all((rec["fate"] == f).sum() >= 20 for f in fates)


def test_regenerated_fixtures_are_identical(driver, hesaff_ref):
    """the committed fixtures are what the binaries of this build write: every array byte for byte, and the manifest block"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("make_ref_golden", os.path.join(R.GOLD, "make_ref_golden.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    arrays, block = mod.generate(driver, hesaff_ref)
    committed = sorted(f for f in os.listdir(R.GOLD) if f.startswith("ref_") and f.endswith(".npz"))
    assert committed == sorted("ref_%s.npz" % k for k in arrays)
    for name, want in arrays.items():
        got = R.load_fixture(name)
        assert sorted(got) == sorted(want), name
        for k in want:
            a, b = np.asarray(want[k]), got[k]
            assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes(), (name, k)
    import json
    assert json.loads(json.dumps(block)) == R.manifest()["reference"]


# ------------------------------------------------------------------ GPU: the library against the fixtures ------------------------------------------------------------------

def _params(**kw):
    import hesaff_amd
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def expected_regions_and_keys(rec):
    """records[RECORD] of the reference -> what hesaff_detect_regions returns for them (REGION_DTYPE without octave and level,
    which the reference does not name; KEYPOINT_DTYPE)"""
    from hesaff_amd import _binding
    reg = np.zeros(len(rec), _binding.REGION_DTYPE)
    for k in ("x", "y", "s", "pixelDistance", "response", "type", "iters"):
        reg[k] = rec[k]
    for j, k in enumerate(("a11", "a12", "a21", "a22")):
        reg[k] = rec["U"][:, j]
    reg["outcome"] = rec["fate"]
    d = rec["fate"] == R.DESCRIBED
    reg["key"] = -1
    reg["key"][d] = np.arange(int(d.sum()), dtype=np.int32)
    keys = np.zeros(int(d.sum()), _binding.KEYPOINT_DTYPE)
    for k in ("x", "y", "s", "response", "type", "desc"):
        keys[k] = rec[k][d]
    for j, k in enumerate(("a11", "a12", "a21", "a22")):
        keys[k] = rec["A"][d, j]
    return reg, keys


def same_struct(got, want, what, skip=()):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if len(got) == 0:
        return
    for name in got.dtype.names:
        if name in skip:
            continue
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        ne = (a != b).reshape(len(got), -1).any(axis=1)
        if ne.any():
            i = int(np.argmax(ne))
            raise AssertionError("%s: field %s differs in %d of %d records, first %d: %r vs %r" % (what, name, int(ne.sum()), len(got), i,
                                                                                               got[name][i], want[name][i]))


def check_regions_against_records(regions, keys, rec, what):
    want_r, want_k = expected_regions_and_keys(rec)
    same_struct(regions, want_r, what + ": regions", skip=("octave", "level"))
    same_struct(keys, want_k, what + ": keys")
    # (octave, level) names the plane the reference handed to its callback: octave from pixelDistance, and numbering the library's
    # pairs in order of first appearance gives the reference's buffer numbers
    assert np.array_equal(regions["pixelDistance"], np.float32(2.0) ** regions["octave"].astype(np.float32)), what
    seen = {}
    mine = [seen.setdefault(ol, len(seen)) for ol in zip(regions["octave"].tolist(), regions["level"].tolist())]
    assert mine == rec["plane"].tolist(), what + ": (octave, level) against the reference's plane numbers"
    assert np.isin(regions["level"], (0, 1, 2)).all() and list(seen) == sorted(seen), what


@pytest.mark.gpu
@pytest.mark.parametrize("name", SET_NAMES)
def test_gpu_parameter_sets(name):
    """detect_regions and detect_batch under each parameter set: every field of every record and key is the compiled reference's.
    The .hesaff.sift text is compared where the reference can write one: its main takes no parameters, so at the defaults."""
    import hesaff_amd
    rec = R.load_fixture(name)["records"]
    u8 = R.fixture_image() if R.manifest()["reference"]["fixtures"]["ref_%s.npz" % name]["image"] == "band_160x120" else R.sparse_image()
    p = _params(**R.PARAM_SETS[name])
    with hesaff_amd.HesaffContext(p, device=0) as c:
        (regions, keys), = c.detect_regions([u8])
        (n_hess, keys_b), = c.detect_batch([u8])
        text = hesaff_amd.format_sift(keys_b, p.mrSize)
    check_regions_against_records(regions, keys, rec, name)
    assert n_hess == len(rec) and keys_b.tobytes() == keys.tobytes(), name
    if name == "default":
        # hesaff_ref's own file (test_whole_files: the committed one is byte-identical to it)
        assert R.manifest()["reference"]["hesaff_ref_sift"]["band_160x120"]["sift_md5"] == hashlib.md5(text).hexdigest()
        assert text == open(os.path.join(R.GOLD, "band_160x120.hesaff.sift"), "rb").read()


@pytest.mark.gpu
def test_gpu_float_fixture(ctx):
    rec = R.load_fixture("float")["records"]
    plane = R.float_fixture_plane()
    (regions, keys), = ctx.detect_regions_f32([plane])
    (n_hess, keys_b), = ctx.detect_batch_f32([plane])
    check_regions_against_records(regions, keys, rec, "float plane")
    assert n_hess == len(rec) and keys_b.tobytes() == keys.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("from_", ["points", "shapes"])
def test_gpu_foreign_fixture(ctx, from_):
    """describe_regions on keypoints that no detector produced, against the reference's own stages on the same records"""
    from hesaff_amd import _binding
    import hesaff_amd
    z = R.load_fixture("foreign")
    q, rec = (z["points"], z["point_records"]) if from_ == "points" else (z["shapes"], z["shape_records"])
    rin = np.zeros(len(q), _binding.REGION_DTYPE)
    for k in ("x", "y", "s"):
        rin[k] = q[k]
    if from_ == "points":
        rin["octave"], rin["level"] = q["octave"], q["level"]
    else:
        for j, k in enumerate(("a11", "a12", "a21", "a22")):
            rin[k] = q["U"][:, j]
    (regions, keys), = ctx.describe_regions([R.fixture_image()], [rin], hesaff_amd.FROM_POINTS if from_ == "points" else hesaff_amd.FROM_SHAPES)
    want_r, want_k = expected_regions_and_keys(rec)
    want_r["octave"], want_r["level"] = rin["octave"], rin["level"]
    want_r["pixelDistance"] = np.float32(2.0) ** rin["octave"].astype(np.float32)
    same_struct(regions, want_r, from_ + ": regions")
    same_struct(keys, want_k, from_ + ": keys")


@pytest.mark.gpu
def test_gpu_pyramid_planes(ctx):
    """the blur planes of ctx.pyramid against the planes the reference's detector handed to its callback"""
    pyr = ctx.pyramid(R.fixture_image())
    n = 0
    for octave in range(3):
        z = R.load_fixture("planes_o%d" % octave)
        for level in z["levels"].tolist():
            got, want = pyr[octave][0][level], z["L%d" % level]
            assert got.shape == want.shape and np.array_equal(_u32(got), _u32(want)), (octave, level)
            n += 1
    assert n == 8
