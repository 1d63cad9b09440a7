"""The compiled reference (oracle/_ref/, built by `make -C oracle ref`) as seen from Python, and the
fixtures it wrote into tests/golden/ (tests/golden/make_ref_golden.py).

Test infrastructure only.  The binaries are static, so a tree that carries them runs them anywhere;
the reference's sources are needed only to build them.
"""
import hashlib
import json
import os
import subprocess
import tempfile
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REF_OUT = os.path.join(ROOT, "oracle", "_ref")
REFERENCE = os.environ.get("HESAFF_REFERENCE", "/root/reference")

SMALL_BANDS = ((1.5, 40.0), (3.0, 40.0), (6.0, 50.0))
GOLDEN_PGMS = ["band_131x77", "band_160x120", "band_96x96", "thin_12x40", "tiny_20x15"]

# struct Record of oracle/ref_driver.cpp
NOT_CONVERGED, REJECTED, DESCRIBED = 0, 1, 2
RECORD = np.dtype([("x", "<f4"), ("y", "<f4"), ("s", "<f4"), ("pixelDistance", "<f4"), ("response", "<f4"),
                   ("type", "<i4"), ("fate", "<i4"), ("iters", "<i4"), ("plane", "<i4"),
                   ("U", "<f4", (4,)), ("A", "<f4", (4,)), ("desc", "u1", (128,))])
assert RECORD.itemsize == 196
POINT_IN = np.dtype([("plane", "<i4"), ("x", "<f4"), ("y", "<f4"), ("s", "<f4")])
SHAPE_IN = np.dtype([("x", "<f4"), ("y", "<f4"), ("s", "<f4"), ("U", "<f4", (4,))])

# the reference's defaults (pyramid.h:32-40, affine.h:37-45, siftdesc.h:25-31), in float32 as it computes them
DEFAULTS = dict(threshold=float(np.float32(16.0) / np.float32(3.0)), edgeEigenValueRatio=10.0, initialSigma=float(np.float32(1.6)),
                maxIterations=16, convergenceThreshold=float(np.float32(0.05)),
                mrSize=float(np.float32(3.0) * np.sqrt(np.float32(3.0))), maxBinValue=float(np.float32(0.2)), upscaleInputImage=0)

# name -> parameters that differ from the defaults.  Every set of test_gpu_parity.NONDEFAULT that does not up-sample the input
# (the reference's doubleImage reads outside its buffer), and initialSigma below and far above the usual.
PARAM_SETS = {
    "default": {},
    "threshold9": dict(threshold=9.0),
    "threshold2.5_edge4": dict(threshold=2.5, edgeEigenValueRatio=4.0),
    "mrSize1": dict(mrSize=1.0),
    "mrSize2_maxBin0.1": dict(mrSize=2.0, maxBinValue=0.1),
    "mrSize9": dict(mrSize=9.0),
    "maxIter3": dict(maxIterations=3),
    "maxIter40_conv0.01": dict(maxIterations=40, convergenceThreshold=0.01),
    "conv0.2": dict(convergenceThreshold=0.2),
    "sigma1.0": dict(initialSigma=1.0),
    "sigma2.0": dict(initialSigma=2.0),
    "sigma0.62": dict(initialSigma=0.62),
    "sigma3.1": dict(initialSigma=3.1),
    "sigma0.45_threshold3": dict(initialSigma=0.45, threshold=3.0),
    "maxBin0.05": dict(maxBinValue=0.05),
    "maxBin1.0": dict(maxBinValue=1.0),
}


def params_of(kw):
    """the reference-side fields of hesaff_params for a parameter set, as tests/_oracle.set_params reads them"""
    return types.SimpleNamespace(**{**DEFAULTS, **kw})


def binary(name):
    """Path of oracle/_ref/<name>.  Absent binary: a failure where the reference's sources are present (build() should have made
    it), a skip only where they are absent too."""
    import pytest
    path = os.path.join(REF_OUT, name)
    if os.path.isfile(path) and os.access(path, os.X_OK):
        return path
    if os.path.isdir(REFERENCE):
        pytest.fail("oracle/_ref/%s is missing although the reference sources are at %s: run __graft_entry__.build() "
                    "or `make -C oracle ref`" % (name, REFERENCE))
    pytest.skip("neither oracle/_ref/%s nor the reference sources (%s) are here" % (name, REFERENCE))


def _run(args, what):
    r = subprocess.run(args, capture_output=True, text=True)
    # the reference's asserts are enabled: an abort is a failure of the test that ran it
    assert r.returncode == 0, "%s: exit status %d\nstdout: %s\nstderr: %s" % (what, r.returncode, r.stdout[-2000:], r.stderr[-2000:])
    return r.stdout


def read_planes(path):
    """planes=FILE of ref_driver -> list of (pixelDistance, plane[rows, cols])"""
    raw = open(path, "rb").read()
    out, at = [], 0
    while at < len(raw):
        rows, cols = np.frombuffer(raw, "<i4", 2, at)
        pd = float(np.frombuffer(raw, "<f4", 1, at + 8)[0])
        n = int(rows) * int(cols)
        out.append((pd, np.frombuffer(raw, "<f4", n, at + 12).reshape(rows, cols).copy()))
        at += 12 + 4 * n
    return out


def run_driver(exe, gray, kw=None, planes=False, points=None, shapes=None):
    """ref_driver on a float32 grey plane.  kw: parameters by the driver's names (affineInitialSigma included).
    -> records[RECORD], or (records, planes) with planes=True"""
    gray = np.ascontiguousarray(gray, np.float32)
    assert gray.ndim == 2
    with tempfile.TemporaryDirectory(prefix="hesaff_ref_") as tmp:
        src, out = os.path.join(tmp, "in.f32"), os.path.join(tmp, "out.rec")
        gray.tofile(src)
        args = [exe, src, str(gray.shape[0]), str(gray.shape[1]), out]
        for k, v in (kw or {}).items():
            args.append("%s=%d" % (k, v) if k == "maxIterations" else "%s=%.9g" % (k, float(np.float32(v))))
        if planes:
            args.append("planes=" + os.path.join(tmp, "planes.bin"))
        if points is not None:
            np.ascontiguousarray(points, POINT_IN).tofile(os.path.join(tmp, "points.bin"))
            args.append("points=" + os.path.join(tmp, "points.bin"))
        if shapes is not None:
            np.ascontiguousarray(shapes, SHAPE_IN).tofile(os.path.join(tmp, "shapes.bin"))
            args.append("shapes=" + os.path.join(tmp, "shapes.bin"))
        _run(args, "ref_driver %s %s" % (gray.shape, kw or {}))
        rec = np.fromfile(out, RECORD)
        if planes:
            return rec, read_planes(os.path.join(tmp, "planes.bin"))
        return rec


def run_hesaff_ref(exe, pgm_path):
    """The reference's own main on a copy of the PGM -> (n_hessian, n_described, bytes of the .hesaff.sift it wrote)"""
    import re
    import shutil
    with tempfile.TemporaryDirectory(prefix="hesaff_ref_") as tmp:
        p = os.path.join(tmp, os.path.basename(pgm_path))
        shutil.copy(pgm_path, p)
        out = _run([exe, p], "hesaff_ref " + os.path.basename(pgm_path))
        m = re.search(r"Detected (\d+) keypoints and (\d+) affine shapes", out)
        assert m, out
        return int(m.group(1)), int(m.group(2)), open(p + ".hesaff.sift", "rb").read()


def oracle_records(oracle, gray, kw=None, run=None):
    """What ref_driver writes, computed by the oracle alone: OracleRun -> records[RECORD]"""
    o = run if run is not None else oracle.OracleRun(np.ascontiguousarray(gray, np.float32), params=params_of(kw or {}))
    hf, hi = o.hessian()
    U, ci = o.affine()
    g, t, d = o.keys()
    src = o.key_sources()
    rec = np.zeros(o.n_hessian, RECORD)
    for j, name in enumerate(["x", "y", "s", "pixelDistance", "response"]):
        rec[name] = hf[:, j]
    rec["type"] = hi[:, 0]
    conv = ci[:, 0] != 0
    rec["fate"] = conv.astype(np.int32)
    rec["fate"][src] = DESCRIBED
    rec["iters"] = np.where(conv, ci[:, 1], 0)
    rec["U"] = np.where(conv[:, None], U, np.float32(0))
    rec["A"][src] = g[:, 3:7]
    rec["desc"][src] = d
    # planes in order of first appearance, as the driver numbers the buffers it is handed
    seen = {}
    for k, ol in enumerate(zip(hi[:, 1].tolist(), hi[:, 2].tolist())):
        rec["plane"][k] = seen.setdefault(ol, len(seen))
    return rec, list(seen)


def same_records(got, want, what, fields=None):
    """every field of every record, floats as bit patterns"""
    assert got.dtype == want.dtype == RECORD
    assert len(got) == len(want), "%s: %d records, expected %d" % (what, len(got), len(want))
    if len(got) == 0:
        return
    for name in fields or RECORD.names:
        a, b = got[name], want[name]
        if a.dtype == np.float32:
            a, b = a.view(np.uint32), b.view(np.uint32)
        ne = (a != b).reshape(len(got), -1).any(axis=1)
        if ne.any():
            i = int(np.argmax(ne))
            raise AssertionError("%s: field %s differs in %d of %d records, first %d: %r vs %r (fate %d vs %d)" % (
                what, name, int(ne.sum()), len(got), i, got[name][i], want[name][i], got["fate"][i], want["fate"][i]))
    if fields is None:
        assert got.tobytes() == want.tobytes(), what


def records_md5(rec):
    return hashlib.md5(np.ascontiguousarray(rec).tobytes()).hexdigest()


# ---- fixtures under tests/golden/ ----

def fixture_path(name):
    return os.path.join(GOLD, "ref_%s.npz" % name)


def load_fixture(name):
    with np.load(fixture_path(name)) as z:
        return {k: z[k] for k in z.files}


def manifest():
    with open(os.path.join(GOLD, "manifest.json")) as f:
        return json.load(f)


def fixture_image():
    """the 8-bit grey image every fixture is made on (tests/golden/band_160x120.pgm), without the library: P5, no comments"""
    import re
    raw = open(os.path.join(GOLD, "band_160x120.pgm"), "rb").read()
    m = re.match(rb"P5\s+(\d+)\s+(\d+)\s+255\s", raw)
    w, h = int(m.group(1)), int(m.group(2))
    return np.frombuffer(raw, np.uint8, w * h, m.end()).reshape(h, w).copy()


def grey_of(u8):
    """hesaff.cpp:138-148 on a grey image read as B = G = R: (float(v) + v + v) / 3.0f, in float32"""
    v = u8.astype(np.float32)
    return ((v + v + v) / np.float32(3.0)).astype(np.float32)


def float_fixture_plane():
    return (grey_of(fixture_image()) * np.float32(1.37) - np.float32(300.75)).astype(np.float32)


def sparse_image():
    """the image for a parameter set that leaves fewer than 30 described keypoints on band_160x120"""
    from hesaff_amd.synth import band_noise_image
    return band_noise_image(200, 260, 92, SMALL_BANDS)
