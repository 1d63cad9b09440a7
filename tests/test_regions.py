"""hesaff_detect_regions and the reference's two detector callbacks (pyramid.h:43-47, affine.h:48-58, chained by
hesaff.cpp:66-105): one hesaff_region record per Hessian keypoint, bit for bit against the oracle's per-keypoint dumps
(tests/golden/*_stages.npz and OracleRun), and the C++ callback interface of hesaff_amd/csrc/hesaff.hpp replayed from them.

The CPU tests check the layout, the header and the argument checks; the GPU tests (marked) the records themselves."""
import ctypes as C
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from hesaff_amd.synth import band_noise_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REPLAY_SRC = os.path.join(ROOT, "tests", "native", "callbacks_replay.cpp")
SMALL_BANDS = ((1.5, 40.0), (3.0, 40.0), (6.0, 50.0))
F_HESS = ("x", "y", "s", "pixelDistance", "response")
I_HESS = ("type", "octave", "level")
F_AFF = ("a11", "a12", "a21", "a22")


# ------------------------------------------------------------------ CPU ------------------------------------------------------------------

def test_region_record_layout():
    L = hesaff_amd.load_library()
    L.hesaff_sizeof_region.restype = C.c_size_t
    assert L.hesaff_sizeof_region() == 64 == C.sizeof(_binding.Region) == _binding.REGION_DTYPE.itemsize
    for name, _ in _binding.Region._fields_:
        assert _binding.REGION_DTYPE.fields[name][1] == getattr(_binding.Region, name).offset, name
    assert [n for n, _ in _binding.Region._fields_] == list(_binding.REGION_DTYPE.names)
    assert L.hesaff_abi_version() == _binding.ABI_VERSION == 8


def test_callback_interface_compiles():
    """A translation unit that subclasses HessianKeypointCallback and AffineShapeCallback through hesaff.hpp and installs them
    with the two setters (the way code written against the reference does) compiles."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", REPLAY_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_detect_regions_argument_errors():
    L = hesaff_amd.load_library()
    res = (_binding._RegionResult * 1)()
    one = (C.c_int * 1)(16)
    img = (C.c_void_p * 1)(None)
    # no context: HESAFF_ERR_ARG, not a crash (a context cannot be made without a GPU)
    assert L.hesaff_detect_regions(None, 0, None, None, None, None, None, None) == -2
    assert L.hesaff_detect_regions(None, 1, img, one, one, None, None, res) == -2


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _eq(got, want, what):
    got = np.asarray(got); want = np.asarray(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    ne = got != want
    if ne.ndim > 1:
        ne = ne.any(axis=tuple(range(1, ne.ndim)))
    if ne.any():
        i = int(np.argmax(ne))
        raise AssertionError("%s: %d of %d rows differ, first row %d: %s vs %s" % (what, int(ne.sum()), len(ne), i, got[i], want[i]))


def check_regions(regions, hess_f, hess_i, aff_U, aff_i, key_src, what):
    """regions (REGION_DTYPE) against the oracle's per-keypoint dumps, float fields as uint32 bit patterns."""
    n = len(hess_f)
    assert len(regions) == n, (what, len(regions), n)
    _eq(_u32(np.stack([regions[k] for k in F_HESS], 1).reshape(n, 5)), _u32(hess_f[:, :5]), what + ": x y s pixelDistance response")
    _eq(np.stack([regions[k] for k in I_HESS], 1).reshape(n, 3), hess_i[:, :3], what + ": type octave level")
    _eq(_u32(np.stack([regions[k] for k in F_AFF], 1).reshape(n, 4)), _u32(aff_U), what + ": U (un-rectified; 0 when not converged)")
    _eq(np.stack([(regions["outcome"] >= 1).astype(np.int32), regions["iters"]], 1).reshape(n, 2), aff_i, what + ": converged, iters")
    want_key = np.full(n, -1, np.int32)
    want_key[np.asarray(key_src, np.int64)] = np.arange(len(key_src), dtype=np.int32)
    _eq(regions["key"], want_key, what + ": key (inverse of the oracle's key sources)")
    _eq(regions["outcome"] == 2, want_key >= 0, what + ": outcome 2 <=> described")
    assert np.isin(regions["outcome"], (0, 1, 2)).all() and (regions["reserved"] == 0).all(), what


def check_against_oracle(regions, oracle_run, what):
    hf, hi = oracle_run.hessian()
    U, ai = oracle_run.affine()
    check_regions(regions, hf, hi, U, ai, oracle_run.key_sources(), what)


def check_keys(c, img, regions, keys, what):
    (n_hess, keys_b), = c.detect_batch([img])
    assert keys.tobytes() == keys_b.tobytes(), what + ": keys differ from detect_batch's"
    assert len(regions) == n_hess and len(keys) == int((regions["outcome"] == 2).sum()), what


GOLDEN_STAGES = sorted(os.path.basename(p)[:-len("_stages.npz")] for p in glob.glob(os.path.join(GOLD, "*_stages.npz")))


@pytest.mark.gpu
@pytest.mark.parametrize("name", GOLDEN_STAGES)
def test_golden_stage_fixtures(ctx, name):
    """Every golden image with a stage dump (thin_12x40 included: no keypoint at all)."""
    img = hesaff_amd.read_pnm(os.path.join(GOLD, name + ".pgm"))
    st = np.load(os.path.join(GOLD, name + "_stages.npz"))
    (regions, keys), = ctx.detect_regions([img])
    check_regions(regions, st["hess_f"], st["hess_i"], st["aff_U"], st["aff_i"], st["key_src"], name)
    check_keys(ctx, img, regions, keys, name)


@pytest.mark.gpu
def test_oracle_vga_and_fhd(ctx, oracle):
    """The probe photograph-like VGA image and a synthetic FHD image in one call, against OracleRun; all three outcomes occur."""
    vga = hesaff_amd.read_pnm(os.path.join(GOLD, "probe_vga.pgm"))
    fhd = band_noise_image(1080, 1920, 77)
    res = ctx.detect_regions([vga, fhd])
    seen = set()
    for img, (regions, keys), what in zip((vga, fhd), res, ("probe_vga", "fhd")):
        check_against_oracle(regions, oracle.OracleRun(oracle.gray_from_u8(img)), what)
        check_keys(ctx, img, regions, keys, what)
        seen |= set(np.unique(regions["outcome"]).tolist())
    assert seen == {0, 1, 2}, seen


@pytest.mark.gpu
def test_chunks_and_mixed_sizes(ctx):
    """11 images of three sizes through max_batch = 4 (several chunks per size, pinned block per chunk): each image's records
    and keys equal those of the image alone."""
    sizes = [(120, 160), (97, 131), (150, 90)]
    imgs = [band_noise_image(*sizes[i % 3], 300 + i, SMALL_BANDS) for i in range(11)]
    p = hesaff_amd.default_params(); p.max_batch = 4
    with hesaff_amd.HesaffContext(p, device=0) as c4:
        res = c4.detect_regions(imgs)
        batch = c4.detect_batch(imgs)
    total = 0
    for i, (img, (regions, keys), (n_hess, keys_b)) in enumerate(zip(imgs, res, batch)):
        (r1, k1), = ctx.detect_regions([img])
        assert regions.tobytes() == r1.tobytes(), "image %d: records differ from the single-image call" % i
        assert keys.tobytes() == k1.tobytes() == keys_b.tobytes(), "image %d: keys" % i
        assert len(regions) == n_hess
        total += len(regions)
    assert total > 500


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(maxIterations=2), dict(upscaleInputImage=1), dict(threshold=3.0)],
                         ids=lambda kw: ",".join("%s=%g" % kv for kv in kw.items()))
def test_non_default_parameters(oracle, kw):
    p = _params(**kw)
    imgs = [band_noise_image(300, 420, 91), band_noise_image(200, 260, 92, SMALL_BANDS)]
    with hesaff_amd.HesaffContext(p, device=0) as c2:
        res = c2.detect_regions(imgs)
        for img, (regions, keys) in zip(imgs, res):
            check_against_oracle(regions, oracle.OracleRun(oracle.gray_from_u8(img), params=p), str(kw))
            check_keys(c2, img, regions, keys, str(kw))
    regions = np.concatenate([r for r, _ in res])
    assert len(regions) > 100
    if "maxIterations" in kw:
        assert regions["iters"].max() <= 1 and (regions["outcome"] == 0).mean() > 0.5
    if "upscaleInputImage" in kw:
        assert set(regions["pixelDistance"][regions["octave"] == 0].tolist()) == {0.5}


@pytest.mark.gpu
def test_fast_mode_regions_equal_parity_mode(ctx):
    """fast = 2 changes descriptors of large windows only: detection, affine shapes and the set of described keypoints - every
    field of every record - are parity mode's."""
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, "probe_vga.pgm")), band_noise_image(300, 420, 91)]
    with hesaff_amd.HesaffContext(_params(fast=2), device=0) as cf:
        fast = cf.detect_regions(imgs)
    parity = ctx.detect_regions(imgs)
    for (rf, kf), (rp, kp) in zip(fast, parity):
        assert rf.tobytes() == rp.tobytes()
        assert len(kf) == len(kp)


def _build_replay(tmp_path):
    exe = str(tmp_path / "callbacks_replay")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, REPLAY_SRC, "-L" + lib_dir, "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    return exe


def _parse_replay(out):
    """-> list per image of (callback lines, keys bytes, (g_numberOfPoints, g_numberOfAffinePoints, keys.size()))"""
    images = []
    for line in out.splitlines():
        if line.startswith("I "):
            images.append([[], b"", None])
        elif line[:2] in ("H ", "A "):
            images[-1][0].append(line)
        elif line.startswith("K "):
            images[-1][1] += bytes.fromhex(line[2:])
        elif line.startswith("N "):
            images[-1][2] = tuple(int(v) for v in line[2:].split())
        else:
            raise AssertionError("unexpected line from callbacks_replay: %r" % line)
    return images


def _expected_stream(o):
    """The oracle's call sequence of hesaff.cpp:66-105: onHessianKeypointDetected for each keypoint, onAffineShapeFound right
    after it when findAffineShape converged - in the replay program's print format."""
    hf, hi = o.hessian()
    U, ai = o.affine()
    b = _u32(hf); bu = _u32(U)
    lines = []
    for k in range(len(hf)):
        lines.append("H %08x %08x %08x %08x %d %08x %d %d" % (b[k, 0], b[k, 1], b[k, 2], b[k, 3], hi[k, 0], b[k, 4], hi[k, 1], hi[k, 2]))
        if ai[k, 0]:
            lines.append("A %08x %08x %08x %08x %08x %08x %08x %08x %d %08x %d" % (b[k, 0], b[k, 1], b[k, 2], b[k, 3], bu[k, 0], bu[k, 1],
                                                                                 bu[k, 2], bu[k, 3], hi[k, 0], b[k, 4], ai[k, 1]))
    return lines


@pytest.mark.gpu
def test_cpp_callbacks_replay(ctx, oracle, tmp_path):
    """tests/native/callbacks_replay.cpp subclasses both callbacks through hesaff.hpp: its callback stream is the oracle's, in
    order and interleaving, and its keys are detect_batch's - with and without callbacks installed."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = _build_replay(tmp_path)
    paths = [os.path.join(GOLD, "band_160x120.pgm"), os.path.join(GOLD, "probe_vga.pgm")]
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run([exe, "--plain"] + paths, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr
    got, got_plain = _parse_replay(r.stdout), _parse_replay(plain.stdout)
    assert len(got) == len(got_plain) == 2
    n_affine = 0
    for path, (stream, keys, counts), (stream_p, keys_p, counts_p) in zip(paths, got, got_plain):
        img = hesaff_amd.read_pnm(path)
        o = oracle.OracleRun(oracle.gray_from_u8(img))
        want = _expected_stream(o)
        assert len(stream) == len(want), (path, len(stream), len(want))
        for k, (a, b) in enumerate(zip(stream, want)):
            assert a == b, "%s: callback %d: %s vs oracle %s" % (path, k, a, b)
        (n_hess, keys_b), = ctx.detect_batch([img])
        assert keys == keys_b.tobytes() == keys_p, path
        assert stream_p == []
        n_affine += len(keys_b)
        assert counts == (n_hess, n_affine, len(keys_b)) and counts_p == counts, (path, counts, counts_p)
