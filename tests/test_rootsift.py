"""GPU suite of the descriptor modes (hesaff_set_descriptor, include/hesaff_amd.h).  The reference is tests/rootsift_ref.py over
the CPU oracle's values: the oracle's un-normalised histogram -> normalize / clip / normalize and the RootSIFT epilogue in numpy
float32 -> bytes.  Nothing is compared with mode 0 of the library itself, and everything is held bit for bit; the one inequality is
the fast-mode test's derived bound on the norm, where no oracle exists."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import DESC_ROOTSIFT, DESC_SIFT, FROM_POINTS, FROM_SHAPES, ORI_DOMINANT, _binding
from tests import orientation_ref as R
from tests import rootsift_ref as RS
from tests import stage_inputs as SI
from tests.test_rootsift_host import SAT_AT_1, SAT_AT_DEFAULT

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
KEY = _binding.KEYPOINT_DTYPE
E2E_IMAGES = ["band_160x120", "tiny_20x15", "band_96x96"]
NOT_DESC = [f for f in KEY.names if f != "desc"]


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


def _renumbered(records):
    out = records.copy()
    d = out["outcome"] == 2
    out["key"] = -1
    out["key"][d] = np.arange(int(d.sum()), dtype=np.int32)
    return out


def _identity(keys):
    return [tuple(_u32(np.array([k[f] for f in ("x", "y", "s", "response")], np.float32)).tolist()) for k in keys]


@pytest.fixture(scope="module")
def rctx():
    """a context of its own in RootSIFT mode (the session's context stays in mode 0)"""
    with hesaff_amd.HesaffContext(device=0) as c:
        assert c.descriptor == DESC_SIFT
        c.set_descriptor("rootsift")
        assert c.descriptor == DESC_ROOTSIFT
        yield c


_golden = {}


def golden(oracle, name):
    """image, float grey plane, the RootSIFT reference chain's (regions, keys, n_hessian) and the SIFT chain's keys: computed once"""
    if name not in _golden:
        img = hesaff_amd.read_pnm(os.path.join(GOLD, name + ".pgm"))
        gray = oracle.gray_from_u8(img)
        _golden[name] = (img, gray) + RS.chain(oracle, gray, RS.ROOTSIFT) + (RS.chain(oracle, gray, RS.SIFT)[1],)
    return _golden[name]


_stage = {}


def stage_reference(oracle, max_bin):
    """the 67 interleaved patches under the oracle with this maxBinValue: (hist, oracle's SIFT bytes, helper's RootSIFT bytes, clipped)"""
    key = float(np.float32(max_bin))
    if key not in _stage:
        handle = oracle.OracleHandle(_params(maxBinValue=max_bin))
        parts = [handle.sift_parts(p) for p in SI.interleaved(67)]
        hist = np.stack([h for _, h, _ in parts])
        _stage[key] = (hist, np.stack([d for _, _, d in parts]), np.stack([RS.to_bytes(h, max_bin, RS.ROOTSIFT) for h in hist]),
                       np.array([RS.normalized(h, max_bin)[1] for h in hist]))
    return _stage[key]


# ---------------------------------------------------------------- the stage operator

@pytest.mark.gpu
@pytest.mark.parametrize("max_bin", [0.2, 0.5, 1.0])
def test_stage_on_constructed_patches(oracle, max_bin):
    """hesaff_stage_sift_mode in mode 1 on stage_inputs.interleaved(67) - 16 wavefronts of four keypoints and a tail of three,
    clipped and unclipped keypoints and zero histograms mixed within the wavefronts (tests/test_rootsift_host.py counts them) - at
    maxBinValue 0.2, 0.5 and 1.0 (nothing clipped: the single normalisation alone): the helper's bytes, all at once and one patch
    per call; the histogram the kernel started from is the oracle's as bits."""
    patches = SI.interleaved(67)
    hist, _, want, clipped = stage_reference(oracle, max_bin)
    zero = ~hist.any(axis=1)
    if max_bin == 1.0:
        assert not clipped.any()
    else:
        assert 0 < clipped.sum() < 67
    assert zero.sum() == 11 and not want[zero].any()
    with hesaff_amd.HesaffContext(_params(maxBinValue=max_bin), device=0) as c:
        got = c.sift_mode(patches, DESC_ROOTSIFT, fill=0xEE)
        _, ghist, _ = c.sift_parts(patches)
        assert np.array_equal(_u32(ghist), _u32(hist))
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, "maxBinValue %g: patches %s differ" % (max_bin, bad.tolist())
        for k in range(67):
            one = c.sift_mode(patches[k:k + 1], DESC_ROOTSIFT, fill=0xEE)
            assert np.array_equal(one[0], want[k]), "maxBinValue %g, n = 1: patch %d" % (max_bin, k)
        assert c.descriptor == DESC_SIFT   # the operator neither reads nor changes the context's mode


@pytest.mark.gpu
def test_stage_saturation(ctx, oracle):
    """Bytes of 255: with maxBinValue 1.0 six patches of stage_inputs.saturating() have one, with the default two flat patches do
    (that they do is a condition on the input, asserted on the helper); the kernel's bytes are the helper's."""
    with hesaff_amd.HesaffContext(_params(maxBinValue=1.0), device=0) as c1:
        want, _, _ = RS.describe_many(oracle.OracleHandle(_params(maxBinValue=1.0)), SI.saturating(), 1.0, RS.ROOTSIFT)
        assert [n for n, row in zip(SI.saturating_names(), want) if row.max() == 255] == SAT_AT_1
        got = c1.sift_mode(SI.saturating(), DESC_ROOTSIFT)
        assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0].tolist()
    want, _, _ = RS.describe_many(oracle.OracleHandle(), SI.flat(), 0.2, RS.ROOTSIFT)
    assert [n for n, row in zip(SI.flat_names(), want) if row.max() == 255] == SAT_AT_DEFAULT
    got = ctx.sift_mode(SI.flat(), DESC_ROOTSIFT)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0].tolist()


@pytest.mark.gpu
def test_stage_dead_keypoints_keep_their_rows(ctx, oracle):
    alive = np.array([1, 0, 0, 1, 0, 1, 1], np.int32)
    _, _, want, _ = stage_reference(oracle, 0.2)
    got = ctx.sift_mode(SI.interleaved(67)[:7], DESC_ROOTSIFT, alive=alive, fill=0xAB)
    for k in range(7):
        assert np.array_equal(got[k], want[k] if alive[k] else np.full(128, 0xAB, np.uint8)), k


@pytest.mark.gpu
def test_stage_mode_0_is_the_oracle(ctx, oracle):
    _, want, root, _ = stage_reference(oracle, 0.2)
    got = ctx.sift_mode(SI.interleaved(67), DESC_SIFT)
    assert np.array_equal(got, want), np.nonzero((got != want).any(axis=1))[0].tolist()
    assert (want != root).any()
    with pytest.raises(hesaff_amd.HesaffError):
        ctx.sift_mode(SI.interleaved(67)[:1], 2)


# ---------------------------------------------------------------- end to end

@pytest.mark.gpu
def test_end_to_end_host_entry_points(rctx, oracle):
    """detect_batch and detect_regions on three images of two sizes (they chunk separately; tiny_20x15 has one Hessian keypoint and
    no key) in mode 1: counts, regions and every key field are the reference chain's, desc the helper's; back in mode 0 on the same
    context the keys are the oracle's again."""
    gold = [golden(oracle, n) for n in E2E_IMAGES]
    imgs = [g[0] for g in gold]
    assert len(gold[0][3]) == 221 and gold[1][4] == 1 and len(gold[1][3]) == 0
    regions = rctx.detect_regions(imgs)
    batch = rctx.detect_batch(imgs)
    for name, (_, _, want_r, want_k, n_hess, sift_k), (got_r, got_k), (nh, keys_b) in zip(E2E_IMAGES, gold, regions, batch):
        assert nh == n_hess == len(got_r), name
        _same_records(got_r, want_r, name + ": regions")
        _same_records(got_k, want_k, name + ": keys")
        assert keys_b.tobytes() == got_k.tobytes(), name
        if len(want_k):
            assert (want_k["desc"] != sift_k["desc"]).any(axis=1).all()
            for f in NOT_DESC:
                assert np.array_equal(want_k[f], sift_k[f])
    rctx.set_descriptor("sift")
    try:
        assert rctx.descriptor == DESC_SIFT
        for name, g, (nh, keys_b) in zip(E2E_IMAGES, gold, rctx.detect_batch(imgs)):
            _same_records(keys_b, g[5], name + ": keys back in mode 0")
        with pytest.raises(hesaff_amd.HesaffError):
            rctx.set_descriptor(2)
        with pytest.raises(ValueError):
            rctx.set_descriptor("surf")
        assert rctx.descriptor == DESC_SIFT   # a refused call changes nothing
    finally:
        rctx.set_descriptor(DESC_ROOTSIFT)


@pytest.mark.gpu
def test_end_to_end_device_resident(rctx, oracle):
    import torch
    from tests.test_gpu_parity import _device_keys
    img, _, _, want_k, n_hess, _ = golden(oracle, "band_131x77")
    assert len(want_k) > 20
    t = torch.from_numpy(np.stack([img, img])).cuda()
    torch.cuda.synchronize()
    ch, cd, dkeys, total = rctx.detect_batch_device(t.data_ptr(), 2, img.shape[1], img.shape[0])
    assert ch.tolist() == [n_hess] * 2 and cd.tolist() == [len(want_k)] * 2 and total == 2 * len(want_k)
    got = _device_keys(dkeys, total)
    _same_records(got[:len(want_k)], want_k, "device keys, image 0")
    _same_records(got[len(want_k):], want_k, "device keys, image 1")


@pytest.mark.gpu
@pytest.mark.parametrize("from_", [FROM_POINTS, FROM_SHAPES])
def test_describe_regions(ctx, rctx, oracle, from_):
    """hesaff_describe_regions in mode 1 over the records of a mode-0 detect_regions (themselves the oracle's): the helper's bytes"""
    img, _, want_r, want_k, _, sift_k = golden(oracle, "band_96x96")
    (rec, k0), = ctx.detect_regions([img])
    _same_records(rec, want_r, "mode-0 records")
    _same_records(k0, sift_k, "mode-0 keys")
    rin = rec if from_ == FROM_POINTS else rec[rec["outcome"] >= 1]
    (got_r, got_k), = rctx.describe_regions([img], [rin], from_)
    _same_records(got_r, _renumbered(rin), "regions")
    _same_records(got_k, want_k, "keys")


class _RootHandle:
    """an OracleHandle whose sift() is the helper's RootSIFT over the oracle's histogram"""

    def __init__(self, handle):
        self.handle = handle

    def normalize_affine(self, *a):
        return self.handle.normalize_affine(*a)

    def sift(self, patch):
        return RS.describe(self.handle, patch, 0.2, RS.ROOTSIFT)


class _RootOracle:
    """tests._oracle with that handle, for tests/orientation_ref.py's chain"""

    def __init__(self, oracle):
        self.oracle = oracle

    def __getattr__(self, name):
        return getattr(self.oracle, name)

    def OracleHandle(self, params=None):
        return _RootHandle(self.oracle.OracleHandle(params))


@pytest.mark.gpu
def test_with_dominant_orientation(oracle):
    """both modes on: orientation_ref's chain (describe_one) with the helper in place of handle.sift"""
    img, gray = golden(oracle, "band_96x96")[:2]
    want_r, want_k, n_hess = R.oriented_run(_RootOracle(oracle), gray)
    assert len(want_k) > 20 and (want_k["a12"] != 0).any()
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_orientation(ORI_DOMINANT)
        c.set_descriptor(DESC_ROOTSIFT)
        (got_r, got_k), = c.detect_regions([img])
    assert len(got_r) == n_hess
    _same_records(got_r, want_r, "regions")
    _same_records(got_k, want_k, "keys")


@pytest.mark.gpu
def test_with_limit_and_grid(oracle):
    """limit 50 on a 2 x 2 grid: every kept key's bytes are its bytes in the unlimited mode-1 reference chain"""
    img, _, _, want_k, n_hess, _ = golden(oracle, "band_160x120")
    full = {ident: k.tobytes() for ident, k in zip(_identity(want_k), want_k)}
    assert len(full) == len(want_k)
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_descriptor(DESC_ROOTSIFT)
        c.set_keypoint_limit(50)
        c.set_keypoint_grid(2, 2)
        (nh, kept), = c.detect_batch([img])
    assert 0 < nh <= 50 < n_hess and 10 < len(kept) <= nh
    for ident, k in zip(_identity(kept), kept):
        assert full.get(ident) == k.tobytes(), ident


@pytest.mark.gpu
def test_with_fast_mode(oracle):
    """fast = 2 has no oracle.  Every field but desc is that of the same context's mode-0 run, and every non-zero descriptor
    without a saturated byte has 0.977 <= ||desc / 512|| <= 1: u has unit norm, truncation loses less than 1/512 per element, at
    most sqrt(128) / 512 = 0.0221 in norm."""
    img = golden(oracle, "band_160x120")[0]
    with hesaff_amd.HesaffContext(_params(fast=2), device=0) as c:
        (r0, k0), = c.detect_regions([img])
        c.set_descriptor(DESC_ROOTSIFT)
        (r1, k1), = c.detect_regions([img])
    assert r0.tobytes() == r1.tobytes() and len(k0) == len(k1) > 100
    for f in NOT_DESC:
        assert np.array_equal(_u32(k0[f]) if k0[f].dtype == np.float32 else k0[f], _u32(k1[f]) if k1[f].dtype == np.float32 else k1[f]), f
    d = k1["desc"]
    use = d.any(axis=1) & (d.max(axis=1) < 255)
    assert (d != k0["desc"]).any(axis=1)[use].all()
    assert use.sum() > 100
    norm = np.sqrt(((d[use].astype(np.float64) / 512.0) ** 2).sum(axis=1))
    print("fast = 2, mode 1: %d descriptors, norm %.4f .. %.4f" % (use.sum(), norm.min(), norm.max()))
    assert (norm >= 0.977).all() and (norm <= 1.0).all()


# ---------------------------------------------------------------- files, CLI, C++

@pytest.mark.gpu
def test_process_files_and_cli(oracle, tmp_path):
    """hesaff_process_files in mode 1, text and sidecar: the rows are hesaff_format_sift / hesaff_write_bin of the reference chain's
    keys; `hesaff image --descriptor rootsift` writes the same text."""
    names = ["band_160x120", "band_96x96", "band_131x77"]
    paths = []
    for n in names:
        paths.append(str(tmp_path / (n + ".pgm")))
        shutil.copyfile(os.path.join(GOLD, n + ".pgm"), paths[-1])
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_descriptor("rootsift")
        c.set_output_format(3)
        mr = c.params.mrSize
        st = c.process_files(paths)
    for n, p, s in zip(names, paths, st):
        want_k = golden(oracle, n)[3]
        assert s[0] == 0 and s[3] == len(want_k), (n, s)
        text = hesaff_amd.format_sift(want_k, mr)
        assert open(p + ".hesaff.sift", "rb").read() == text, n
        ref = str(tmp_path / (n + ".ref.bin"))
        hesaff_amd.write_bin(ref, want_k, mr)
        assert open(p + ".hesaff.bin", "rb").read() == open(ref, "rb").read(), n
    p = paths[1]
    os.remove(p + ".hesaff.sift")
    r = subprocess.run([EXE, p, "--descriptor", "rootsift"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(p + ".hesaff.sift", "rb").read() == hesaff_amd.format_sift(golden(oracle, "band_96x96")[3], mr)


@pytest.mark.gpu
def test_cpp_detector_with_descriptor_mode(oracle, tmp_path):
    """tests/native/descriptor_mode_keys.cpp: AffineHessianDetector::setDescriptor(HESAFF_DESC_ROOTSIFT) holds the reference chain's keys."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    _, _, _, want_k, n_hess, _ = golden(oracle, "band_96x96")
    exe = str(tmp_path / "descriptor_mode_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "descriptor_mode_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, "1", os.path.join(GOLD, "band_96x96.pgm")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "N %d %d %d" % (n_hess, len(want_k), len(want_k)), lines[0]
    assert [ln[2:] for ln in lines[1:]] == [k.tobytes().hex() for k in want_k]
