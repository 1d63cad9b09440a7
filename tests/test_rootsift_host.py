"""CPU suite of the descriptor modes (hesaff_set_descriptor): the yardstick tests/rootsift_ref.py is held to the oracle in SIFT mode,
the constructed inputs of tests/test_rootsift.py are shown to be what that suite says they are, and the interface (symbols,
constants, argument errors, the CLI's refusal) is checked without a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import rootsift_ref as RS
from tests import stage_inputs as SI

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
BANDS = ("band_160x120", "band_96x96", "band_131x77")
SAT_AT_1 = ["edge:45:6", "edge:135:6", "edge:225:6", "edge:315:6", "spike:r19:x", "spike:r19:y"]
SAT_AT_DEFAULT = ["outside:spike:20:x", "outside:spike:20:y"]


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


# ---------------------------------------------------------------- the yardstick

def test_sift_mode_of_the_helper_is_the_oracle_on_constructed_patches(oracle):
    """normalize / clip / normalize / quantise restated in numpy float32 reproduces the oracle's bytes on all 135 patches of the
    constructed families, zero histograms (NaN all the way, bytes 0) included."""
    patches = np.concatenate([SI.flat(), SI.saturating(), SI.threshold(), SI.ordinary()[:40]])
    assert len(patches) == 135
    handle = oracle.OracleHandle()
    zero = clipped = 0
    for k, p in enumerate(patches):
        _, hist, desc = handle.sift_parts(p)
        assert np.array_equal(RS.to_bytes(hist, 0.2, RS.SIFT), desc), k
        zero += not hist.any()
        clipped += RS.normalized(hist, 0.2)[1]
    assert zero > 10 and clipped > 40 and clipped + zero < 135


def test_sift_mode_of_the_chain_is_the_oracle_on_the_golden_images(oracle):
    """rootsift_ref.chain in SIFT mode - every patch recomputed with normalizeAffine from the rectified matrix the key stores - gives
    the oracle's own keys on the three band_* golden images, 366 in all, and its regions' outcomes count them."""
    total = 0
    for name in BANDS:
        gray = oracle.gray_from_u8(hesaff_amd.read_pnm(os.path.join(GOLD, name + ".pgm")))
        rec, keys, n = RS.chain(oracle, gray, RS.SIFT)
        run = oracle.OracleRun(gray)
        g, t, d = run.keys()
        assert n == run.n_hessian and len(keys) == run.n_keys == int((rec["outcome"] == 2).sum())
        got = np.stack([keys[f] for f in ("x", "y", "s", "a11", "a12", "a21", "a22", "response")], axis=1)
        assert np.array_equal(got.view(np.uint32), g.view(np.uint32)) and np.array_equal(keys["type"], t)
        assert np.array_equal(keys["desc"], d), name
        total += len(keys)
    assert total == 366


def test_rootsift_of_the_helper_is_a_unit_vector(oracle):
    """u = sqrt(v / sum v) has unit L2 norm to rounding; its bytes lose less than 1 each to truncation."""
    handle = oracle.OracleHandle()
    for p in SI.ordinary()[:10]:
        hist = handle.sift_parts(p)[1]
        u = RS.unit_vector(hist, 0.2, RS.ROOTSIFT).astype(np.float64)
        assert abs(np.sqrt((u * u).sum()) - 1.0) < 1e-5
        b = RS.to_bytes(hist, 0.2, RS.ROOTSIFT).astype(np.float64)
        assert ((512.0 * u - b >= 0) & (512.0 * u - b < 1)).all()


# ---------------------------------------------------------------- the constructed inputs of the GPU suite

def test_interleaved_67_is_what_the_gpu_suite_says(oracle):
    """stage_inputs.interleaved(67): 16 wavefronts of four keypoints and a tail of three; at maxBinValue 0.2, 52 patches are clipped,
    13 of the 17 groups hold clipped and unclipped keypoints side by side, 11 patches have a zero histogram; at 1.0 none is clipped."""
    patches = SI.interleaved(67)
    handle = oracle.OracleHandle()
    _, hist, clipped = RS.describe_many(handle, patches, 0.2, RS.ROOTSIFT)
    zero = ~hist.any(axis=1)
    assert int(clipped.sum()) == 52 and int(zero.sum()) == 11
    mixed = sum(0 < int(clipped[g:g + 4].sum()) < len(clipped[g:g + 4]) for g in range(0, 67, 4))
    assert mixed == 13
    for mode in (RS.SIFT, RS.ROOTSIFT):
        d = np.stack([RS.to_bytes(h, 0.2, mode) for h in hist])
        assert not d[zero].any() and d[~zero].any(axis=1).all()
    assert not RS.describe_many(handle, patches, 1.0, RS.ROOTSIFT)[2].any()
    assert 0 < int(RS.describe_many(handle, patches, 0.5, RS.ROOTSIFT)[2].sum()) < 52


def test_saturating_patches_reach_255(oracle):
    """which patches have a RootSIFT byte of 255: six of stage_inputs.saturating() at maxBinValue 1.0, two flat ones at the default"""
    h1 = oracle.OracleHandle(_params(maxBinValue=1.0))
    d, _, _ = RS.describe_many(h1, SI.saturating(), 1.0, RS.ROOTSIFT)
    assert [n for n, row in zip(SI.saturating_names(), d) if row.max() == 255] == SAT_AT_1
    h0 = oracle.OracleHandle()
    d, _, _ = RS.describe_many(h0, SI.flat(), 0.2, RS.ROOTSIFT)
    assert [n for n, row in zip(SI.flat_names(), d) if row.max() == 255] == SAT_AT_DEFAULT


# ---------------------------------------------------------------- the interface

def test_descriptor_abi():
    """Symbols only: the three new entry points exist, the header carries the constants, the ABI version and every struct size are
    what they were; the argument errors on a NULL context need no device."""
    L = hesaff_amd.load_library()
    for name in ("hesaff_set_descriptor", "hesaff_get_descriptor", "hesaff_stage_sift_mode"):
        assert hasattr(L, name), name
        assert name in _binding.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    assert "#define HESAFF_DESC_SIFT 0" in hdr and "#define HESAFF_DESC_ROOTSIFT 1" in hdr and "#define HESAFF_ABI_VERSION 8" in hdr
    assert (hesaff_amd.DESC_SIFT, hesaff_amd.DESC_ROOTSIFT) == (0, 1)
    assert callable(hesaff_amd.HesaffContext.set_descriptor)
    L.hesaff_abi_version.restype = C.c_int
    assert L.hesaff_abi_version() == 8
    for fn, size in (("hesaff_sizeof_params", C.sizeof(_binding.Params)), ("hesaff_sizeof_timings", C.sizeof(_binding.Timings)),
                     ("hesaff_sizeof_region", 64)):
        f = getattr(L, fn)
        f.restype = C.c_size_t
        assert f() == size, fn
    assert C.sizeof(_binding.Params) == 44 and C.sizeof(_binding.Timings) == 80 and _binding.KEYPOINT_DTYPE.itemsize == 164
    L.hesaff_set_descriptor.restype = C.c_int
    L.hesaff_get_descriptor.restype = C.c_int
    L.hesaff_stage_sift_mode.restype = C.c_int
    mode = C.c_int(7)
    assert L.hesaff_set_descriptor(None, 0) == -2 and L.hesaff_set_descriptor(None, 1) == -2 and L.hesaff_set_descriptor(None, 2) == -2
    assert L.hesaff_get_descriptor(None, None) == -2 and L.hesaff_get_descriptor(None, C.byref(mode)) == -2 and mode.value == 7
    p = np.zeros((1, 41 * 41), np.float32); d = np.zeros((1, 128), np.uint8)
    assert L.hesaff_stage_sift_mode(None, 1, p, None, 1, d) == -2


def test_descriptor_interface_compiles():
    """tests/native/descriptor_mode_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "descriptor_mode_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_refuses_an_unknown_descriptor_before_any_device(tmp_path):
    """--descriptor bogus: the usage text and exit status 1, in the batch form and behind a single image; nothing is written"""
    img = str(tmp_path / "band.pgm")
    with open(os.path.join(GOLD, "band_96x96.pgm"), "rb") as f, open(img, "wb") as g:
        g.write(f.read())
    lst = tmp_path / "list.txt"
    lst.write_text(img + "\n")
    for args in (["--batch", str(lst), "--descriptor", "bogus"], ["--batch", str(lst), "--descriptor"], [img, "--descriptor", "bogus"],
                 [img, "--descriptor"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 1, (args, r.stdout, r.stderr)
        assert r.stderr.startswith("hesaff: usage: hesaff ") and "[--descriptor sift|rootsift]" in r.stderr, r.stderr
        assert r.stdout == ""
        assert not os.path.exists(img + ".hesaff.sift")
