"""CPU suite of the orientation count (hesaff_set_orientation_count: secondary orientation peaks, up to four keys per region): the
peak rule of hesaff_amd/csrc/orient_peaks.h on constructed histograms and the peaks stream / event order of group_schedule.h, each under a
stand-alone checker built with AddressSanitizer + UBSan (tests/native/orient_peaks_check.cpp, the peaks part of schedule_check.cpp), and the C ABI
(three new symbols, their argument refusals, version and struct sizes as before).  No GPU."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests.schedule_native import run_schedule_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _native(tmp_path, name, extra=()):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / name)
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", *extra,
           "-o", exe, os.path.join(ROOT, "tests", "native", name + ".cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, "%s failed (rc %d)\n%s\n%s" % (name, r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    assert name + " ok" in r.stdout, r.stdout


def test_peak_rule_on_constructed_histograms(tmp_path):
    """hs_ori_peaks / hs_ori_theta, the text k_orientation_peaks runs: all zero, one bin, a plateau, equal candidates, the 80 % line
    at, below and above, the wrap at bins 0 and 35, six peaks with K = 4, K = 1, 2, 3, NaN bins, the angle around any bin."""
    _native(tmp_path, "orient_peaks_check", ["-ffp-contract=off"])


def test_peaks_schedule(tmp_path):
    """run_group_schedule with an orientation count over a recording device: the hazards of the (group, rank) units at 0 .. 7 groups
    (HS_NSLOT and HS_NSLOT + 2 among them) for K = 2, 3, 4 under every ScheduleOptions form; every wait and record is needed; the
    sequences of the peaks form the header had (tests/golden/group_schedule_oriented_parent.txt)."""
    run_schedule_check(tmp_path, "peaks")


def test_orientation_count_abi():
    """Symbols only: the three new entry points exist, the ABI version and every struct size are what they were; the argument
    refusals that need no device."""
    L = hesaff_amd.load_library()
    for name in ("hesaff_set_orientation_count", "hesaff_get_orientation_count", "hesaff_stage_orientation_peaks"):
        assert hasattr(L, name), name
        assert name in _binding.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    assert "#define HESAFF_ABI_VERSION 8" in hdr
    L.hesaff_abi_version.restype = C.c_int
    assert L.hesaff_abi_version() == 8
    for fn, size in (("hesaff_sizeof_params", C.sizeof(_binding.Params)), ("hesaff_sizeof_timings", C.sizeof(_binding.Timings)),
                     ("hesaff_sizeof_region", 64)):
        f = getattr(L, fn)
        f.restype = C.c_size_t
        assert f() == size, fn
    assert C.sizeof(_binding.Params) == 44 and C.sizeof(_binding.Timings) == 80 and _binding.KEYPOINT_DTYPE.itemsize == 164
    assert _binding.REGION_DTYPE.itemsize == 64 and "reserved" in _binding.REGION_DTYPE.names
    for fn in (L.hesaff_set_orientation_count, L.hesaff_get_orientation_count, L.hesaff_stage_orientation_peaks):
        fn.restype = C.c_int
    k = C.c_int(7)
    for count in (0, 1, 2, 4, 5, -1):
        assert L.hesaff_set_orientation_count(None, count) == -2
    assert L.hesaff_get_orientation_count(None, C.byref(k)) == -2 and k.value == 7
    assert L.hesaff_get_orientation_count(None, None) == -2
    assert L.hesaff_set_orientation(None, 2) == -2   # (still only 0 and 1: the count is its own setter)


def test_cli_usage_names_the_option():
    exe = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
    if not os.path.exists(exe):
        pytest.skip("CLI not built")
    r = subprocess.run([exe, "--batch", "/nonexistent.list", "--orientations", "5"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 1 and "--orientations 1..4" in r.stderr, r.stderr
