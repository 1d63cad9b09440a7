"""CPU suite of the dominant-orientation mode (hesaff_set_orientation): hm_sincosf on a host build against this image's libm, the
oriented stream / event order of group_schedule.h under a stand-alone checker built with AddressSanitizer + UBSan
(the oriented part of tests/native/schedule_check.cpp), and the C ABI (three new symbols, version and struct sizes as before).  No GPU."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests.schedule_native import run_schedule_check

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sincos_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("hm_sincos")
    src = d / "hm.cpp"
    src.write_text('#include "%s/hesaff_amd/csrc/hmath.h"\n'
                   'extern "C" void hm_sincosf_v(int n,const float*t,float*s,float*c){for(int i=0;i<n;i++)hm_sincosf(t[i],s+i,c+i);}\n' % ROOT)
    so = d / "hm.so"
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    f32p = np.ctypeslib.ndpointer(np.float32, flags="C")
    L.hm_sincosf_v.argtypes = [C.c_int, f32p, f32p, f32p]
    return L


def test_hm_sincosf_equals_libm_rounded_once(sincos_host):
    """(float)sin((double)theta) and (float)cos((double)theta) of this image's libm, bit for bit: the 36 bin centres, each
    +- {0, 2^-20, a quarter bin}, +-pi, +-0, and 10^6 uniform random binary32 angles in [-pi, pi].
    Double-rounding boundaries met in these samples: none."""
    f32 = np.float32
    PI = f32(np.pi)
    width = (f32(2.0) * PI) / f32(36.0)
    centres = (np.arange(36, dtype=np.float32) + f32(0.5)) * width - PI
    fixed = [centres + d for d in (f32(0), f32(2.0 ** -20), -f32(2.0 ** -20), f32(0.25) * width, -f32(0.25) * width)]
    rng = np.random.default_rng(2024)
    theta = np.concatenate(fixed + [np.array([PI, -PI, 0.0, -0.0], np.float32), rng.uniform(-np.pi, np.pi, 1000000).astype(np.float32)])
    theta = np.clip(theta, -PI, PI).astype(np.float32)
    n = len(theta)
    s = np.zeros(n, np.float32); c = np.zeros(n, np.float32)
    sincos_host.hm_sincosf_v(n, theta, s, c)
    # math.sin / math.cos are libm's double functions; the conversion to float32 rounds once
    t64 = theta.astype(np.float64).tolist()
    rs = np.array([math.sin(t) for t in t64], np.float64).astype(np.float32)
    rc = np.array([math.cos(t) for t in t64], np.float64).astype(np.float32)
    bad = np.nonzero((s.view(np.uint32) != rs.view(np.uint32)) | (c.view(np.uint32) != rc.view(np.uint32)))[0]
    assert len(bad) == 0, [(hex(int(theta[i:i + 1].view(np.uint32)[0])), float(s[i]), float(rs[i]), float(c[i]), float(rc[i])) for i in bad[:8]]


def test_oriented_schedule(tmp_path):
    run_schedule_check(tmp_path, "oriented")


def test_orientation_abi():
    """Symbols only: the three new entry points exist, the ABI version and every struct size are what they were."""
    L = hesaff_amd.load_library()
    for name in ("hesaff_set_orientation", "hesaff_get_orientation", "hesaff_stage_orientation"):
        assert hasattr(L, name), name
        assert name in _binding.ABI_SYMBOLS
    hdr = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    assert "#define HESAFF_ORI_UP 0" in hdr and "#define HESAFF_ORI_DOMINANT 1" in hdr and "#define HESAFF_ABI_VERSION 8" in hdr
    assert (hesaff_amd.ORI_UP, hesaff_amd.ORI_DOMINANT) == (0, 1)
    L.hesaff_abi_version.restype = C.c_int
    assert L.hesaff_abi_version() == 8
    for fn, size in (("hesaff_sizeof_params", C.sizeof(_binding.Params)), ("hesaff_sizeof_timings", C.sizeof(_binding.Timings)),
                     ("hesaff_sizeof_region", 64)):
        f = getattr(L, fn)
        f.restype = C.c_size_t
        assert f() == size, fn
    assert C.sizeof(_binding.Params) == 44 and C.sizeof(_binding.Timings) == 80 and _binding.KEYPOINT_DTYPE.itemsize == 164
    # argument errors need no device
    L.hesaff_set_orientation.restype = C.c_int
    L.hesaff_get_orientation.restype = C.c_int
    assert L.hesaff_set_orientation(None, 1) == -2 and L.hesaff_get_orientation(None, None) == -2
