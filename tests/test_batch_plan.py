"""The batch plan's host arithmetic (hesaff_amd/csrc/batch_plan.h) on the CPU: octave geometry, capacities, the layouts of the counter
and starts blocks, image groups, the launch shape of the large-window row kernel and the band heights - the integers that decide what
the kernels may touch, checked by a stand-alone program under AddressSanitizer + UBSan (tests/native/plan_check.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_batch_plan_arithmetic(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, "plan_check failed (rc %d)\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    assert "plan_check ok" in r.stdout, r.stdout
