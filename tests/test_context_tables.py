"""Context setup's host arithmetic (hesaff_amd/csrc/context_tables.h) and the order-map epochs (OrderMapEpochs, batch_plan.h) on the
CPU: the masks, k_sift_grad's per-pixel offsets, the gradient-pair layout, the pyramid and patch tap tables, DConsts - indices and
offsets the kernels follow without a bounds check - and when the order-key map is filled, checked by a stand-alone program under
AddressSanitizer + UBSan (tests/native/tables_check.cpp)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_context_tables_arithmetic(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "tables_check")
    # -ffp-contract=off as the library's own build: the tables' bytes are compared with those of the code they were moved from
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "tables_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, "tables_check failed (rc %d)\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    assert "tables_check ok" in r.stdout, r.stdout
