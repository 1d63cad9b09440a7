"""Builds tests/native/schedule_check.cpp - the stand-alone checker of the group pipeline's stream / event order
(hesaff_amd/csrc/group_schedule.h) - with AddressSanitizer + UBSan and runs one of its parts."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_schedule_check(tmp_path, part):
    """part: "upright", "oriented" or "peaks" (schedule_check.cpp says what each holds)."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "schedule_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "schedule_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden"), part], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, "schedule_check %s failed (rc %d)\n%s\n%s" % (part, r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    assert "schedule_check ok" in r.stdout, r.stdout
