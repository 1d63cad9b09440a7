"""The group pipeline's stream / event order (hesaff_amd/csrc/group_schedule.h) on the CPU: the template pipeline.hip runs, over a
recording device, checked by a stand-alone program under AddressSanitizer + UBSan (tests/native/schedule_check.cpp) - the hazards the
order exists for at every group count 0 .. 10 under every option, that each wait and record is needed, and equality with the
sequences of the code the header replaced (tests/golden/group_schedule_parent.txt)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_group_schedule(tmp_path):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "schedule_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "schedule_check.cpp")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe, os.path.join(ROOT, "tests", "golden", "group_schedule_parent.txt")], capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, "schedule_check failed (rc %d)\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    assert "schedule_check ok" in r.stdout, r.stdout
