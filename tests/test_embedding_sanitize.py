"""AddressSanitizer + UBSan run of the two readers of Hamming embedding (hesaff_read_embedding, hesaff_read_signatures) on whole,
truncated and corrupt files, in the manner of tests/test_host_sanitize.py: a stand-alone program with its own main
(tests/native/embedding_files_sanitize.cpp) compiled from the product's host sources.  CPU only, nothing is preloaded."""
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = [os.path.join(ROOT, "hesaff_amd", "csrc", "hostio.cpp"), os.path.join(ROOT, "hesaff_amd", "csrc", "jpeg_decode.cpp"),
       os.path.join(ROOT, "tests", "native", "embedding_files_sanitize.cpp")]


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("san") / "embedding_files_sanitize")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", out] + SRC + ["-lz", "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(driver, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, "sanitizer or driver failure (rc %d)\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    return r.stdout


def _embedding_file(k, seed):
    rng = np.random.RandomState(seed)
    P = rng.randint(-127, 128, (64, 128)).astype(np.int8)
    tau = rng.randint(-(1 << 22), 1 << 22, (k, 64)).astype("<i4")
    return b"HESAFFE1" + np.array([64, 128, k, 0], "<u4").tobytes() + P.tobytes() + tau.tobytes()


def _signatures_file(n, seed):
    rng = np.random.RandomState(seed)
    return b"HESAFFS1" + np.array([64, n], "<u4").tobytes() + rng.randint(0, 256, 8 * n).astype(np.uint8).tobytes()


def _mutants(data, rng, n):
    out = []
    for _ in range(n):
        b = bytearray(data)
        kind = rng.randrange(4)
        if kind == 0:                                      # truncated, often inside the head
            b = b[: rng.randrange(0, 40) if rng.random() < 0.5 else rng.randrange(0, len(b))]
        elif kind == 1:                                    # a few flipped bytes, the head favoured
            for _ in range(rng.randrange(1, 6)):
                pos = rng.randrange(min(len(b), 24)) if rng.random() < 0.7 else rng.randrange(len(b))
                b[pos] = rng.randrange(256)
        elif kind == 2:                                    # a header field blown up (bits, dim, k, count)
            pos = 8 + 4 * rng.randrange(4)
            b[pos:pos + 4] = bytes([0xFF, 0xFF, 0xFF, rng.randrange(256)])
        else:                                              # a slice removed or duplicated
            i = rng.randrange(len(b)); j = min(len(b), i + rng.randrange(1, 64))
            b = b[:i] + (b[i:j] * 2 if rng.random() < 0.5 else b"") + b[j:]
        out.append(bytes(b))
    return out


def test_readers_on_whole_truncated_and_corrupt_files(driver, tmp_path):
    rng = random.Random(20)
    whole = [_embedding_file(1, 1), _embedding_file(33, 2), _signatures_file(0, 3), _signatures_file(1, 4), _signatures_file(221, 5)]
    paths = []
    for i, data in enumerate(whole):
        p = str(tmp_path / ("whole_%d.bin" % i))
        open(p, "wb").write(data)
        paths.append(p)
    out = _run(driver, paths)
    assert "embeddings=2 signatures=3 refused=5" in out, out   # each whole file is one format's and is refused by the other reader
    damaged = []
    for i, data in enumerate(whole):
        for j, m in enumerate(_mutants(data, rng, 60)):
            p = str(tmp_path / ("bad_%d_%d.bin" % (i, j)))
            open(p, "wb").write(m)
            damaged.append(p)
    # a head that promises far more than the file holds, and one whose k makes 24 + 8192 + 256 k wrap 32 bits
    for name, data in (("huge_count", b"HESAFFS1" + np.array([64, 0x7fffffff], "<u4").tobytes()),
                       ("huge_k", b"HESAFFE1" + np.array([64, 128, 0x00ffffe0, 0], "<u4").tobytes() + b"\0" * 8192),
                       ("head_only", b"HESAFFE1"), ("empty", b"")):
        p = str(tmp_path / (name + ".bin"))
        open(p, "wb").write(data)
        damaged.append(p)
    out = _run(driver, damaged)
    assert "read embeddings=" in out
    refused = int(out.split("refused=")[1].split()[0])
    assert refused >= len(damaged), out   # every file is refused by at least one of the two readers
