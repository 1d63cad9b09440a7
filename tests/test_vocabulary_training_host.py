"""CPU suite of vocabulary training (hesaff_train_vocabulary, include/hesaff_amd.h): the definition in numpy
(tests/vocabulary_training_ref.py) has the properties the header states, the host arithmetic of hesaff_amd/csrc/train_plan.h holds
the same numbers (a stand-alone program under AddressSanitizer + UBSan), and the entry points and the CLI refuse what they must
without a device.  Nothing here needs a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import vocabulary_ref as V
from tests import vocabulary_training_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_train_vocabulary", "hesaff_train_vocabulary_device", "hesaff_stage_accumulate_words", "hesaff_get_training_ms")


@pytest.mark.parametrize("name", V.FAMILIES)
def test_distortion_never_increases(name):
    """the four families at n = 257, K in {1, 2, 33, 65}, T = 8: distortion[t] <= distortion[t - 1], one entry per iteration run, and an
    early stop only at a fixed point"""
    desc = V.family(name, 257, seed=41)
    for K in (1, 2, 33, 65):
        words, dist, empty = T.train(desc, K, 8)
        assert 1 <= len(dist) == len(empty) <= 8 and words.shape == (K, 128) and words.dtype == np.uint8
        assert (np.diff(dist) <= 0).all(), (name, K, dist.tolist())
        assert (empty >= 0).all() and (empty < K).all()
        if len(dist) < 8:   # stopped: one more iteration changes nothing
            again, d2, _ = T.train(desc, K, 1, init=words)
            assert np.array_equal(again, words) and d2[0] <= dist[-1]
    # K = 1: the word is the rounded mean of all keys after one iteration, and the second iteration finds it unchanged
    words, dist, empty = T.train(desc, 1, 8)
    s = desc.astype(np.int64).sum(axis=0)
    assert np.array_equal(words[0], (2 * s + 257) // (2 * 257)) and len(dist) == 2 and empty.tolist() == [0, 0]


def test_rounding_rule():
    """{0, 1} -> 1 (a half rounds up), {0, 0, 1} -> 0, all 255 stays 255; an empty word keeps its row"""
    col = lambda *v: np.repeat(np.array(v, np.uint8)[:, None], 128, axis=1)
    one = lambda desc: T.train(desc, 1, 1)[0][0].tolist()
    assert one(col(0, 1)) == [1] * 128
    assert one(col(0, 0, 1)) == [0] * 128
    assert one(col(1, 1, 0)) == [1] * 128
    assert one(np.full((4099, 128), 255, np.uint8)) == [255] * 128
    init = np.stack([np.full(128, 10, np.uint8), np.full(128, 200, np.uint8)])
    words, dist, empty = T.train(col(0, 1), 2, 3, init=init)
    assert words[1].tolist() == [200] * 128 and words[0].tolist() == [1] * 128 and empty.tolist() == [1, 1]
    assert dist.tolist() == [128 * (100 + 81), 128 * 1]


def test_clustered_set_reaches_a_fixed_point():
    """what the GPU suite compares against: 8 iterations, 2 words empty, non-increasing"""
    words, dist, empty = T.train(T.clustered(), 33, 10)
    assert len(dist) == 8 and empty[-1] == 2 and (np.diff(dist) <= 0).all()


def test_train_plan_arithmetic(tmp_path):
    """tests/native/train_plan_check.cpp: the 2^24 bound on both sides, the sampling index at n = K and n = 2^24, the update rule against
    the minimiser of the squared error, the working arrays disjoint and aligned"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "train_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "train_plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "train_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_sampling_rule_of_the_reference_is_the_headers():
    """row r = desc[r * n // K]: at n = K the keys themselves, at n = 257, K = 33 the indices the native check pins"""
    desc = V.family("uniform", 257, seed=3)
    assert np.array_equal(T.sample(desc, 257), desc)
    assert np.array_equal(T.sample(desc, 33)[32], desc[249]) and np.array_equal(T.sample(desc, 2)[1], desc[128])


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s), s
    assert L.hesaff_abi_version() == 8
    for m in ("train_vocabulary", "train_vocabulary_device", "accumulate_words"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))


def test_entry_points_refuse_a_null_context():
    L = hesaff_amd.load_library()
    desc = V.family("uniform", 4, seed=1)
    words = np.zeros(4, np.int32)
    out = np.full((2, 128), 7, np.uint8)
    sums = np.full((2, 128), 7, np.uint32); counts = np.full(2, 7, np.uint32)
    dist = np.full(3, 7, np.int64); empty = np.full(3, 7, np.int32); done = C.c_int(7)
    a, b, u = C.c_float(7), C.c_float(7), C.c_float(7)
    assert L.hesaff_train_vocabulary(None, 4, desc.ctypes.data, 2, None, 3, out.ctypes.data, dist.ctypes.data, empty.ctypes.data, C.byref(done)) == -2
    assert L.hesaff_train_vocabulary_device(None, 4, desc.ctypes.data, 128, 0, 2, None, 3, out.ctypes.data, dist.ctypes.data, empty.ctypes.data,
                                            C.byref(done)) == -2
    assert L.hesaff_stage_accumulate_words(None, 4, desc.ctypes.data, words.ctypes.data, 2, sums.ctypes.data, counts.ctypes.data) == -2
    assert L.hesaff_get_training_ms(None, C.byref(a), C.byref(b), C.byref(u)) == -2
    assert (out == 7).all() and (sums == 7).all() and (counts == 7).all() and (dist == 7).all() and (empty == 7).all() and done.value == 7
    assert (a.value, b.value, u.value) == (7.0, 7.0, 7.0)


def test_cli_refuses_training_without_words_before_any_image(tmp_path):
    """--train-vocabulary without --words (and --words without it, a K of 0, a K beyond 2^20, training combined with --vocabulary): the
    usage text, exit status 1, nothing on stdout, no vocabulary file - and the list is never opened: it names a file that does not exist"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    lst = tmp_path / "list.txt"
    lst.write_text(str(tmp_path / "no_such_image.pgm") + "\n")
    out = str(tmp_path / "vocab.bin")
    some = str(tmp_path / "some.bin")
    hesaff_amd.write_vocabulary(some, V.family("uniform", 3, seed=1))
    cases = (["--train-vocabulary", out], ["--train-vocabulary", out, "--iterations", "3"], ["--words", "8"], ["--iterations", "3"],
             ["--train-vocabulary", out, "--words", "0"], ["--train-vocabulary", out, "--words", "1048577"], ["--train-vocabulary", out, "--words", "8x"],
             ["--train-vocabulary", out, "--words", "8", "--iterations", "0"], ["--train-vocabulary", out, "--words", "8", "--vocabulary", some],
             ["--train-vocabulary", out, "--words"], ["--train-vocabulary"])
    for extra in cases:
        for lpath in (str(lst), str(tmp_path / "no_such_list.txt")):
            r = subprocess.run([EXE, "--batch", lpath] + extra, capture_output=True, text=True)
            assert r.returncode == 1 and r.stdout == "", (extra, r.stdout, r.stderr)
            assert r.stderr.startswith("hesaff: usage: hesaff --batch <list file>"), (extra, r.stderr)
            assert "[--train-vocabulary <vocabulary file> --words K [--iterations T]]" in r.stderr
            assert r.stderr.rstrip().endswith("[--orientation up|dominant] [--grid RxC]")
    assert not os.path.exists(out)


def test_training_interface_compiles():
    """tests/native/train_vocabulary_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "train_vocabulary_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
