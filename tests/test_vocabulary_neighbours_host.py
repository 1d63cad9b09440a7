"""CPU suite of vocabulary neighbours (hesaff_set_vocabulary_neighbours, include/hesaff_amd.h): the definition in numpy
(tests/neighbours_ref.py) against a plain double loop; the symbols, the binding and the C++ interface; hesaff_amd.expand_rows on a
hand-written case; the entry points and the CLI refuse what they must without a device.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import neighbours_ref as N
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_set_vocabulary_neighbours", "hesaff_get_vocabulary_neighbours", "hesaff_get_neighbours", "hesaff_get_neighbours_device",
               "hesaff_assign_neighbours_device", "hesaff_stage_assign_neighbours")
BATCH_USAGE = "hesaff: usage: hesaff --batch <list file>"
IMAGE_USAGE = "hesaff: usage: hesaff <image>"


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    text = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    assert "And for vocabulary neighbours (" in text and "): symbols only, version 8." in text
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s) and ("int %s(" % s) in header, s
    assert L.hesaff_abi_version() == 8 and "#define HESAFF_ABI_VERSION 8" in header
    for m in ("set_vocabulary_neighbours", "vocabulary_neighbours", "neighbours", "assign_neighbours", "assign_neighbours_device", "neighbours_device"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))
    assert callable(hesaff_amd.expand_rows)


def test_neighbours_interface_compiles():
    """tests/native/vocabulary_neighbours_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "vocabulary_neighbours_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    hpp = open(os.path.join(ROOT, "hesaff_amd", "csrc", "hesaff.hpp")).read()
    assert "setVocabularyNeighbours" in hpp and "vocabularyNeighbours()" in hpp


def test_the_reference_against_a_double_loop_with_ties():
    """nine rows of bits with two duplicated rows and a key that is a row: ties inside the list and at its cut, K < R"""
    rng = np.random.RandomState(4)
    vocab = rng.randint(0, 2, (9, 128)).astype(np.uint8)
    vocab[4] = vocab[1]
    vocab[7] = vocab[1]
    desc = rng.randint(0, 2, (6, 128)).astype(np.uint8)
    desc[0] = vocab[1]
    desc[1] = 0
    vocab[2] = 0; vocab[2, :3] = 1
    vocab[8] = 0; vocab[8, 5:8] = 1
    for R in (1, 2, 3, 8):
        for K in (1, 2, 9):
            got = N.neighbours(desc, vocab[:K], R)
            assert got.dtype == np.int32 and got.shape == (6, R, 2)
            assert np.array_equal(got, N.neighbours_loops(desc, vocab[:K], R)), (R, K)
    full = N.neighbours(desc, vocab, 8)
    assert full[0, :3].tolist() == [[1, 0], [4, 0], [7, 0]]                     # equal rows in ascending order
    assert full[1, :2].tolist() == [[2, 3], [8, 3]]                             # equal distances: the lower row first
    assert N.neighbours(desc, vocab, 1)[1].tolist() == [[2, 3]]                  # ... and alone where the list is cut between them
    assert N.neighbours(desc, vocab[:2], 3)[:, 2].tolist() == [[-1, 2 ** 31 - 1]] * 6
    assert np.array_equal(N.neighbours(desc, vocab, 1)[:, 0], V.assign(desc, vocab))
    assert np.array_equal(N.neighbours(desc, vocab, 8)[:, :3], N.neighbours(desc, vocab, 3))
    assert N.neighbours(desc[:0], vocab, 3).shape == (0, 3, 2)


def test_expand_rows_on_a_hand_written_case():
    rows = np.zeros(3, hesaff_amd.WORDS_ROW_DTYPE)
    rows["x"] = [1.5, 2.5, 3.5]
    rows["c"] = [0.25, 0.5, 0.75]
    rows["word"] = [99, 99, 99]                                                  # (not read)
    nb = np.array([[[7, 0], [3, 10], [5, 11]],
                   [[2, 4], [-1, 2 ** 31 - 1], [-1, 2 ** 31 - 1]],               # absent ranks give no row
                   [[0, 1], [9, 1], [-1, 2 ** 31 - 1]]], np.int32)
    out = hesaff_amd.expand_rows(rows, nb)
    assert out.dtype == hesaff_amd.WORDS_ROW_DTYPE
    assert out["word"].tolist() == [7, 3, 5, 2, 0, 9]
    assert out["x"].tolist() == [1.5, 1.5, 1.5, 2.5, 3.5, 3.5] and out["c"].tolist() == [0.25, 0.25, 0.25, 0.5, 0.75, 0.75]
    assert rows["word"].tolist() == [99, 99, 99]
    sigs = np.array([[10, 11, 12], [20, 21, 22], [30, 31, 32]], np.uint64)
    out2, s2 = hesaff_amd.expand_rows(rows, nb, sigs)
    assert out2.tobytes() == out.tobytes() and s2.dtype == np.uint64 and s2.tolist() == [10, 11, 12, 20, 30, 31]
    one = hesaff_amd.expand_rows(rows, nb[:, :1])
    assert one["word"].tolist() == [7, 2, 0] and one["x"].tolist() == [1.5, 2.5, 3.5]
    assert len(hesaff_amd.expand_rows(rows[:0], nb[:0])) == 0
    for bad in (lambda: hesaff_amd.expand_rows(rows, nb[:2]), lambda: hesaff_amd.expand_rows(rows, nb[:, :, 0]),
                lambda: hesaff_amd.expand_rows(rows, nb, sigs[:, :2]), lambda: hesaff_amd.expand_rows(np.zeros(3), nb)):
        with pytest.raises(ValueError):
            bad()


def test_entry_points_refuse_without_a_device():
    L = hesaff_amd.load_library()
    r = C.c_int(7); n = C.c_int(7); p = C.c_void_p(7); tot = C.c_int64(7)
    for bad in (None,):
        assert L.hesaff_set_vocabulary_neighbours(bad, 2) == -2 and L.hesaff_set_vocabulary_neighbours(bad, 0) == -2
        assert L.hesaff_set_vocabulary_neighbours(bad, 9) == -2
        assert L.hesaff_get_vocabulary_neighbours(bad, C.byref(r)) == -2 and r.value == 7
        assert L.hesaff_get_neighbours(bad, 0, C.byref(p), C.byref(n), C.byref(r)) == -2
        assert L.hesaff_get_neighbours_device(bad, C.byref(p), C.byref(tot), C.byref(r)) == -2
    assert (p.value, n.value, r.value, tot.value) == (7, 7, 7, 7)
    desc = V.family("uniform", 2, seed=1)
    out = np.full((2, 8, 2), 7, np.int32)
    assert L.hesaff_stage_assign_neighbours(None, 2, desc.ctypes.data, out.ctypes.data) == -2
    assert L.hesaff_assign_neighbours_device(None, 2, desc.ctypes.data, 128, 0, out.ctypes.data) == -2
    assert (out == 7).all()


def test_cli_refuses_bad_neighbours_before_any_file(tmp_path):
    """--neighbours without a vocabulary, outside 1..8, without its argument, or beside a training mode: the mode's usage line, exit
    status 1, no file; beside --cells with a count above 1: the refusal that says the two do not combine"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    lst = str(tmp_path / "no_such_list.txt")
    out = str(tmp_path / "trained.bin")
    some = str(tmp_path / "some.bin")
    cells = some + ".cells"
    hesaff_amd.write_vocabulary(some, V.family("uniform", 4, seed=1))
    hesaff_amd.write_vocabulary_cells(cells, V.family("uniform", 2, seed=1), [0, 1, 4])
    before = sorted(os.listdir(tmp_path))
    cases = (["--neighbours", "2"], ["--vocabulary", some, "--neighbours", "0"], ["--vocabulary", some, "--neighbours", "9"],
             ["--vocabulary", some, "--neighbours", "2x"], ["--vocabulary", some, "--neighbours", "-1"], ["--vocabulary", some, "--neighbours"],
             ["--train-vocabulary", out, "--words", "8", "--neighbours", "2"],
             ["--vocabulary", some, "--train-embedding", out, "--neighbours", "2"])
    for extra in cases:
        r = subprocess.run([EXE, "--batch", lst] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "", (extra, r.stdout, r.stderr)
        assert r.stderr.startswith(BATCH_USAGE) and "[--neighbours 1..8]" in r.stderr and "[--probes 1..8]" in r.stderr, (extra, r.stderr)
    r = subprocess.run([EXE, "--batch", lst, "--vocabulary", some, "--cells", cells, "--neighbours", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("hesaff: --neighbours above 1 and --cells do not combine"), r.stderr
    # a good count - and 1 beside a layer - gets as far as the list, which does not exist
    for extra in (["--vocabulary", some, "--neighbours", "8"], ["--vocabulary", some, "--cells", cells, "--neighbours", "1"]):
        r = subprocess.run([EXE, "--batch", lst] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("hesaff: cannot read list"), (extra, r.stderr)
    img = str(tmp_path / "no_such_image.pgm")
    for extra in (["--neighbours", "2"], ["--vocabulary", some, "--neighbours", "0"], ["--vocabulary", some, "--neighbours", "9"],
                  ["--vocabulary", some, "--neighbours", "22"], ["--vocabulary", some, "--neighbours"]):
        r = subprocess.run([EXE, img] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith(IMAGE_USAGE) and "[--neighbours 1..8]" in r.stderr, (extra, r.stderr)
    r = subprocess.run([EXE, img, "--vocabulary", some, "--cells", cells, "--neighbours", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("hesaff: --neighbours above 1 and --cells do not combine"), r.stderr
    r = subprocess.run([EXE, img, "--vocabulary", some, "--neighbours", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("hesaff: cannot read '%s'" % img), r.stderr
    assert sorted(os.listdir(tmp_path)) == before
    # the bare usage text does not change
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("\nUsage: hesaff image_name.ppm\n") and "neighbours" not in r.stdout
