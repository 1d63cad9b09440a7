"""CPU suite of vocabulary probes (hesaff_set_vocabulary_probes, include/hesaff_amd.h): the definition in numpy
(tests/vocabulary_probes_ref.py) has the properties the header states and its two fixed ends - one probe is the cells definition, as
many probes as cells the flat one - on the inputs the GPU suite compares against; the host arithmetic of hesaff_amd/csrc/cells_plan.h
holds the numbers (a stand-alone program under AddressSanitizer + UBSan); the entry points and the CLI refuse what they must without a
device.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import vocabulary_cells_ref as R
from tests import vocabulary_probes_ref as P
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_set_vocabulary_probes", "hesaff_get_vocabulary_probes", "hesaff_stage_probe_cells")
FIRST = [0, 31, 70, 71, 200, 257]


def inputs(family):
    """K = 257 in five cells whose borders lie inside tiles: the inputs of the cells suite"""
    return V.family(family, 257, seed=303), V.family(family, 257, seed=301), V.family(family, 5, seed=302)


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    text = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    assert "And for vocabulary probes (" in text and "): symbols only, version 8." in text
    header = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s) and ("int %s(" % s) in header, s
    assert L.hesaff_abi_version() == 8 and "#define HESAFF_ABI_VERSION 8" in header
    for m in ("set_vocabulary_probes", "vocabulary_probes", "probe_cells"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))
    plan = open(os.path.join(ROOT, "hesaff_amd", "csrc", "cells_plan.h")).read()
    assert "HS_CELLS_MAX_PROBES = 8" in plan


def test_probes_interface_compiles():
    """tests/native/vocabulary_probes_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "vocabulary_probes_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert "setVocabularyProbes" in open(os.path.join(ROOT, "hesaff_amd", "csrc", "hesaff.hpp")).read()


def test_probes_plan_arithmetic(tmp_path):
    """tests/native/probes_plan_check.cpp: the keys of a slice for P = 1..8, the item bound over distributions of n P entries, the
    entry -> key map, the scratch layout, which at P = 1 is cell_scratch's byte for byte"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "probes_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "probes_plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "probes_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


@pytest.mark.parametrize("family", V.FAMILIES)
def test_the_two_fixed_ends_and_what_lies_between(family):
    """P = 1 is the cells definition, P = 5 = C and P = 8 > C the flat one, dist2 never increases with P, and for P = 2..5 every probe
    rank wins for at least 30 keys - so a device that ignored a rank, or merged by rank, could not pass the GPU comparisons"""
    desc, vocab, coarse = inputs(family)
    flat = V.assign(desc, vocab)
    by_p = {p: P.assign_probes(desc, vocab, coarse, FIRST, p) for p in (1, 2, 3, 4, 5, 8)}
    assert np.array_equal(by_p[1], R.assign_cells(desc, vocab, coarse, FIRST))
    assert np.array_equal(by_p[5], flat) and np.array_equal(by_p[8], flat)
    for a, b in ((1, 2), (2, 3), (3, 4), (4, 5)):
        assert (by_p[b][:, 1] <= by_p[a][:, 1]).all(), (a, b)
    for p in (2, 3, 4, 5):
        wins = np.bincount(P.winning_rank(desc, vocab, coarse, FIRST, p), minlength=p)
        print("%s, P = %d: keys won by each probe rank %s" % (family, p, wins.tolist()))
        assert len(wins) == p and (wins >= 30).all(), (family, p, wins)


def test_agreement_with_flat_rises_with_the_probes():
    desc, vocab, coarse = inputs("uniform")
    flat = V.assign(desc, vocab)
    same = [int((P.assign_probes(desc, vocab, coarse, FIRST, p)[:, 0] == flat[:, 0]).sum()) for p in (1, 2, 3, 4, 5)]
    assert same == [41, 83, 121, 164, 257], same


def test_probe_order_of_the_reference():
    """probe_cells: the stable order (dist2, c); its first column is the cells definition's cell; equal coarse rows in ascending c"""
    desc, vocab, coarse = inputs("low")
    cells, dist2 = P.probe_cells(desc, coarse, 8)
    assert cells.shape == (257, 5) and cells.dtype == np.int32 and dist2.dtype == np.int32
    assert np.array_equal(cells[:, 0], V.assign(desc, coarse)[:, 0]) and np.array_equal(dist2[:, 0], V.assign(desc, coarse)[:, 1])
    assert (np.sort(cells, axis=1) == np.arange(5)).all() and (np.diff(dist2, axis=1) >= 0).all()
    ties = np.diff(dist2, axis=1) == 0
    assert ties.sum() >= 20 and (np.diff(cells, axis=1)[ties] > 0).all()   # the `low` family: Hamming distances, ties everywhere
    same = np.repeat(coarse[:1], 4, axis=0)
    assert P.probe_cells(desc[:9], same, 3)[0].tolist() == [[0, 1, 2]] * 9
    assert P.probe_cells(desc[:0], coarse, 3)[0].shape == (0, 3)


def test_constructed_cases_of_the_reference():
    """an unprobed cell never wins; a tie between rows of two probed cells goes to the lower row whatever the ranks"""
    const = lambda vals: np.stack([np.full(128, v, np.uint8) for v in vals])
    coarse = const([100, 110, 120, 130])
    key = const([104])   # ranks: cell 0 (16 per byte), 1 (36), 2 (256), 3 (676)
    assert P.probe_cells(key, coarse, 4)[0].tolist() == [[0, 1, 2, 3]]
    first = [0, 2, 4, 6, 8]
    for p in range(4):
        vocab = const([90, 91, 92, 93, 94, 95, 96, 97])
        vocab[2 * p + 1] = key[0]
        for probes in range(1, 5):
            got = P.assign_probes(key, vocab, coarse, first, probes)[0].tolist()
            assert (got == [2 * p + 1, 0]) == (probes > p), (p, probes, got)
    # the same bytes at row 7 (cell 3) and row 1 (cell 0), coarse rows chosen so that cell 3 ranks first: row 1 wins from P = 4 on
    coarse = const([130, 120, 110, 100])
    vocab = const([90, 104, 92, 93, 94, 95, 96, 104])
    assert P.probe_cells(key, coarse, 4)[0].tolist() == [[3, 2, 1, 0]]
    assert [P.assign_probes(key, vocab, coarse, first, p)[0].tolist() for p in (1, 3, 4)] == [[7, 0], [7, 0], [1, 0]]


def test_entry_points_refuse_without_a_device():
    L = hesaff_amd.load_library()
    p = C.c_int(7)
    assert L.hesaff_set_vocabulary_probes(None, 2) == -2
    assert L.hesaff_get_vocabulary_probes(None, C.byref(p)) == -2 and p.value == 7
    desc = V.family("uniform", 2, seed=1)
    cells = np.full((2, 8), 7, np.int32); dist2 = np.full((2, 8), 7, np.int32)
    assert L.hesaff_stage_probe_cells(None, 2, desc.ctypes.data, cells.ctypes.data, dist2.ctypes.data) == -2
    assert (cells == 7).all() and (dist2 == 7).all()


def test_cli_refuses_bad_probes_before_any_image(tmp_path):
    """--probes without a cells file, outside 1..8, or with --train-vocabulary: the usage text, exit status 1, no file; behind a
    single image: a message, exit status 1, before the image is read"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    lst = str(tmp_path / "no_such_list.txt")
    out = str(tmp_path / "trained.bin")
    some = str(tmp_path / "some.bin")
    cells = some + ".cells"
    hesaff_amd.write_vocabulary(some, V.family("uniform", 4, seed=1))
    hesaff_amd.write_vocabulary_cells(cells, V.family("uniform", 2, seed=1), [0, 1, 4])
    cases = (["--vocabulary", some, "--probes", "2"], ["--probes", "2"], ["--vocabulary", some, "--cells", cells, "--probes", "0"],
             ["--vocabulary", some, "--cells", cells, "--probes", "9"], ["--vocabulary", some, "--cells", cells, "--probes", "2x"],
             ["--vocabulary", some, "--cells", cells, "--probes", "-1"], ["--vocabulary", some, "--cells", cells, "--probes"],
             ["--train-vocabulary", out, "--words", "8", "--cells", "2", "--probes", "2"], ["--train-vocabulary", out, "--words", "8", "--probes", "2"])
    for extra in cases:
        r = subprocess.run([EXE, "--batch", lst] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "", (extra, r.stdout, r.stderr)
        assert r.stderr.startswith("hesaff: usage: hesaff --batch <list file>") and "[--probes 1..8]" in r.stderr, (extra, r.stderr)
    assert not os.path.exists(out) and not os.path.exists(out + ".cells")
    # a good count gets as far as the list, which does not exist
    r = subprocess.run([EXE, "--batch", lst, "--vocabulary", some, "--cells", cells, "--probes", "8"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("hesaff: cannot read list"), r.stderr
    img = str(tmp_path / "no_such_image.pgm")
    for extra in (["--vocabulary", some, "--probes", "2"], ["--probes", "2"], ["--vocabulary", some, "--cells", cells, "--probes", "0"],
                  ["--vocabulary", some, "--cells", cells, "--probes", "9"], ["--vocabulary", some, "--cells", cells, "--probes"]):
        r = subprocess.run([EXE, img] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("hesaff: --probes takes 1 .. 8"), (extra, r.stderr)
    r = subprocess.run([EXE, img, "--vocabulary", some, "--cells", cells, "--probes", "2"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stderr.startswith("hesaff: cannot read '%s'" % img), r.stderr
    # the bare usage text does not change
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.startswith("\nUsage: hesaff image_name.ppm\n") and "probes" not in r.stdout
