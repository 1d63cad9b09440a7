"""CPU suite of vocabulary cells (hesaff_set_vocabulary_cells, include/hesaff_amd.h): the definition in numpy
(tests/vocabulary_cells_ref.py) has the properties the header states, the host arithmetic of hesaff_amd/csrc/cells_plan.h holds the
same numbers (a stand-alone program under AddressSanitizer + UBSan), the cells file makes a round trip and every malformed file is
refused, and the entry points refuse what they must without a device.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import vocabulary_cells_ref as R
from tests import vocabulary_ref as V
from tests import vocabulary_training_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_set_vocabulary_cells", "hesaff_get_vocabulary_cells", "hesaff_get_assign_cells_ms", "hesaff_build_vocabulary_cells",
               "hesaff_train_vocabulary_cells", "hesaff_train_vocabulary_cells_device", "hesaff_read_vocabulary_cells", "hesaff_write_vocabulary_cells")


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s) and ("int %s(" % s) in header, s
    assert L.hesaff_abi_version() == 8
    for m in ("set_vocabulary_cells", "vocabulary_cells", "build_vocabulary_cells", "train_vocabulary_cells", "train_vocabulary_cells_device",
              "train_cell_vocabulary"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))
    assert callable(hesaff_amd.read_vocabulary_cells) and callable(hesaff_amd.write_vocabulary_cells)


def test_cells_plan_arithmetic(tmp_path):
    """tests/native/cells_plan_check.cpp: the rules of `first`, the item bound over distributions of keys, the wave -> cell search against
    a linear walk, the edge-tile mask against the rows of a cell, the slices of a long source, the stable grouping, the scratch layout"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "cells_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "cells_plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "cells_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_cells_interface_compiles():
    """tests/native/vocabulary_cells_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "vocabulary_cells_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cells_file_round_trip(tmp_path):
    coarse = V.family("uniform", 3, seed=7)
    first = np.array([0, 5, 9, 33], np.uint32)
    p = str(tmp_path / "vocab.bin.cells")
    hesaff_amd.write_vocabulary_cells(p, coarse, first)
    assert open(p, "rb").read() == R.cells_file(coarse, first)
    assert not os.path.exists(p + ".part")
    g, f = hesaff_amd.read_vocabulary_cells(p)
    assert np.array_equal(g, coarse) and f.dtype == np.uint32 and np.array_equal(f, first)
    # one cell over one row, the smallest file
    hesaff_amd.write_vocabulary_cells(p, coarse[:1], [0, 1])
    g, f = hesaff_amd.read_vocabulary_cells(p)
    assert np.array_equal(g, coarse[:1]) and f.tolist() == [0, 1]


def test_writer_refuses_a_first_that_is_no_layer(tmp_path):
    coarse = V.family("uniform", 3, seed=7)
    p = str(tmp_path / "bad.cells")
    L = hesaff_amd.load_library()
    for first in ([1, 5, 9, 33], [0, 5, 5, 33], [0, 9, 5, 33], [0, 5, 9, (1 << 20) + 1]):
        f = np.array(first, np.uint32)
        assert L.hesaff_write_vocabulary_cells(os.fsencode(p), 3, coarse.ctypes.data, f.ctypes.data) == -2, first
    f = np.array([0, 5, 9, 33], np.uint32)
    assert L.hesaff_write_vocabulary_cells(os.fsencode(p), 0, coarse.ctypes.data, f.ctypes.data) == -2
    assert L.hesaff_write_vocabulary_cells(os.fsencode(p), 3, None, f.ctypes.data) == -2
    assert L.hesaff_write_vocabulary_cells(os.fsencode(p), 3, coarse.ctypes.data, None) == -2
    assert L.hesaff_write_vocabulary_cells(None, 3, coarse.ctypes.data, f.ctypes.data) == -2
    assert not os.path.exists(p)
    with pytest.raises(ValueError):
        hesaff_amd.write_vocabulary_cells(p, coarse, [0, 5, 33])


def test_every_malformed_cells_file_is_refused(tmp_path):
    coarse = V.family("uniform", 3, seed=7)
    good = R.cells_file(coarse, [0, 5, 9, 33])
    head = lambda dim, cells, rows, reserved: b"HESAFFC1" + struct.pack("<IIII", dim, cells, rows, reserved)
    body = good[24:]
    first_at = 24 + 3 * 128
    with_first = lambda f: good[:first_at] + np.array(f, "<u4").tobytes()
    bad = {
        "empty": b"", "short head": good[:23], "magic": b"HESAFFV1" + good[8:], "dim": head(64, 3, 33, 0) + body, "reserved": head(128, 3, 33, 1) + body,
        "no cells": head(128, 0, 33, 0) + body, "more cells than rows": head(128, 3, 2, 0) + body, "rows beyond 2^20": head(128, 3, (1 << 20) + 1, 0) + body,
        "cells do not match the size": head(128, 4, 33, 0) + body, "truncated": good[:-1], "trailing byte": good + b"\0",
        "first[0] != 0": with_first([1, 5, 9, 33]), "first[c] != rows": with_first([0, 5, 9, 32]), "an empty cell": with_first([0, 5, 5, 33]),
        "not increasing": with_first([0, 9, 5, 33]),
    }
    p = str(tmp_path / "x.cells")
    for name, data in bad.items():
        open(p, "wb").write(data)
        with pytest.raises(hesaff_amd.HesaffError) as e:
            hesaff_amd.read_vocabulary_cells(p)
        assert e.value.code == -4, name
    with pytest.raises(hesaff_amd.HesaffError) as e:
        hesaff_amd.read_vocabulary_cells(str(tmp_path / "no_such_file"))
    assert e.value.code == -4
    open(p, "wb").write(good)
    assert hesaff_amd.read_vocabulary_cells(p)[1].tolist() == [0, 5, 9, 33]


@pytest.mark.parametrize("name", V.FAMILIES)
def test_one_cell_is_the_flat_assignment(name):
    desc = V.family(name, 257, seed=11)
    vocab = V.family(name, 65, seed=12)
    coarse = V.family(name, 1, seed=13)
    assert np.array_equal(R.assign_cells(desc, vocab, coarse, [0, 65]), V.assign(desc, vocab))


def test_a_row_outside_the_cell_never_wins():
    """a constructed case: the key equals row 3, but its nearest coarse row owns rows 0 .. 1"""
    vocab = np.stack([np.full(128, v, np.uint8) for v in (10, 30, 200, 100)])
    coarse = np.stack([np.full(128, 90, np.uint8), np.full(128, 250, np.uint8)])
    first = [0, 2, 4]
    key = np.full((1, 128), 100, np.uint8)
    assert V.assign(key, vocab).tolist() == [[3, 0]]
    assert R.assign_cells(key, vocab, coarse, first).tolist() == [[1, 128 * 70 * 70]]
    # equal coarse rows: the lower cell; duplicate rows in a cell: the lower row
    coarse2 = np.stack([coarse[0], coarse[0]])
    assert R.assign_cells(key, vocab, coarse2, first)[0, 0] == 1
    vocab2 = np.stack([vocab[1], vocab[1], vocab[3], vocab[3]])
    assert R.assign_cells(key, vocab2, coarse, first)[0, 0] == 0


def test_reference_build_and_training():
    words = V.family("uniform", 257, seed=21)
    coarse = V.family("uniform", 33, seed=22)
    coarse[5] = 255 - words[0]   # (still attracts rows or not: whichever - the properties below hold)
    w, order, g, first = R.build_cells(words, coarse)
    assert R.first_ok(first, len(g), 257) and np.array_equal(w, words[order]) and sorted(order.tolist()) == list(range(257))
    cell = V.assign(w, g)[:, 0]
    assert (np.diff(cell) >= 0).all() and np.array_equal(np.bincount(cell), np.diff(first.astype(np.int64)))
    # C = 1: training inside the one cell is flat training from the same rows
    desc = T.clustered(n=515)
    init = T.sample(desc, 33)
    a = R.train_cells(desc, init, V.family("low", 1, seed=1), [0, 33], 4)
    b = T.train(desc, 33, 4, init=init)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))
    # the composite: distortion never increases, first describes the rows
    words, g, first, dist, empty = R.train_cell_vocabulary(desc, 33, 4, 4, 3)
    assert words.shape == (33, 128) and R.first_ok(first, len(g), 33) and (np.diff(dist) <= 0).all() and len(dist) == len(empty)


def test_entry_points_refuse_a_null_context():
    L = hesaff_amd.load_library()
    desc = V.family("uniform", 4, seed=1)
    rows = V.family("uniform", 2, seed=2)
    coarse = V.family("uniform", 1, seed=3)
    first = np.array([0, 2], np.uint32)
    out = np.full((2, 128), 7, np.uint8); order = np.full(2, 7, np.int32); g_out = np.full((1, 128), 7, np.uint8); f_out = np.full(2, 7, np.uint32)
    dist = np.full(3, 7, np.int64); empty = np.full(3, 7, np.int32); done = C.c_int(7); kept = C.c_int(7)
    a, b, f = C.c_float(7), C.c_float(7), C.c_float(7)
    assert L.hesaff_set_vocabulary_cells(None, 1, coarse.ctypes.data, first.ctypes.data) == -2
    assert L.hesaff_get_vocabulary_cells(None, C.byref(kept)) == -2
    assert L.hesaff_get_assign_cells_ms(None, C.byref(a), C.byref(b), C.byref(f)) == -2
    assert L.hesaff_build_vocabulary_cells(None, 2, rows.ctypes.data, 1, coarse.ctypes.data, out.ctypes.data, order.ctypes.data, g_out.ctypes.data,
                                           f_out.ctypes.data, C.byref(kept)) == -2
    assert L.hesaff_train_vocabulary_cells(None, 4, desc.ctypes.data, 2, rows.ctypes.data, 1, coarse.ctypes.data, first.ctypes.data, 3, out.ctypes.data,
                                           dist.ctypes.data, empty.ctypes.data, C.byref(done)) == -2
    assert L.hesaff_train_vocabulary_cells_device(None, 4, desc.ctypes.data, 128, 0, 2, rows.ctypes.data, 1, coarse.ctypes.data, first.ctypes.data, 3,
                                                  out.ctypes.data, dist.ctypes.data, empty.ctypes.data, C.byref(done)) == -2
    assert (out == 7).all() and (order == 7).all() and (g_out == 7).all() and (f_out == 7).all() and (dist == 7).all() and (empty == 7).all()
    assert done.value == 7 and kept.value == 7 and (a.value, b.value, f.value) == (7.0, 7.0, 7.0)


def test_computing_entry_points_fail_loudly_without_a_gpu():
    """no device: creating the context the entry points need raises; with one, the same call computes what the reference does"""
    import torch
    words, coarse = V.family("uniform", 33, seed=2), V.family("uniform", 4, seed=3)
    if torch.cuda.is_available():
        with hesaff_amd.HesaffContext() as ctx:
            got = ctx.build_vocabulary_cells(words, coarse)
        assert all(np.array_equal(g, w) for g, w in zip(got, R.build_cells(words, coarse)))
        return
    with pytest.raises(hesaff_amd.HesaffError) as e:
        with hesaff_amd.HesaffContext() as ctx:
            ctx.build_vocabulary_cells(words, coarse)
    assert "no CPU fallback" in str(e.value) or "HIP" in str(e.value)


def test_cli_refuses_bad_cells_options_before_any_image(tmp_path):
    """--cells without --vocabulary or --train-vocabulary, a cell count that is no number or exceeds --words, --coarse-iterations without
    cells: the usage text, exit status 1, no file; a cells file that cannot be read ends the run before the list is opened"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    lst = str(tmp_path / "no_such_list.txt")
    out = str(tmp_path / "vocab.bin")
    some = str(tmp_path / "some.bin")
    hesaff_amd.write_vocabulary(some, V.family("uniform", 3, seed=1))
    cases = (["--cells", some], ["--train-vocabulary", out, "--words", "8", "--cells", "9"], ["--train-vocabulary", out, "--words", "8", "--cells", "0"],
             ["--train-vocabulary", out, "--words", "8", "--cells", "2x"], ["--train-vocabulary", out, "--words", "8", "--coarse-iterations", "3"],
             ["--train-vocabulary", out, "--words", "8", "--cells", "2", "--coarse-iterations", "0"], ["--vocabulary", some, "--coarse-iterations", "3"],
             ["--vocabulary", some, "--cells"])
    for extra in cases:
        r = subprocess.run([EXE, "--batch", lst] + extra, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "", (extra, r.stdout, r.stderr)
        assert r.stderr.startswith("hesaff: usage: hesaff --batch <list file>"), (extra, r.stderr)
        assert "[--cells <cells file>|C [--coarse-iterations Tc]]" in r.stderr
    assert not os.path.exists(out) and not os.path.exists(out + ".cells")
    # a vocabulary file is no cells file; a cells file over other rows is refused as well
    cells = str(tmp_path / "some.bin.cells")
    hesaff_amd.write_vocabulary_cells(cells, V.family("uniform", 2, seed=1), [0, 1, 4])
    for path in (some, cells, str(tmp_path / "missing.cells")):
        r = subprocess.run([EXE, "--batch", lst, "--vocabulary", some, "--cells", path], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and r.stderr.startswith("hesaff: cannot read cells"), (path, r.stderr)
