"""CPU suite of batched index queries (hesaff_index_query_batch*, include/hesaff_amd.h): the symbols, the host arithmetic of
hesaff_amd/csrc/index_batch_plan.h (a stand-alone program under AddressSanitizer + UBSan), the refusals that need no device, the
command line's usage errors and the C++ members.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_index_query_batch", "hesaff_index_query_batch_device", "hesaff_index_query_batch_embedded", "hesaff_index_query_batch_embedded_device",
               "hesaff_index_set_batch_budget", "hesaff_index_get_batch_budget", "hesaff_index_get_batch_chunks", "hesaff_get_index_batch_ms")
ARG = -2


def test_index_batch_plan_arithmetic(tmp_path):
    """tests/native/index_batch_plan_check.cpp: the bounds of a batch on both sides (Q = 1 and 2^16, counts 0 and 2^18, 2^28 words),
    the chunks non-empty, consecutive and covering, a chunk of several queries inside the budget, one-query chunks under a budget too
    small for one, the layouts disjoint and aligned, and no size that wraps at N = 2^20 with 2^18-word queries"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "index_batch_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "index_batch_plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "index_batch_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s), s
        assert re.search(r"^int %s\(" % s, header, re.M), s
    assert L.hesaff_abi_version() == 8 and "#define HESAFF_ABI_VERSION 8" in header
    for m in ("query_index_batch", "query_index_batch_device", "set_index_batch_budget"):
        assert callable(getattr(hesaff_amd.HesaffContext, m)), m
    for p in ("index_batch_budget", "index_batch_chunks", "index_batch_ms"):
        assert isinstance(getattr(hesaff_amd.HesaffContext, p), property), p


def test_entry_points_refuse_a_null_context():
    L = hesaff_amd.load_library()
    counts = np.array([2, 1], np.int32); words = np.array([0, 1, 1], np.int32); sigs = np.zeros(3, np.uint64)
    images = np.full(8, 7, np.int32); scores = np.full(8, 7.0); n = C.c_int(7)
    cp, wp, gp, ip, sp = counts.ctypes.data, words.ctypes.data, sigs.ctypes.data, images.ctypes.data, scores.ctypes.data
    assert L.hesaff_index_query_batch(None, 2, cp, wp, 1, 4, ip, sp, C.byref(n)) == ARG
    assert L.hesaff_index_query_batch_device(None, 2, cp, wp, 1, 4, ip, sp, C.byref(n)) == ARG
    assert L.hesaff_index_query_batch_embedded(None, 2, cp, wp, 1, gp, 8, 4, ip, sp, C.byref(n)) == ARG
    assert L.hesaff_index_query_batch_embedded_device(None, 2, cp, wp, 1, gp, 8, 4, ip, sp, C.byref(n)) == ARG
    size = C.c_size_t(7); chunks = C.c_int(7)
    a, b, c = C.c_float(7), C.c_float(7), C.c_float(7)
    assert L.hesaff_index_set_batch_budget(None, 1 << 20) == ARG
    assert L.hesaff_index_get_batch_budget(None, C.byref(size)) == ARG
    assert L.hesaff_index_get_batch_chunks(None, C.byref(chunks)) == ARG
    assert L.hesaff_get_index_batch_ms(None, C.byref(a), C.byref(b), C.byref(c)) == ARG
    assert (images == 7).all() and (scores == 7.0).all() and n.value == 7 and size.value == 7 and chunks.value == 7
    assert (a.value, b.value, c.value) == (7.0, 7.0, 7.0)


class _NoLibrary:
    """stands where a context would: the Python forms' own checks come before any library call"""
    h = None

    def __getattr__(self, name):
        raise AssertionError("the library was reached: " + name)


def test_python_forms_refuse_malformed_arrays():
    batch = hesaff_amd.HesaffContext.query_index_batch
    device = hesaff_amd.HesaffContext.query_index_batch_device
    budget = hesaff_amd.HesaffContext.set_index_batch_budget
    nothing = _NoLibrary()
    ok = np.array([1, 2, 3], np.int32)
    for bad in (np.zeros(3, np.int64), np.zeros((3, 3), np.int32), np.zeros((2, 2, 2), np.int32), [0, 1, 2]):
        with pytest.raises(ValueError):
            batch(nothing, [ok, bad], 3)
    with pytest.raises(ValueError):   # [n] beside [n, 2]
        batch(nothing, [ok, np.zeros((3, 2), np.int32)], 3)
    sig = np.zeros(3, np.uint64)
    with pytest.raises(ValueError):   # signatures without a threshold, and a threshold without signatures
        batch(nothing, [ok, ok], 3, signatures=[sig, sig])
    with pytest.raises(ValueError):
        batch(nothing, [ok, ok], 3, hamming=8)
    with pytest.raises(ValueError):   # one signature array per query
        batch(nothing, [ok, ok], 3, signatures=[sig], hamming=8)
    with pytest.raises(ValueError):   # one signature per word
        batch(nothing, [ok, ok], 3, signatures=[sig, sig[:2]], hamming=8)
    with pytest.raises(ValueError):
        batch(nothing, [ok, ok], 3, signatures=[sig, np.zeros((3, 1), np.uint64)], hamming=8)
    with pytest.raises(ValueError):
        device(nothing, 0, np.zeros((2, 2), np.int32), 1, 3)
    with pytest.raises(ValueError):
        device(nothing, 0, [3, 3], 1, 3, sigs_ptr=0)
    with pytest.raises(ValueError):
        device(nothing, 0, [3, 3], 1, 3, hamming=8)
    with pytest.raises(ValueError):
        budget(nothing, -1)


def test_cli_queries_usage_errors(tmp_path):
    """--queries with --query, a missing list, --queries without --search or --index: the mode's own usage line, exit status 1,
    nothing on stdout - and the lists are never opened: they name files that do not exist"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    lst, qs, q, ix = str(tmp_path / "no_such_list.txt"), str(tmp_path / "no_such_queries.txt"), str(tmp_path / "no_such_query.hesaff.words"), str(tmp_path / "no_such.index")
    search = "hesaff: usage: hesaff --search <list of .hesaff.words files> --query <.hesaff.words file> | --queries <list of .hesaff.words files>"
    index = "hesaff: usage: hesaff --index <index file> --query <.hesaff.words file> | --queries <list of .hesaff.words files>"
    cases = ((search, ["--search", lst, "--queries", qs, "--query", q]), (search, ["--search", lst, "--query", q, "--queries", qs]),
             (search, ["--search", lst, "--queries"]), (search, ["--queries", "--search", lst]), (search, ["--search", lst, "--queries", qs, "--queries", qs]),
             (search, ["--search", lst, "--queries", qs, "--save-index", ix]), (search, ["--search", lst, "--queries", qs, "--top", "0"]),
             (search, ["--search", lst, "--queries", qs, "--tolerance", "4"]),
             (index, ["--index", ix, "--queries", qs, "--query", q]), (index, ["--index", ix, "--queries"]), (index, ["--index", ix, "--queries", qs, "--add", lst]),
             (index, ["--queries", qs]), (index, ["--queries", qs, "--top", "3"]), (index, ["--queries"]), (index, ["image.pgm", "--queries", qs]))
    for usage, args in cases:
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "", (args, r.stdout, r.stderr)
        assert r.stderr.startswith(usage) and r.stderr.count("\n") == 1, (args, r.stderr)
    # well-formed arguments reach the list, which cannot be read: another message, still nothing on stdout
    r = subprocess.run([EXE, "--search", lst, "--queries", qs, "--top", "3", "--verify"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == "" and "cannot read list" in r.stderr


def test_batch_interface_compiles():
    """tests/native/index_batch_members.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "index_batch_members.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
