"""CPU suite of the image index (hesaff_index_build / hesaff_index_query, include/hesaff_amd.h): the definition in numpy
(tests/index_ref.py) against a brute-force dense computation, the host arithmetic of hesaff_amd/csrc/index_plan.h (a stand-alone
program under AddressSanitizer + UBSan), the words-file reader, and the refusals that need no device.  Nothing here needs a GPU."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_index_build", "hesaff_index_build_device", "hesaff_index_query", "hesaff_index_query_device", "hesaff_index_get_scores",
               "hesaff_index_get_tables", "hesaff_index_get_info", "hesaff_index_clear", "hesaff_get_index_ms", "hesaff_read_words")
ARG, IO = -2, -4


def test_ilog2_q8_values():
    """the values the header states, and floor(256 log2(N / df)) on random pairs but for the truncations (never more than one below)"""
    assert R.ilog2_q8(7, 7) == 0 and R.ilog2_q8(4, 1) == 512 and R.ilog2_q8(3, 2) == 149 and R.ilog2_q8((1 << 24) - 1, 1) == 6143
    rng = np.random.RandomState(5)
    for _ in range(2000):
        n = int(rng.randint(1, 1 << 20))
        df = int(rng.randint(1, n + 1))
        assert 0 <= math.floor(256 * math.log2(n / df)) - R.ilog2_q8(n, df) <= 1, (n, df)


def test_reference_against_a_dense_computation():
    """N = 7 images over K = 13 words as a dense [N, K] tf matrix in Python integers: df, idf, norm2, and for three queries nq2, dot,
    the scores and the ranking; an image without keys, two equal images and a word of every other image are among them"""
    rng = np.random.RandomState(11)
    K = 13
    images = [np.concatenate([[0], rng.randint(0, K, n)]).astype(np.int32) for n in (5, 40, 1, 17)]
    images += [images[1].copy(), np.zeros(0, np.int32), np.array([0, 12, 12, 12], np.int32)]
    N = len(images)
    index = R.build(images, K)
    tf = [[int((img == w).sum()) for w in range(K)] for img in images]
    df = [sum(1 for i in range(N) if tf[i][w] > 0) for w in range(K)]
    idf = [R.ilog2_q8(N, d) if d else 0 for d in df]
    assert index[1].tolist() == df and index[2].tolist() == idf and df[0] == N - 1
    norm2 = [sum((tf[i][w] * idf[w]) ** 2 for w in range(K)) for i in range(N)]
    assert index[3].tolist() == norm2 and norm2[5] == 0
    for q in (images[1], np.array([12, 12, 3], np.int32), np.zeros(0, np.int32)):
        tfq = [int((q == w).sum()) for w in range(K)]
        nq2 = sum((tfq[w] * idf[w]) ** 2 for w in range(K))
        dot = [sum(tfq[w] * tf[i][w] * idf[w] ** 2 for w in range(K)) for i in range(N)]
        score = [0.0 if d == 0 else float(d) / math.sqrt(float(nq2) * float(norm2[i])) for i, d in enumerate(dot)]
        order = sorted(range(N), key=lambda i: (-score[i], i))
        for top in (1, 3, N, N + 5):
            im, sc, rdot, rscore, rnq2 = R.query(index, q, top)
            assert im.tolist() == order[:top] and sc.tolist() == [score[i] for i in order[:top]]
            assert rdot.tolist() == dot and rscore.tolist() == score and rnq2 == nq2
    im, sc, _, _, _ = R.query(index, images[1], 2)
    assert im.tolist() == [1, 4] and sc[0] == sc[1] and abs(sc[0] - 1.0) < 1e-15   # equal images tie, the lower index first


def test_index_plan_arithmetic(tmp_path):
    """tests/native/index_plan_check.cpp: every bound on both sides, ilog2_q8 with its products checked in 128 bits, the worst-case
    sums, the hash size rule at T = 1, 511, 512, 513 and 2^28, the layouts disjoint and aligned, the working set of the largest case;
    index_stage_words at strides 1 .. 3, n = 0, k = 1 and a first or last word of -1 or k; index_starts with zero counts in front,
    inside and behind, n = 0, and a total of exactly 2^32 - 1"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "index_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "index_plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "index_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s), s
    assert L.hesaff_abi_version() == 8
    for m in ("build_index", "build_index_device", "query_index", "query_index_device", "index_scores", "index_tables", "clear_index"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))
    assert isinstance(hesaff_amd.HesaffContext.index_info, property)


def _read_words(path):
    L = hesaff_amd.load_library()
    p = C.c_void_p(); n = C.c_int(7); k = C.c_int(7)
    rc = L.hesaff_read_words(os.fsencode(path), C.byref(p), C.byref(n), C.byref(k))
    if rc != 0:
        assert not p.value and n.value == 0 and k.value == 0
        return rc, None, None
    try:
        words = np.frombuffer(C.string_at(p.value, n.value * 4), np.int32).copy() if n.value else np.zeros(0, np.int32)
    finally:
        L.hesaff_free(p)
    return rc, words, k.value


def test_read_words_round_trip_and_torn_files(tmp_path):
    """a file hesaff_write_words wrote comes back word for word (with the library's own Python reader beside it); no rows: count 0
    and no array; a file cut anywhere, with a byte too many, with another magic or missing: HESAFF_ERR_IO"""
    rng = np.random.RandomState(3)
    keys = np.zeros(37, _binding.KEYPOINT_DTYPE)
    for f in ("x", "y"):
        keys[f] = rng.rand(37) * 100
    keys["s"] = 2.0; keys["a11"] = 1.0; keys["a22"] = 1.0
    words = np.stack([rng.randint(0, 4099, 37), rng.randint(0, 1000, 37)], axis=1).astype(np.int32)
    path = str(tmp_path / "a.hesaff.words")
    hesaff_amd.write_words(path, keys, words, 5.196, 4099)
    rc, got, k = _read_words(path)
    assert rc == 0 and k == 4099 and np.array_equal(got, words[:, 0])
    vs, rows = hesaff_amd.read_words(path)
    assert vs == 4099 and np.array_equal(rows["word"].astype(np.int32), got)
    empty = str(tmp_path / "empty.hesaff.words")
    hesaff_amd.write_words(empty, keys[:0], words[:0], 5.196, 33)
    rc, got, k = _read_words(empty)
    assert rc == 0 and k == 33 and len(got) == 0
    blob = open(path, "rb").read()
    assert len(blob) == 16 + 24 * 37
    for name, data in (("cut_head", blob[:15]), ("cut_row", blob[:16 + 24 * 20 + 7]), ("cut_last", blob[:-1]), ("long", blob + b"\0"),
                       ("magic", b"HESAFFV1" + blob[8:]), ("none", b"")):
        torn = str(tmp_path / name)
        open(torn, "wb").write(data)
        assert _read_words(torn)[0] == IO, name
    assert _read_words(str(tmp_path / "no_such_file"))[0] == IO
    L = hesaff_amd.load_library()
    p = C.c_void_p(); n = C.c_int(); k = C.c_int()
    assert L.hesaff_read_words(None, C.byref(p), C.byref(n), C.byref(k)) == ARG
    assert L.hesaff_read_words(os.fsencode(path), None, C.byref(n), C.byref(k)) == ARG
    assert L.hesaff_read_words(os.fsencode(path), C.byref(p), None, C.byref(k)) == ARG
    assert L.hesaff_read_words(os.fsencode(path), C.byref(p), C.byref(n), None) == ARG


def test_entry_points_refuse_a_null_context():
    L = hesaff_amd.load_library()
    counts = np.array([2, 1], np.int32); words = np.array([0, 1, 1], np.int32)
    images = np.full(4, 7, np.int32); scores = np.full(4, 7.0); n = C.c_int(7)
    a, b = C.c_float(7), C.c_float(7)
    ni, k = C.c_int(7), C.c_int(7)
    t, p = C.c_int64(7), C.c_int64(7)
    assert L.hesaff_index_build(None, 2, counts.ctypes.data, words.ctypes.data, 1, 2) == ARG
    assert L.hesaff_index_build_device(None, 2, counts.ctypes.data, words.ctypes.data, 1, 2) == ARG
    assert L.hesaff_index_query(None, 3, words.ctypes.data, 1, 4, images.ctypes.data, scores.ctypes.data, C.byref(n)) == ARG
    assert L.hesaff_index_query_device(None, 3, words.ctypes.data, 1, 4, images.ctypes.data, scores.ctypes.data, C.byref(n)) == ARG
    assert L.hesaff_index_get_scores(None, None, scores.ctypes.data, None) == ARG
    assert L.hesaff_index_get_tables(None, None, None, None) == ARG
    assert L.hesaff_index_get_info(None, C.byref(ni), C.byref(k), C.byref(t), C.byref(p)) == ARG
    assert L.hesaff_index_clear(None) == ARG
    assert L.hesaff_get_index_ms(None, C.byref(a), C.byref(b)) == ARG
    assert (images == 7).all() and (scores == 7.0).all() and n.value == 7 and (a.value, b.value) == (7.0, 7.0)
    assert (ni.value, k.value, t.value, p.value) == (7, 7, 7, 7)


def test_python_forms_refuse_malformed_word_arrays():
    """the array checks of build_index / query_index come before any library call: no context is needed to meet them"""
    for bad in (np.zeros(3, np.int64), np.zeros((3, 3), np.int32), np.zeros((2, 2, 2), np.int32), [0, 1, 2]):
        with pytest.raises(ValueError):
            _binding._index_words(bad)
    with pytest.raises(ValueError):
        _binding._index_stride([np.zeros(3, np.int32), np.zeros((3, 2), np.int32)])
    assert _binding._index_stride([np.zeros(3, np.int32)]) == 1 and _binding._index_stride([np.zeros((3, 2), np.int32)]) == 2 and _binding._index_stride([]) == 1


def test_cli_search_usage_errors(tmp_path):
    """a bad or missing argument of the search mode: the mode's own usage line, exit status 1, nothing on stdout - and the lists are
    never opened: they name files that do not exist.  --search wins over --batch and over an image argument"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    lst, q = str(tmp_path / "no_such_list.txt"), str(tmp_path / "no_such_query.hesaff.words")
    cases = (["--search", lst], ["--search"], ["--query", q, "--search"], ["--search", lst, "--query"], ["--search", lst, "--query", q, "--top", "0"],
             ["--search", lst, "--query", q, "--top", "1025"], ["--search", lst, "--query", q, "--top", "5x"], ["--search", lst, "--query", q, "--top"],
             ["--search", lst, "--query", q, "--device", "-1"], ["--search", lst, "--query", q, "--device", "x"], ["--search", lst, "--query", q, "--frobnicate", "1"],
             ["--search", lst, "--query", q, "--batch", lst], ["image.pgm", "--search", lst, "--query", q], ["--search", lst, "--search", lst, "--query", q])
    for args in cases:
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "", (args, r.stdout, r.stderr)
        assert r.stderr.startswith("hesaff: usage: hesaff --search <list of .hesaff.words files> --query <.hesaff.words file>"), (args, r.stderr)
        assert r.stderr.count("\n") == 1
    # well-formed arguments reach the list, which cannot be read: another message, still nothing on stdout
    r = subprocess.run([EXE, "--search", lst, "--query", q, "--top", "3"], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == "" and "cannot read list" in r.stderr


def test_index_interface_compiles():
    """tests/native/index_search_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "index_search_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
