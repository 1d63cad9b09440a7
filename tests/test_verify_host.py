"""CPU suite of spatial verification (hesaff_verify_matches, include/hesaff_amd.h): the definition in numpy (tests/verify_ref.py)
against a plain-Python triple loop, the host arithmetic of hesaff_amd/csrc/verify_plan.h (a stand-alone program under
AddressSanitizer + UBSan), the rows reader, and the refusals that need no device.  Nothing here needs a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from hesaff_amd import WORDS_ROW_DTYPE as ROW
from tests import verify_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_verify_matches", "hesaff_verify_matches_device", "hesaff_verify_get_pairs", "hesaff_verify_get_query_inert",
               "hesaff_stage_verify_pairs", "hesaff_get_verify_ms", "hesaff_read_words_rows")
ARG, IO = -2, -4
F = np.float32


def _loop_verify(q, cands, P, tol):
    """the definition once more, one float32 operation at a time in Python loops"""
    def frame(k):
        x, y, a, b, c = (F(k[f]) for f in "xyabc")
        with np.errstate(all="ignore"):
            r = np.sqrt(c); qq = b / r; t = a - qq * qq; p = np.sqrt(t)
        live = bool(c > 0 and t > 0 and F(2.0 ** -20) <= p <= F(2.0 ** 20) and F(2.0 ** -20) <= r <= F(2.0 ** 20) and a <= F(2.0 ** 40)
                    and abs(x) <= F(2.0 ** 20) and abs(y) <= F(2.0 ** 20))
        return (x, y, p, qq, r), live
    fq = [frame(k) for k in q]
    res = []
    for cand in cands:
        fc = [frame(k) for k in cand]
        pairs = []
        for j, (dj, lj) in enumerate(fc):
            if not lj:
                continue
            w = cand["word"][j]
            tfq = sum(1 for i, (_, li) in enumerate(fq) if li and q["word"][i] == w)
            tf = sum(1 for jj, (_, ll) in enumerate(fc) if ll and cand["word"][jj] == w)
            if tfq * tf <= P:
                pairs += [(i, j) for i, (_, li) in enumerate(fq) if li and q["word"][i] == w]
        found, pairs = len(pairs), pairs[:4096]
        best = (0, -1, F(0), F(0), F(0))
        tol2 = F(tol) * F(tol)
        for h, (ih, jh) in enumerate(pairs):
            (xq, yq, pq, qq, rq), (xd, yd, pd, qd, rd) = fq[ih][0], fc[jh][0]
            L11 = pq / pd; L22 = rq / rd; L21 = (qq - qd * L11) / rd
            inl = 0
            for ik, jk in pairs:
                dx = fq[ik][0][0] - xq; dy = fq[ik][0][1] - yq
                u = L11 * dx; v = L21 * dx + L22 * dy
                ex = (xd + u) - fc[jk][0][0]; ey = (yd + v) - fc[jk][0][1]
                inl += bool(ex * ex + ey * ey <= tol2)
            if inl > best[0]:
                best = (inl, h, L11, L21, L22)
        i, j = pairs[best[1]] if best[1] >= 0 else (-1, -1)
        res.append(([best[0], len(pairs), found, i, j, sum(1 for _, l in fc if not l)], [best[2], best[3], best[4]], pairs))
    order = sorted(range(len(cands)), key=lambda r: (-res[r][0][0], r))
    return res, order, sum(1 for _, l in fq if not l)


def _case():
    """R = 4, M <= 30: an image without keys, inert keys on both sides, a word with tfq * tf = P = 4 and one with P + 1"""
    rng = np.random.RandomState(2)

    def rows(words):
        k = np.zeros(len(words), ROW)
        p = (0.5 + rng.rand(len(k))).astype(F); r = (0.5 + rng.rand(len(k))).astype(F); s = (0.4 * (rng.rand(len(k)) - 0.5)).astype(F)
        k["x"] = (rng.rand(len(k)) * 40).astype(F); k["y"] = (rng.rand(len(k)) * 40).astype(F)
        k["a"] = p * p + s * s; k["b"] = s * r; k["c"] = r * r; k["word"] = words
        return k
    q = rows([0, 0, 1, 2, 3, 4, 5, 5, 5, 5, 5, 6, 7, 8, 9])
    q["c"][12] = np.nan; q["a"][13] = 0.0                          # the keys of words 7 and 8 are inert
    a = rows([0, 0, 1, 1, 2, 3, 4, 5, 6, 9, 7])                    # word 0: 2 x 2 = P; word 5: 5 x 1 = P + 1; word 7: the query's key is inert
    a["x"][:9] = q["x"][[0, 1, 2, 2, 3, 4, 5, 6, 11]] + F(3); a["y"][:9] = q["y"][[0, 1, 2, 2, 3, 4, 5, 6, 11]] - F(2)
    b = rows([9, 9, 9, 9, 9, 0, 1, 3]); b["x"][0] = np.inf         # word 9: 1 x 4 = P with the inert key left out, 1 x 5 otherwise
    return q, [a, np.zeros(0, ROW), b, rows([11, 12, 13])], 4


def test_reference_against_a_triple_loop():
    q, cands, P = _case()
    for tol in (1.5, 6.0):
        out, hyp, order, lists, qinert = R.verify(q, cands, P, tol)
        res, want_order, want_qinert = _loop_verify(q, cands, P, tol)
        assert out.tolist() == [r[0] for r in res], tol
        assert np.array_equal(hyp.view(np.uint32), np.array([r[1] for r in res], F).view(np.uint32))
        assert order.tolist() == want_order and qinert == want_qinert == 2
        for got, r in zip(lists, res):
            assert got.tolist() == [list(p) for p in r[2]]
        assert 0 < out[0, 1] <= 30 and out[0, 2] == 4 + 2 + 1 + 1 + 1 + 1 + 1 and out[1].tolist() == [0, 0, 0, -1, -1, 0]
        assert out[2, 2] == 4 + 2 + 1 + 1 and out[2, 5] == 1 and out[3].tolist() == [0, 0, 0, -1, -1, 0]
    assert R.verify(q, cands, P, 6.0)[0][0, 0] >= R.verify(q, cands, P, 1.5)[0][0, 0] >= 1


def test_verify_plan_arithmetic(tmp_path):
    """tests/native/verify_plan_check.cpp: every bound on both sides, the liveness rule at its edges (p and r at exactly 2^-20 and
    2^20, t the smallest positive float, a NaN in each field), the layouts disjoint and aligned, the working set of the largest call"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "verify_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "verify_plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "verify_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s) and ("int %s(" % s) in header, s
    assert L.hesaff_abi_version() == 8
    for m in ("verify_matches", "verify_matches_device", "verify_pairs", "stage_verify_pairs"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))


def test_entry_points_refuse_a_null_context():
    L = hesaff_amd.load_library()
    q = np.zeros(2, ROW); q["a"] = 1; q["c"] = 1
    counts = np.array([2], np.int32)
    out = np.full(6, 7, np.int32); hyp = np.full(3, 7, F); order = np.full(1, 7, np.int32)
    inl = np.full(2, 7, np.int32); best = C.c_int32(7)
    pairs = C.c_void_p(7); n = C.c_int(7)
    a, b = C.c_float(7), C.c_float(7)
    corr = np.ones((2, 10), F)
    for f in (L.hesaff_verify_matches, L.hesaff_verify_matches_device):
        assert f(None, 2, q.ctypes.data, 1, counts.ctypes.data, q.ctypes.data, 2, 1, 5.0, out.ctypes.data, hyp.ctypes.data, order.ctypes.data) == ARG
    assert L.hesaff_verify_get_pairs(None, 0, C.byref(pairs), C.byref(n)) == ARG
    assert L.hesaff_verify_get_query_inert(None, C.byref(n)) == ARG
    assert L.hesaff_stage_verify_pairs(None, 2, corr.ctypes.data, 5.0, inl.ctypes.data, C.byref(best)) == ARG
    assert L.hesaff_get_verify_ms(None, C.byref(a), C.byref(b)) == ARG
    assert (out == 7).all() and (hyp == 7).all() and (order == 7).all() and (inl == 7).all() and best.value == 7
    assert pairs.value == 7 and n.value == 7 and (a.value, b.value) == (7.0, 7.0)


def test_python_forms_refuse_malformed_rows():
    """the array checks of verify_matches come before any library call: no context is needed to meet them"""
    for bad in (np.zeros(3, np.int32), np.zeros((3, 6), np.float32), np.zeros((2, 2), ROW), [0, 1, 2]):
        with pytest.raises(ValueError):
            _binding._verify_rows(bad)
    assert _binding._verify_rows(np.zeros(3, ROW)[::2]).flags["C_CONTIGUOUS"]


def _read_rows(path):
    L = hesaff_amd.load_library()
    p = C.c_void_p(); n = C.c_int(7); k = C.c_int(7)
    rc = L.hesaff_read_words_rows(os.fsencode(path), C.byref(p), C.byref(n), C.byref(k))
    if rc != 0:
        assert not p.value and n.value == 0 and k.value == 0
        return rc, None, None
    try:
        rows = np.frombuffer(C.string_at(p.value, n.value * 24), ROW).copy() if n.value else np.zeros(0, ROW)
        assert bool(p.value) == (n.value > 0)
    finally:
        L.hesaff_free(p)
    return rc, rows, k.value


def test_read_words_rows_round_trip_and_torn_files(tmp_path):
    """a file hesaff_write_words wrote comes back row for row, byte-equal to the library's own Python reader; no rows: count 0 and no
    array; a file cut anywhere, with a byte too many, with another magic or missing: HESAFF_ERR_IO"""
    rng = np.random.RandomState(3)
    keys = np.zeros(37, _binding.KEYPOINT_DTYPE)
    for f in ("x", "y"):
        keys[f] = rng.rand(37) * 100
    keys["s"] = 2.0; keys["a11"] = 1.0; keys["a22"] = 1.0; keys["a21"] = 0.25
    words = np.stack([rng.randint(0, 4099, 37), rng.randint(0, 1000, 37)], axis=1).astype(np.int32)
    path = str(tmp_path / "a.hesaff.words")
    hesaff_amd.write_words(path, keys, words, 5.196, 4099)
    rc, got, k = _read_rows(path)
    vs, rows = hesaff_amd.read_words(path)
    assert rc == 0 and k == vs == 4099 and got.tobytes() == rows.tobytes() and np.array_equal(got["word"].astype(np.int32), words[:, 0])
    assert np.array_equal(got["x"], keys["x"]) and R.frames(got)[1].all()
    empty = str(tmp_path / "empty.hesaff.words")
    hesaff_amd.write_words(empty, keys[:0], words[:0], 5.196, 33)
    rc, got, k = _read_rows(empty)
    assert rc == 0 and k == 33 and len(got) == 0
    blob = open(path, "rb").read()
    for name, data in (("cut_head", blob[:15]), ("cut_row", blob[:16 + 24 * 20 + 7]), ("cut_last", blob[:-1]), ("long", blob + b"\0"),
                       ("magic", b"HESAFFV1" + blob[8:]), ("none", b"")):
        torn = str(tmp_path / name)
        open(torn, "wb").write(data)
        assert _read_rows(torn)[0] == IO, name
    assert _read_rows(str(tmp_path / "no_such_file"))[0] == IO
    L = hesaff_amd.load_library()
    p = C.c_void_p(); n = C.c_int(); k = C.c_int()
    assert L.hesaff_read_words_rows(None, C.byref(p), C.byref(n), C.byref(k)) == ARG
    assert L.hesaff_read_words_rows(os.fsencode(path), None, C.byref(n), C.byref(k)) == ARG
    assert L.hesaff_read_words_rows(os.fsencode(path), C.byref(p), None, C.byref(k)) == ARG
    assert L.hesaff_read_words_rows(os.fsencode(path), C.byref(p), C.byref(n), None) == ARG


def test_cli_verify_usage_errors(tmp_path):
    """--verify takes no value; --tolerance and --pairs need it and a value in range: otherwise the search mode's usage line, exit
    status 1, nothing on stdout, and the lists - which do not exist - are never opened"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    lst, q = str(tmp_path / "no_such_list.txt"), str(tmp_path / "no_such_query.hesaff.words")
    base = ["--search", lst, "--query", q]
    cases = (base + ["--tolerance", "5"], base + ["--pairs", "2"], base + ["--verify", "--tolerance"], base + ["--verify", "--pairs"],
             base + ["--verify", "--tolerance", "0"], base + ["--verify", "--tolerance", "-1"], base + ["--verify", "--tolerance", "nan"],
             base + ["--verify", "--tolerance", "inf"], base + ["--verify", "--tolerance", "1048577"], base + ["--verify", "--tolerance", "5px"],
             base + ["--verify", "--pairs", "0"], base + ["--verify", "--pairs", "17"], base + ["--verify", "--pairs", "2.5"],
             base + ["--verify", "--verify"], base + ["--verify", "yes"], ["--verify"] + base[:2], ["--search", lst, "--verify", "--query"])
    for args in cases:
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "", (args, r.stdout, r.stderr)
        assert r.stderr.startswith("hesaff: usage: hesaff --search <list of .hesaff.words files> --query <.hesaff.words file>"), (args, r.stderr)
        assert r.stderr.count("\n") == 1 and "--verify" in r.stderr
    # well-formed arguments, --verify anywhere, reach the list, which cannot be read
    for args in (base + ["--verify"], ["--verify"] + base + ["--tolerance", "2.5", "--pairs", "16"], base[:2] + ["--pairs", "1", "--verify", "--top", "3"] + base[2:]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and "cannot read list" in r.stderr, (args, r.stderr)


def test_verify_interface_compiles():
    """tests/native/verify_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "verify_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
