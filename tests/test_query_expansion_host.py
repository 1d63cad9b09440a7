"""CPU suite of query expansion (hesaff_expand_query, include/hesaff_amd.h): the definition in numpy (tests/expand_ref.py) against a
plain-Python loop, the host arithmetic of hesaff_amd/csrc/expand_plan.h (a stand-alone program under AddressSanitizer + UBSan), the
refusals that need no device, and the new symbols.  Nothing here needs a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from hesaff_amd import WORDS_ROW_DTYPE as ROW
from tests import expand_ref as X
from tests import verify_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_expand_query", "hesaff_expand_query_device", "hesaff_get_expand_ms")
ARG = -2
F = np.float32


def _loop_expand(q, cands, out, hyp, min_inliers, max_images, roi, max_rows):
    """the definition once more, one float32 operation at a time in Python loops"""
    def live(x, y, a, b, c):
        with np.errstate(all="ignore"):
            r = np.sqrt(c); qq = b / r; t = a - qq * qq; p = np.sqrt(t)
        return bool(c > 0 and t > 0 and F(2.0 ** -20) <= p <= F(2.0 ** 20) and F(2.0 ** -20) <= r <= F(2.0 ** 20) and a <= F(2.0 ** 40)
                    and abs(x) <= F(2.0 ** 20) and abs(y) <= F(2.0 ** 20))
    eligible = [r for r in range(len(cands)) if out[r][0] >= min_inliers]
    selected = sorted(eligible, key=lambda r: (-out[r][0], r))[:max_images]
    rows = [tuple(k) for k in q.tolist()]
    info = [[-1, 0, 0, 0] for _ in cands]
    x0, y0, x1, y1 = (F(v) for v in roi)
    for s, r in enumerate(selected):
        L11, L21, L22 = (F(v) for v in hyp[r])
        xq, yq = F(q["x"][out[r][3]]), F(q["y"][out[r][3]])
        xd, yd = F(cands[r]["x"][out[r][4]]), F(cands[r]["y"][out[r][4]])
        info[r][0] = s
        for k in cands[r]:
            x, y, a, b, c = (F(k[f]) for f in "xyabc")
            if not live(x, y, a, b, c):
                continue
            info[r][1] += 1
            with np.errstate(all="ignore"):
                dx = x - xd; dy = y - yd
                u = dx / L11; t = L21 * u; sv = dy - t; v = sv / L22
                xn = xq + u; yn = yq + v
                m0 = a * L11; m1 = b * L21; e00 = m0 + m1
                m2 = b * L11; m3 = c * L21; e10 = m2 + m3
                e01 = b * L22; e11 = c * L22
                n0 = L11 * e00; n1 = L21 * e10; an = n0 + n1
                n2 = L11 * e01; n3 = L21 * e11; bn = n2 + n3
                cn = L22 * e11
            if x0 <= xn <= x1 and y0 <= yn <= y1 and live(xn, yn, an, bn, cn):
                info[r][2] += 1
                if len(rows) < max_rows:
                    info[r][3] += 1
                    rows.append((xn, yn, an, bn, cn, int(k["word"])))
    return np.array(rows, ROW) if rows else np.zeros(0, ROW), info


def _case():
    """five candidates with maps of every sign of shear, inert keys on both sides, keys outside the region, ties in the inlier count"""
    rng = np.random.RandomState(4)

    def rows(n):
        k = np.zeros(n, ROW)
        p = (0.5 + rng.rand(n)).astype(F); r = (0.5 + rng.rand(n)).astype(F); s = (0.4 * (rng.rand(n) - 0.5)).astype(F)
        k["x"] = (rng.rand(n) * 60 - 10).astype(F); k["y"] = (rng.rand(n) * 60 - 10).astype(F)
        k["a"] = p * p + s * s; k["b"] = s * r; k["c"] = r * r; k["word"] = rng.randint(0, 50, n)
        return k
    q = rows(12)
    q["c"][3] = np.nan
    cands = [rows(n) for n in (30, 0, 17, 9, 25)]
    cands[0]["a"][5] = -1.0; cands[2]["x"][0] = np.inf; cands[4]["b"][7] = np.nan
    out = np.array([[6, 9, 9, 0, 2, 1], [0, 0, 0, -1, -1, 0], [9, 9, 9, 5, 4, 1], [6, 9, 9, 7, 1, 0], [2, 9, 9, 1, 1, 1]], np.int32)
    hyp = np.array([[1.25, 0.5, 0.75], [0, 0, 0], [0.5, -0.25, 2.0], [1.0, 0.0, 1.0], [3.0, 1.0, 0.3]], F)
    return q, cands, out, hyp, (-2.0, 0.0, 45.0, 40.0)


def test_reference_against_a_plain_loop():
    q, cands, out, hyp, roi = _case()
    seen = set()
    for min_inliers, max_images, max_rows in ((6, 1024, 2 ** 18), (6, 2, 2 ** 18), (2, 1024, 2 ** 18), (7, 1, 2 ** 18), (10, 1024, 2 ** 18), (2, 1024, 20), (2, 1024, 12)):
        rows, words, sigs, info = X.expand(q, cands, out, hyp, min_inliers, max_images, roi, max_rows)
        want_rows, want_info = _loop_expand(q, cands, out, hyp, min_inliers, max_images, roi, max_rows)
        assert rows.tobytes() == want_rows.tobytes(), (min_inliers, max_images, max_rows)
        assert info.tolist() == want_info and sigs is None and np.array_equal(words, rows["word"].astype(np.int32))
        assert rows[:len(q)].tobytes() == q.tobytes() and len(rows) <= max_rows
        seen.add(tuple(info[:, 0].tolist()))
    assert seen == {(1, -1, 0, 2, -1), (1, -1, 0, -1, -1), (1, -1, 0, 2, 3), (-1, -1, 0, -1, -1), (-1, -1, -1, -1, -1)}
    # the case does what it is for: keys dropped by the region, inert keys counted out, a cut that falls inside a candidate
    rows, words, sigs, info = X.expand(q, cands, out, hyp, 2, 1024, roi, 20)
    assert (info[[0, 2, 4], 1] == [29, 16, 24]).all() and (0 < info[[0, 2, 3], 2]).all() and (info[:, 2] <= info[:, 1]).all()
    assert info[:, 3].sum() == 20 - 12 and (info[:, 3] < info[:, 2]).any()
    # the signatures travel with their rows
    qs = np.arange(12, dtype=np.uint64) + 1000
    cs = [np.arange(len(c), dtype=np.uint64) + 100 * r for r, c in enumerate(cands)]
    rows, words, sigs, info = X.expand(q, cands, out, hyp, 6, 1024, roi, 2 ** 18, qs, cs)
    assert sigs[:12].tolist() == qs.tolist() and len(sigs) == len(rows)
    first = np.nonzero(X.back_project(cands[2], q[5], cands[2][4], hyp[2], roi)[2])[0]
    assert sigs[12:12 + len(first)].tolist() == (first + 200).tolist()


def test_reference_properties():
    """the anchor maps onto the query's anchor exactly; the identity on small integers is bit-exact; nothing selected: the query"""
    q, cands, out, hyp, roi = _case()
    big = (-2.0 ** 20, -2.0 ** 20, 2.0 ** 20, 2.0 ** 20)
    for r in (0, 2, 3, 4):
        new, live, kept = X.back_project(cands[r], q[out[r][3]], cands[r][out[r][4]], hyp[r], big)
        j = out[r][4]
        assert new["x"][j].tobytes() == q["x"][out[r][3]].tobytes() and new["y"][j].tobytes() == q["y"][out[r][3]].tobytes()
    k = q[V.frames(q)[1]].copy()
    k["x"] = np.arange(len(k)) * 3; k["y"] = np.arange(len(k)) * 5 % 7
    shifted = k.copy(); shifted["x"] += F(41); shifted["y"] -= F(13)
    o = np.array([[len(k), len(k), len(k), 4, 4, 0]], np.int32)
    rows, _, _, info = X.expand(k, [shifted], o, np.array([[1, 0, 1]], F), 1, 1, big)
    assert rows.tobytes() == k.tobytes() + k.tobytes() and info.tolist() == [[0, len(k), len(k), len(k)]]
    rows, _, _, info = X.expand(q, cands, out, hyp, 10, 1024, roi)
    assert rows.tobytes() == q.tobytes() and info.tolist() == [[-1, 0, 0, 0]] * 5


def test_expand_plan_arithmetic(tmp_path):
    """tests/native/expand_plan_check.cpp: every bound on both sides, the selection (ties, min_inliers equality, the max_images cut, a
    broken eligible candidate named, a broken one below min_inliers accepted), the back-projection at its extremes, the tile table
    for 0, 1, 63, 64, 65 rows, the layouts and the working set of the largest call"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "expand_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "expand_plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "expand_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s) and ("int %s(" % s) in header, s
    assert L.hesaff_abi_version() == 8
    for m in ("expand_query", "expand_query_device", "query_index_expanded"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))
    assert isinstance(hesaff_amd.HesaffContext.expand_ms, property)


def test_entry_points_refuse_a_null_context():
    L = hesaff_amd.load_library()
    q = np.zeros(2, ROW); q["a"] = 1; q["c"] = 1
    counts = np.array([2], np.int32)
    out = np.array([[2, 2, 2, 0, 0, 0]], np.int32); hyp = np.array([[1, 0, 1]], F); roi = np.array([-1, -1, 1, 1], F)
    rows = np.full(4, 7, ROW); words = np.full(4, 7, np.int32); info = np.full(4, 7, np.int32); n = C.c_int(7)
    a, b = C.c_float(7), C.c_float(7)
    for f in (L.hesaff_expand_query, L.hesaff_expand_query_device):
        assert f(None, 2, q.ctypes.data, None, 1, counts.ctypes.data, q.ctypes.data, None, out.ctypes.data, hyp.ctypes.data, 1, 1, roi.ctypes.data, 1, 4,
                 rows.ctypes.data, words.ctypes.data, None, C.byref(n), info.ctypes.data) == ARG
    assert L.hesaff_get_expand_ms(None, C.byref(a), C.byref(b)) == ARG
    assert rows.tobytes() == np.full(4, 7, ROW).tobytes() and (words == 7).all() and (info == 7).all() and n.value == 7 and (a.value, b.value) == (7.0, 7.0)


def test_python_forms_refuse_malformed_arguments():
    """the array checks of expand_query come before any library call: no context is needed to meet them"""
    with pytest.raises(ValueError):
        _binding._expand_hypotheses(np.zeros((2, 6), np.int32), np.zeros((3, 3), F), 3)
    with pytest.raises(ValueError):
        _binding._expand_hypotheses(np.zeros((3, 5), np.int32), np.zeros((3, 3), F), 3)
    with pytest.raises(ValueError):
        _binding._expand_roi((0, 0, 1), np.zeros(0, ROW))
    with pytest.raises(ValueError):
        _binding._expand_roi(None, None)
    q, cands, out, hyp, roi = _case()
    live = V.frames(q)[1]
    assert np.array_equal(_binding._live_rows(q), live) and not live.all()
    box = _binding._expand_roi(None, q)
    assert box.dtype == np.float32 and box.tolist() == [q["x"][live].min(), q["y"][live].min(), q["x"][live].max(), q["y"][live].max()]
    assert _binding._expand_roi(None, np.zeros(0, ROW)).tolist() == [0, 0, 0, 0]


def test_cli_expand_usage_errors(tmp_path):
    """--expand takes no value and needs --verify and --query; --min-inliers and --expand-images need --expand and a value in range:
    otherwise the mode's usage line, exit status 1, nothing on stdout, and the lists - which do not exist - are never opened.  The bare
    usage text does not mention the option."""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    lst, q = str(tmp_path / "no_such_list.txt"), str(tmp_path / "no_such_query.hesaff.words")
    for mode in ("--search", "--index"):
        base = [mode, lst, "--query", q]
        v = base + ["--verify"]
        cases = (base + ["--expand"], base + ["--min-inliers", "3"], v + ["--min-inliers", "3"], v + ["--expand-images", "3"], v + ["--expand", "--expand"],
                 v + ["--expand", "yes"], v + ["--expand", "--min-inliers"], v + ["--expand", "--min-inliers", "0"], v + ["--expand", "--min-inliers", "-2"],
                 v + ["--expand", "--min-inliers", "2.5"], v + ["--expand", "--expand-images", "0"], v + ["--expand", "--expand-images", "1025"],
                 v + ["--expand", "--expand-images", "x"], [mode, lst, "--queries", q, "--verify", "--expand"])
        for args in cases:
            r = subprocess.run([EXE] + args, capture_output=True, text=True)
            assert r.returncode == 1 and r.stdout == "", (args, r.stdout, r.stderr)
            assert r.stderr.startswith("hesaff: usage: hesaff %s " % mode) and r.stderr.count("\n") == 1 and "--expand [--min-inliers N]" in r.stderr, (args, r.stderr)
        # well-formed arguments, the options anywhere, reach the list, which cannot be read
        for args in (v + ["--expand"], ["--expand"] + v + ["--min-inliers", "20", "--expand-images", "1024"], ["--expand-images", "1", "--expand"] + v):
            r = subprocess.run([EXE] + args, capture_output=True, text=True)
            assert r.returncode == 1 and r.stdout == "" and "cannot read list" in r.stderr, (args, r.stderr)
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert "--expand" not in r.stderr + r.stdout


def test_expand_interface_compiles():
    """tests/native/expand_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "expand_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
