"""CPU suite of removal from the image index (hesaff_index_remove, include/hesaff_amd.h): the numpy definition
(tests/index_remove_ref.py) against a dense computation, the host arithmetic of hesaff_amd/csrc/index_remove_plan.h under
AddressSanitizer + UBSan (a stand-alone program with its own main; nothing is preloaded), the CLI's usage errors and refusals, and
the symbols.  Nothing here needs a GPU."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import index_ref as R
from tests import index_remove_ref as X

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NEW_SYMBOLS = ("hesaff_index_remove", "hesaff_get_index_remove_ms")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ARG = -2


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hesaff_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(hesaff_[a-z0-9_]+)\s*\(", header))
    for s in NEW_SYMBOLS:
        assert s in declared and s in _binding.ABI_SYMBOLS and hasattr(L, s), s
    assert L.hesaff_abi_version() == 8
    for m in ("remove_from_index", "index_remove_ms"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))
    assert "removeFromIndex(const std::vector<int> &images)" in open(os.path.join(ROOT, "hesaff_amd", "csrc", "hesaff.hpp")).read()


def test_the_definition_of_a_removal_is_the_build_of_what_remains():
    """index_remove_ref.remove against a dense computation: the tf matrix with rows deleted, df, idf through ilog2_q8 of N - m, the
    norms; the norm of an image that STAYS changes although its words did not; a word whose holders all go ends at df 0 and idf 0; a
    word every remaining image holds ends at idf 0; a removed image without keys only renumbers and changes N"""
    k = 13
    rng = np.random.RandomState(1)
    images = [rng.randint(0, 11, rng.randint(1, 30)).astype(np.int32) for _ in range(7)]
    images[2] = np.zeros(0, np.int32)
    images[5] = np.concatenate([images[5], [11, 11]]).astype(np.int32)       # word 11 is image 5's alone
    images = [np.concatenate([w, [12]]).astype(np.int32) if i not in (2, 3) else w for i, w in enumerate(images)]   # word 12: all but 2 and 3
    gone = [5, 2, 3]
    before = R.build(images, k)
    after, remap = X.remove(images, gone, k)
    assert remap.tolist() == [0, 1, -1, -1, 2, -1, 3] and remap.dtype == np.int32
    tf = np.array([[int((img == w).sum()) for w in range(k)] for img in images])
    left = np.delete(tf, gone, axis=0)
    df = (left > 0).sum(axis=0)
    assert after[1].tolist() == df.tolist() and (after[1] <= before[1]).all()
    idf = [R.ilog2_q8(4, int(d)) if d else 0 for d in df]
    assert after[2].tolist() == idf
    assert after[3].tolist() == [sum((int(row[w]) * idf[w]) ** 2 for w in range(k)) for row in left]
    stay = [0, 1, 4, 6]
    assert after[3].tolist() != before[3][stay].tolist()
    assert before[1][11] == 1 and after[1][11] == 0 and after[2][11] == 0
    assert before[2][12] > 0 and after[1][12] == 4 and after[2][12] == 0
    only_n = X.remove(images, [2], k)[0]
    assert np.array_equal(only_n[1], before[1]) and only_n[2].tolist() == [R.ilog2_q8(6, int(d)) if d else 0 for d in before[1]]
    assert X.remaining("abcdefg", gone) == list("abeg")
    assert X.remap(3, [1]).tolist() == [0, -1, 1] and X.remap(4097, np.arange(4096))[-1] == 0


def test_plan_arithmetic(tmp_path):
    """tests/native/index_remove_plan_check.cpp: index_remove_ok at m = 0, N - 1 and N; the flags of a number of -1, of N and of a
    number twice; the remap at N = 1, 2 and 4097; the scratch and the working-set bytes at the largest index"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "index_remove_plan_check")
    r = subprocess.run(SAN + ["-o", exe, os.path.join(ROOT, "tests", "native", "index_remove_plan_check.cpp"), "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "index_remove_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])
    print(r.stdout)


def test_entry_points_refuse_a_null_context_and_null_pointers():
    L = hesaff_amd.load_library()
    numbers = np.array([0], np.int32)
    out = np.full(4, -77, np.int32)
    ms = [C.c_float(7) for _ in range(4)]
    assert L.hesaff_index_remove(None, 1, numbers.ctypes.data, out.ctypes.data) == ARG
    assert L.hesaff_index_remove(None, 1, None, None) == ARG
    assert L.hesaff_get_index_remove_ms(None, *[C.byref(x) for x in ms]) == ARG
    assert (out == -77).all() and all(x.value == 7.0 for x in ms)


def test_remove_members_compile():
    """tests/native/index_remove_members.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "index_remove_members.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _pair(tmp_path, names):
    """an index file's bytes (never read: every case below ends before the index is) and its list"""
    idx = str(tmp_path / "idx.bin")
    open(idx, "wb").write(b"HESAFFI1 not an index: no removal below may get as far as reading it")
    open(idx + ".list", "w").write("".join(n + "\n" for n in names))
    return idx


def _bytes(idx):
    return open(idx, "rb").read(), open(idx + ".list", "rb").read()


def test_cli_remove_usage_errors(tmp_path):
    """--remove combines with none of --query, --queries, --add, --save-index, --top, --hamming, --verify: the index mode's usage
    line, one line, exit status 1, nothing on stdout, and both files byte for byte what they were"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    idx = _pair(tmp_path, ["a.words", "b.words"])
    gone = str(tmp_path / "gone.txt")
    open(gone, "w").write("a.words\n")
    before = _bytes(idx)
    usage = "hesaff: usage: hesaff --index <index file> --query <.hesaff.words file>"
    search = "hesaff: usage: hesaff --search <list of .hesaff.words files> --query <.hesaff.words file>"
    q = str(tmp_path / "q.hesaff.words")
    cases = ((usage, ["--index", idx, "--remove", gone, "--query", q]), (usage, ["--index", idx, "--remove", gone, "--queries", gone]),
             (usage, ["--index", idx, "--remove", gone, "--add", gone]), (usage, ["--index", idx, "--remove", gone, "--save-index", idx]),
             (usage, ["--index", idx, "--remove", gone, "--top", "3"]), (usage, ["--index", idx, "--remove", gone, "--hamming", "3"]),
             (usage, ["--index", idx, "--remove", gone, "--verify"]), (usage, ["--index", idx, "--remove"]), (usage, ["--index", idx, "--remove", gone, "--remove", gone]),
             (usage, ["--index", idx, "--remove", gone, "--tolerance", "3"]), (search, ["--search", gone, "--remove", gone, "--query", q]))
    for want, args in cases:
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "", (args, r.stdout, r.stderr)
        assert r.stderr.startswith(want) and r.stderr.count("\n") == 1, (args, r.stderr)
        assert "--remove" in r.stderr or want == search, r.stderr
    assert _bytes(idx) == before and sorted(os.listdir(str(tmp_path))) == ["gone.txt", "idx.bin", "idx.bin.list"]


def test_cli_remove_refusals_leave_both_files(tmp_path):
    """a path the list does not hold (named in the message), an empty list, a removal that would leave no image - a path named twice
    counting once, and every line equal to a named path going: one line on stderr, exit status 1, both files as they were"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    idx = _pair(tmp_path, ["a.words", "b.words", "a.words"])
    before = _bytes(idx)
    gone = str(tmp_path / "gone.txt")
    for text, what in (("b.words\nc.words\n", "holds no image 'c.words'"), ("", "names no image"), ("# nothing\n\n", "names no image"),
                       ("a.words\nb.words\n", "would leave no index"), ("b.words\na.words\nb.words\n", "would leave no index")):
        open(gone, "w").write(text)
        r = subprocess.run([EXE, "--index", idx, "--remove", gone], capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and what in r.stderr and r.stderr.count("\n") == 1 and r.stderr.startswith("hesaff: "), (text, r.stderr)
        assert _bytes(idx) == before, text
    r = subprocess.run([EXE, "--index", idx, "--remove", str(tmp_path / "no_such_list.txt")], capture_output=True, text=True)
    assert r.returncode == 1 and r.stdout == "" and "cannot read list" in r.stderr
    assert _bytes(idx) == before and sorted(os.listdir(str(tmp_path))) == ["gone.txt", "idx.bin", "idx.bin.list"]
