"""CPU suite of the growing, durable index (hesaff_index_add, hesaff_index_get_postings, hesaff_index_save / hesaff_index_load,
include/hesaff_amd.h): the numpy definition (tests/index_growth_ref.py), the host arithmetic of hesaff_amd/csrc/index_plan.h and
the reader of the index file under AddressSanitizer + UBSan (stand-alone programs with their own main; nothing is preloaded), file
round trips over host arrays, every refusal of the reader, and the refusals that need no device.  Nothing here needs a GPU."""
import ctypes as C
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import index_growth_ref as G
from tests import index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hesaff_index_add", "hesaff_index_add_device", "hesaff_index_add_embedded", "hesaff_index_add_embedded_device", "hesaff_index_get_postings",
               "hesaff_index_save", "hesaff_index_load", "hesaff_get_index_growth_ms", "hesaff_write_index_file", "hesaff_read_index_file")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
ARG, IO = -2, -4


def _collection(n, k, seed, empty=()):
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, k, rng.randint(1, 30)).astype(np.int32) for _ in range(n)]
    for i in empty:
        images[i] = np.zeros(0, np.int32)
    sigs = [rng.randint(0, 1 << 62, len(w)).astype(np.uint64) for w in images]
    return images, sigs


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s), s
    assert L.hesaff_abi_version() == 8
    for m in ("add_to_index", "add_to_index_device", "save_index", "load_index", "index_postings"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))


def test_the_definition_of_an_add_is_the_build_of_the_concatenation():
    """index_growth_ref.add against a dense computation: the new images take N .. N + m - 1, df adds up, every idf is ilog2_q8 of
    N + m, and the norm of an OLD image changes although its words did not; the lists hold each (image, word) once"""
    k = 13
    old, _ = _collection(4, k, 1, empty=(2,))
    new, _ = _collection(3, k, 2, empty=(1,))
    before, after = R.build(old, k), G.add(old, new, k)
    tf = [[int((img == w).sum()) for w in range(k)] for img in old + new]
    df = [sum(1 for row in tf if row[w]) for w in range(k)]
    assert after[1].tolist() == df and (after[1] >= before[1]).all()
    assert after[2].tolist() == [R.ilog2_q8(7, d) if d else 0 for d in df]
    assert after[3].tolist() == [sum((row[w] * int(after[2][w])) ** 2 for w in range(k)) for row in tf]
    assert after[3][:4].tolist() != before[3].tolist() and after[3][2] == 0 and after[3][5] == 0
    lists = G.postings(after, k)
    assert [len(l) for l in lists] == df and all(tf[i][w] == c for w, l in enumerate(lists) for i, c in l)
    assert all(l == sorted(l) for l in lists)


def test_plan_arithmetic(tmp_path):
    """tests/native/index_growth_plan_check.cpp: index_add_ok on both sides of N + m = 2^20, of 2^28 keys and of a count of 2^18; the
    working set of an add against the build's; the file's layout, head and head rules; the rules of the load in order"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "index_growth_plan_check")
    r = subprocess.run(SAN + ["-o", exe, os.path.join(ROOT, "tests", "native", "index_growth_plan_check.cpp"), "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "index_growth_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


CASES = [("K = 1", 1, 5, ()), ("K = 33", 33, 6, (0, 3)), ("K = 300", 300, 9, (8,)), ("no postings", 33, 3, (0, 1, 2))]


@pytest.mark.parametrize("what,k,n,empty", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("embedded", [False, True], ids=["plain", "embedded"])
def test_file_round_trip_over_host_arrays(tmp_path, what, k, n, empty, embedded):
    """the library's writer against the format written field by field in numpy, byte for byte; the reader returns every array;
    an odd K pads df (and the key counts) to 8 bytes, an odd number of keys the key images"""
    images, sigs = _collection(n, k, 10 * k + n, empty)
    arrays = G.file_arrays(images, k, sigs if embedded else None)
    n_images, n_keys, df, post, kc, ki, ks = arrays
    path = str(tmp_path / "index.bin")
    hesaff_amd.write_index_file(path, *arrays)
    blob = open(path, "rb").read()
    assert blob == G.file_bytes(*arrays), what
    assert len(blob) == G.layout(k, n_keys, len(post), embedded)[5] and len(blob) % 8 == 0
    if k % 2:
        at = G.layout(k, n_keys, len(post), embedded)[1]
        assert blob[at - 4:at] == b"\0" * 4
    f = hesaff_amd.read_index_file(path)
    assert (f["embedded"], f["k"], f["n_images"], f["n_keys"], f["n_postings"]) == (embedded, k, n_images, n_keys, len(post))
    assert np.array_equal(f["df"], df) and np.array_equal(f["postings"], post) and f["postings"].dtype == np.uint32
    if embedded:
        assert np.array_equal(f["key_count"], kc) and np.array_equal(f["key_image"], ki) and np.array_equal(f["key_sig"], ks) and f["key_sig"].dtype == np.uint64
    else:
        assert f["key_count"] is None and f["key_image"] is None and f["key_sig"] is None
    if not len(post):
        assert n_keys == 0 and len(blob) == (40 + 136 if not embedded else 40 + 136 + 136)


def _refused(tmp_path, name, data):
    p = str(tmp_path / name)
    open(p, "wb").write(data)
    with pytest.raises(hesaff_amd.HesaffError) as e:
        hesaff_amd.read_index_file(p)
    assert e.value.code == IO, name


def test_reader_refusals(tmp_path):
    """every refusal of the reader, each from a file that differs from a valid one in exactly that respect"""
    k = 33
    images, sigs = _collection(6, k, 77, empty=(4,))
    for embedded in (False, True):
        a = list(G.file_arrays(images, k, sigs if embedded else None))
        n_images, n_keys, df, post = a[:4]
        good = G.file_bytes(*a)
        p = str(tmp_path / "good.bin")
        open(p, "wb").write(good)
        assert hesaff_amd.read_index_file(p)["n_postings"] == len(post)
        tag = "e_" if embedded else "p_"
        _refused(tmp_path, tag + "short", good[:-1])
        _refused(tmp_path, tag + "short8", good[:-8])
        _refused(tmp_path, tag + "long", good + b"\0")
        _refused(tmp_path, tag + "long8", good + b"\0" * 8)
        _refused(tmp_path, tag + "head_only", good[:40])
        _refused(tmp_path, tag + "cut_head", good[:39])
        _refused(tmp_path, tag + "empty", b"")
        _refused(tmp_path, tag + "magic", b"HESAFFE1" + good[8:])
        _refused(tmp_path, tag + "flags", G.file_bytes(*a, flags=2 | int(embedded)))
        _refused(tmp_path, tag + "reserved", G.file_bytes(*a, reserved=1))
        # K and n_images out of bounds: the arrays of a file whose own fields say so
        _refused(tmp_path, tag + "k0", G.file_bytes(n_images, 0, np.zeros(0, np.uint32), post[:0], *([np.zeros(0, np.uint32)] * 2 + [np.zeros(0, np.uint64)] if embedded else [])))
        _refused(tmp_path, tag + "k_big", good[:12] + np.array([(1 << 20) + 1], "<u4").tobytes() + good[16:])
        _refused(tmp_path, tag + "n0", G.file_bytes(0, *a[1:]))
        _refused(tmp_path, tag + "n_big", G.file_bytes((1 << 20) + 1, *a[1:]))
        _refused(tmp_path, tag + "keys_big", good[:24] + np.array([(1 << 28) + 1], "<u8").tobytes() + good[32:])
        # n_postings > n_keys: a file of the size its fields imply, with every posting in it
        if not embedded:
            _refused(tmp_path, tag + "postings_over_keys", G.file_bytes(n_images, len(post) - 1, df, post))
        # sum(df) != n_postings: one df off, the size unchanged
        bad = df.copy(); used = int(np.nonzero(df)[0][0]); bad[used] -= 1
        _refused(tmp_path, tag + "df_sum", G.file_bytes(n_images, n_keys, bad, post, *a[4:]))
        # a df > n_images with the sum intact: one word takes another's postings
        bad = df.copy(); donors = np.nonzero(df)[0]; need = n_images + 1 - int(bad[donors[0]])
        for w in donors[1:]:
            take = min(int(bad[w]), need); bad[w] -= take; bad[donors[0]] += take; need -= take
        assert need == 0 and bad.sum() == df.sum() and bad.max() == n_images + 1
        _refused(tmp_path, tag + "df_over_n", G.file_bytes(n_images, n_keys, bad, post, *a[4:]))
        if embedded:
            bad = a[4].copy(); bad[int(np.nonzero(bad)[0][0])] += 1
            _refused(tmp_path, tag + "key_count_sum", G.file_bytes(n_images, n_keys, df, post, bad, a[5], a[6]))
    with pytest.raises(hesaff_amd.HesaffError) as e:
        hesaff_amd.read_index_file(str(tmp_path / "no_such_file"))
    assert e.value.code == IO


def test_writer_refuses_what_the_reader_would(tmp_path):
    k = 33
    images, sigs = _collection(6, k, 78)
    n_images, n_keys, df, post, kc, ki, ks = G.file_arrays(images, k, sigs)
    path = str(tmp_path / "never.bin")
    bad_df = df.copy(); bad_df[int(np.nonzero(df)[0][0])] -= 1
    bad_kc = kc.copy(); bad_kc[0] += 1
    for args in ((0, n_keys, df, post), ((1 << 20) + 1, n_keys, df, post), (n_images, len(post) - 1, df, post), (n_images, (1 << 28) + 1, df, post),
                 (n_images, n_keys, bad_df, post), (n_images, n_keys, df, post, bad_kc, ki, ks), (1, n_keys, df, post)):
        with pytest.raises(hesaff_amd.HesaffError) as e:
            hesaff_amd.write_index_file(path, *args)
        assert e.value.code == ARG and not os.path.exists(path)
    L = hesaff_amd.load_library()
    assert L.hesaff_write_index_file(None, 0, k, n_images, n_keys, len(post), df.ctypes.data, post.ctypes.data, None, None, None) == ARG
    assert L.hesaff_write_index_file(os.fsencode(path), 0, k, n_images, n_keys, len(post), None, post.ctypes.data, None, None, None) == ARG
    assert L.hesaff_write_index_file(os.fsencode(path), 0, k, n_images, n_keys, len(post), df.ctypes.data, None, None, None, None) == ARG
    assert L.hesaff_write_index_file(os.fsencode(path), 0, k, n_images, n_keys, len(post), df.ctypes.data, post.ctypes.data, kc.ctypes.data, None, None) == ARG
    assert L.hesaff_write_index_file(os.fsencode(path), 1, k, n_images, n_keys, len(post), df.ctypes.data, post.ctypes.data, None, None, None) == ARG
    assert L.hesaff_write_index_file(os.fsencode(path), 2, k, n_images, n_keys, len(post), df.ctypes.data, post.ctypes.data, kc.ctypes.data, ki.ctypes.data, ks.ctypes.data) == ARG
    assert not os.path.exists(path)


def test_entry_points_refuse_a_null_context_and_null_pointers():
    L = hesaff_amd.load_library()
    counts = np.array([2, 1], np.int32); words = np.array([0, 1, 1], np.int32); sigs = np.zeros(3, np.uint64)
    out = np.full(8, 7, np.uint32)
    ms = [C.c_float(7) for _ in range(5)]
    assert L.hesaff_index_add(None, 2, counts.ctypes.data, words.ctypes.data, 1) == ARG
    assert L.hesaff_index_add_device(None, 2, counts.ctypes.data, words.ctypes.data, 1) == ARG
    assert L.hesaff_index_add_embedded(None, 2, counts.ctypes.data, words.ctypes.data, 1, sigs.ctypes.data) == ARG
    assert L.hesaff_index_add_embedded_device(None, 2, counts.ctypes.data, words.ctypes.data, 1, sigs.ctypes.data) == ARG
    assert L.hesaff_index_get_postings(None, out.ctypes.data, None, None) == ARG
    assert L.hesaff_index_save(None, b"/nowhere") == ARG and L.hesaff_index_load(None, b"/nowhere") == ARG
    assert L.hesaff_get_index_growth_ms(None, *[C.byref(x) for x in ms]) == ARG
    assert (out == 7).all() and all(x.value == 7.0 for x in ms)
    ptr = [C.c_void_p() for _ in range(5)]
    e, k, n, t, p = C.c_int(), C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
    assert L.hesaff_read_index_file(None, C.byref(e), C.byref(k), C.byref(n), C.byref(t), C.byref(p), *[C.byref(q) for q in ptr]) == ARG
    assert L.hesaff_read_index_file(b"/nowhere", None, C.byref(k), C.byref(n), C.byref(t), C.byref(p), *[C.byref(q) for q in ptr]) == ARG
    assert L.hesaff_read_index_file(b"/nowhere", C.byref(e), C.byref(k), C.byref(n), C.byref(t), C.byref(p), *([C.byref(q) for q in ptr[:4]] + [None])) == ARG


# ---------------------------------------------------------------- the reader under the sanitizers

@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    out = str(tmp_path_factory.mktemp("san") / "index_file_sanitize")
    src = [os.path.join(ROOT, "hesaff_amd", "csrc", "hostio.cpp"), os.path.join(ROOT, "hesaff_amd", "csrc", "jpeg_decode.cpp"),
           os.path.join(ROOT, "tests", "native", "index_file_sanitize.cpp")]
    r = subprocess.run(SAN + ["-o", out] + src + ["-lz", "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    return out


def _run(driver, args):
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0:allocator_may_return_null=1", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([driver] + args, capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, "sanitizer or driver failure (rc %d)\n%s\n%s" % (r.returncode, r.stdout[-2000:], r.stderr[-6000:])
    return r.stdout


def _mutants(data, rng, n):
    out = []
    for _ in range(n):
        b = bytearray(data)
        kind = rng.randrange(4)
        if kind == 0:                                      # truncated, often inside the head
            b = b[: rng.randrange(0, 48) if rng.random() < 0.5 else rng.randrange(0, len(b))]
        elif kind == 1:                                    # a few flipped bytes, the head favoured
            for _ in range(rng.randrange(1, 6)):
                pos = rng.randrange(min(len(b), 40)) if rng.random() < 0.7 else rng.randrange(len(b))
                b[pos] = rng.randrange(256)
        elif kind == 2:                                    # a header field blown up (flags, k, n_images, reserved, n_keys, n_postings)
            pos = 8 + 4 * rng.randrange(8)
            b[pos:pos + 4] = bytes([0xFF, 0xFF, 0xFF, rng.randrange(256)])
        else:                                              # a slice removed or duplicated
            i = rng.randrange(len(b)); j = min(len(b), i + rng.randrange(1, 64))
            b = b[:i] + (b[i:j] * 2 if rng.random() < 0.5 else b"") + b[j:]
        out.append(bytes(b))
    return out


def test_reader_on_whole_truncated_and_corrupt_files(driver, tmp_path):
    rng = random.Random(31)
    whole = []
    for k, n, empty, embedded in ((1, 5, (), False), (33, 6, (1,), True), (300, 9, (), True), (33, 3, (0, 1, 2), False), (33, 3, (0, 1, 2), True)):
        images, sigs = _collection(n, k, 3 * k + n, empty)
        whole.append(G.file_bytes(*G.file_arrays(images, k, sigs if embedded else None)))
    paths = []
    for i, data in enumerate(whole):
        paths.append(str(tmp_path / ("whole_%d.bin" % i)))
        open(paths[-1], "wb").write(data)
    assert "whole=5 refused=0" in _run(driver, paths)
    damaged = []
    for i, data in enumerate(whole):
        for j, m in enumerate(_mutants(data, rng, 60)):
            damaged.append(str(tmp_path / ("bad_%d_%d.bin" % (i, j))))
            open(damaged[-1], "wb").write(m)
    # heads that promise far more than the file holds, or whose sizes wrap
    for name, fields in (("huge_k", (0, 0xffffffff, 1, 0, 0, 0)), ("huge_keys", (1, 1, 1, 0, (1 << 64) - 1, 0)), ("huge_postings", (0, 1, 1, 0, 1 << 28, 1 << 28)),
                         ("wrap", (1, 1 << 20, 1 << 20, 0, (1 << 61) + 5, 1 << 61))):
        damaged.append(str(tmp_path / (name + ".bin")))
        open(damaged[-1], "wb").write(b"HESAFFI1" + np.array(fields[:4], "<u4").tobytes() + np.array(fields[4:], "<u8").tobytes() + b"\0" * 64)
    out = _run(driver, damaged)
    whole_n, refused = (int(out.split(t)[1].split()[0]) for t in ("whole=", "refused="))
    assert whole_n + refused == len(damaged) and refused >= len(damaged) * 3 // 4, out   # (a flipped byte inside a list leaves a whole file)


def test_growth_members_compile():
    """tests/native/index_growth_members.cpp compiles against hesaff.hpp with -Wall -Werror"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "index_growth_members.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_cli_index_usage_errors(tmp_path):
    """a bad or missing argument of the index modes: the mode's own usage line, exit status 1, nothing on stdout, and no file is
    opened: every path names a file that does not exist.  Well-formed arguments reach the files, which cannot be read"""
    exe = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
    if not os.path.exists(exe):
        pytest.skip("hesaff CLI not built")
    lst, q, idx = str(tmp_path / "no_such_list.txt"), str(tmp_path / "no_such_query.hesaff.words"), str(tmp_path / "no_such.index")
    search = "hesaff: usage: hesaff --search <list of .hesaff.words files> --query <.hesaff.words file>"
    index = "hesaff: usage: hesaff --index <index file> --query <.hesaff.words file>"
    cases = ((search, ["--search", lst, "--save-index"]), (search, ["--search", lst, "--save-index", idx, "--query", q]), (search, ["--search", lst, "--save-index", idx, "--top", "3"]),
             (search, ["--search", lst, "--save-index", idx, "--verify"]), (search, ["--search", lst, "--save-index", idx, "--save-index", idx]),
             (search, ["--search", lst, "--index", idx, "--query", q]), (search, ["--search", lst, "--query", q, "--add", lst]),
             (index, ["--index", idx]), (index, ["--index"]), (index, ["--index", idx, "--query", q, "--add", lst]), (index, ["--index", idx, "--add", lst, "--top", "3"]),
             (index, ["--index", idx, "--add", lst, "--hamming", "3"]), (index, ["--index", idx, "--add", lst, "--verify"]), (index, ["--index", idx, "--query", q, "--save-index", idx]),
             (index, ["--index", idx, "--query", q, "--top", "0"]), (index, ["--index", idx, "--query", q, "--pairs", "2"]), (index, ["image.pgm", "--index", idx, "--query", q]),
             (index, ["--index", idx, "--index", idx, "--query", q]))
    for usage, args in cases:
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "", (args, r.stdout, r.stderr)
        assert r.stderr.startswith(usage) and r.stderr.count("\n") == 1, (args, r.stderr)
    for args, what in ((["--search", lst, "--save-index", idx], "cannot read list"), (["--index", idx, "--query", q], "cannot read list"),
                       (["--index", idx, "--add", lst], "cannot read list")):
        r = subprocess.run([exe] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stdout == "" and what in r.stderr, (args, r.stderr)
    assert not os.path.exists(idx) and not os.path.exists(idx + ".list")
