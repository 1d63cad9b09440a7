"""CPU suite of visual-word assignment (hesaff_set_vocabulary, include/hesaff_amd.h): the integer identity the device kernel rests
on against the direct definition, the two file formats against tests/vocabulary_ref.py's builders, the resume check of a words file,
and the CLI's refusal of a bad vocabulary file.  Nothing here needs a device."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
OUT_WORDS = 4   # HESAFF_OUT_WORDS


@pytest.mark.parametrize("name", V.FAMILIES)
def test_xor_identity_equals_the_definition(name):
    """|d'|^2 + |w'|^2 - 2 d'.w' in int32 with the first minimum of the score == int64 differences and argmin: n = 200, K = 4099, with
    duplicated rows, an all-0 and an all-255 key and row, so that ties and both ends of the value range are inside"""
    desc = V.family(name, 200, seed=11)
    vocab = V.family(name, 4099, seed=12)
    vocab[40] = vocab[5]
    vocab[3205] = vocab[5]
    vocab[7] = 0
    vocab[9] = 255
    desc[0] = 0
    desc[1] = 255
    desc[2] = vocab[5]
    want = V.assign(desc, vocab)
    got = V.assign_xor(desc, vocab)
    assert np.array_equal(got, want)
    assert tuple(want[2]) == (5, 0)
    if name == "extremes":   # a binary family at K = 4099: tied minima exist, and the first one wins in both forms
        d2 = ((desc[:, None, :].astype(np.int64) - vocab[None, :257, :].astype(np.int64)) ** 2).sum(axis=2)
        assert ((d2 == d2.min(axis=1, keepdims=True)).sum(axis=1) > 1).any()


def test_all_zero_against_all_255_is_the_largest_distance():
    got = V.assign_xor(np.zeros((1, 128), np.uint8), np.full((1, 128), 255, np.uint8))
    assert got.tolist() == [[0, 8323200]] and np.array_equal(got, V.assign(np.zeros((1, 128), np.uint8), np.full((1, 128), 255, np.uint8)))


@pytest.mark.parametrize("k", [1, 33, 4099])
def test_vocabulary_file_round_trip(tmp_path, k):
    vocab = V.family("uniform", k, seed=k)
    p = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(p, vocab)
    assert open(p, "rb").read() == V.vocabulary_file(vocab)
    back = hesaff_amd.read_vocabulary(p)
    assert back.dtype == np.uint8 and back.shape == (k, 128) and np.array_equal(back, vocab)


def test_vocabulary_arrays_that_are_refused(tmp_path):
    p = str(tmp_path / "v.bin")
    good = V.family("uniform", 4, seed=1)
    for bad in (good.astype(np.int8), good[:, :127], good.reshape(-1), np.zeros((0, 128), np.uint8), good.T.copy().T, good.tolist()):
        with pytest.raises(ValueError):
            hesaff_amd.write_vocabulary(p, bad)
    assert not os.path.exists(p)
    L = hesaff_amd.load_library()
    assert L.hesaff_write_vocabulary(os.fsencode(p), good.ctypes.data, 0) == -2
    assert L.hesaff_write_vocabulary(os.fsencode(p), None, 4) == -2
    assert L.hesaff_write_vocabulary(None, good.ctypes.data, 4) == -2
    assert L.hesaff_write_vocabulary(os.fsencode(p), good.ctypes.data, (1 << 20) + 1) == -2


def test_malformed_vocabulary_files_are_refused(tmp_path):
    """truncated (mid-row and at a row boundary), one byte too long, wrong magic, wrong dim, count 0, missing: HESAFF_ERR_IO"""
    vocab = V.family("uniform", 9, seed=3)
    whole = V.vocabulary_file(vocab)
    cases = {
        "mid_row": whole[:-5],
        "row_boundary": whole[:-128],
        "too_long": whole + b"\0",
        "magic": b"HESAFFB1" + whole[8:],
        "dim": whole[:8] + (64).to_bytes(4, "little") + whole[12:],
        "count0": whole[:12] + (0).to_bytes(4, "little"),
        "header_only": whole[:10],
        "empty": b"",
    }
    for name, data in cases.items():
        p = tmp_path / (name + ".bin")
        p.write_bytes(data)
        with pytest.raises(hesaff_amd.HesaffError) as e:
            hesaff_amd.read_vocabulary(str(p))
        assert e.value.code == -4, name
    with pytest.raises(hesaff_amd.HesaffError):
        hesaff_amd.read_vocabulary(str(tmp_path / "missing.bin"))
    L = hesaff_amd.load_library()
    out = C.c_void_p(); k = C.c_int()
    assert L.hesaff_read_vocabulary(None, C.byref(out), C.byref(k)) == -2
    assert L.hesaff_read_vocabulary(b"x", None, C.byref(k)) == -2 and L.hesaff_read_vocabulary(b"x", C.byref(out), None) == -2


def _hand_made_keys(n):
    rng = np.random.RandomState(5)
    keys = np.zeros(n, _binding.KEYPOINT_DTYPE)
    keys["x"] = rng.uniform(0, 500, n); keys["y"] = rng.uniform(0, 400, n); keys["s"] = rng.uniform(1, 30, n)
    keys["a11"] = rng.uniform(0.5, 2, n); keys["a12"] = 0.0; keys["a21"] = rng.uniform(-1, 1, n); keys["a22"] = 1.0 / keys["a11"]
    keys["desc"] = rng.randint(0, 256, (n, 128))
    return keys


@pytest.mark.parametrize("n", [0, 1, 300, 9000])
def test_words_file_bytes(tmp_path, n):
    """hesaff_write_words against the reference builder: the five floats are those of hesaff_write_bin's rows of the same keys (n = 9000:
    more than one block of the writer's buffer), the word is the first column of the (word, dist2) rows"""
    keys = _hand_made_keys(n)
    mr = hesaff_amd.default_params().mrSize
    words = np.stack([np.arange(n, dtype=np.int32) * 7 % 4099, np.arange(n, dtype=np.int32)], axis=1)
    p, b = str(tmp_path / "k.words"), str(tmp_path / "k.bin")
    hesaff_amd.write_words(p, keys, words, mr, 4099)
    hesaff_amd.write_bin(b, keys, mr)
    rows = hesaff_amd.read_bin(b)
    xyabc = np.stack([rows[f] for f in ("x", "y", "a", "b", "c")], axis=1) if n else np.zeros((0, 5), np.float32)
    assert open(p, "rb").read() == V.words_file(xyabc, words, 4099)
    vs, back = hesaff_amd.read_words(p)
    assert vs == 4099 and len(back) == n and np.array_equal(back["word"], words[:, 0].astype(np.uint32))
    assert not [f for f in os.listdir(str(tmp_path)) if ".part." in f]
    L = hesaff_amd.load_library()
    assert L.hesaff_output_is_complete(os.fsencode(p), OUT_WORDS) == n


def test_words_file_argument_checks(tmp_path):
    L = hesaff_amd.load_library()
    keys = _hand_made_keys(2)
    words = np.zeros((2, 2), np.int32)
    p = os.fsencode(str(tmp_path / "w"))
    assert L.hesaff_write_words(None, keys.ctypes.data, words.ctypes.data, 2, 5.0, 3) == -2
    assert L.hesaff_write_words(p, None, words.ctypes.data, 2, 5.0, 3) == -2
    assert L.hesaff_write_words(p, keys.ctypes.data, None, 2, 5.0, 3) == -2
    assert L.hesaff_write_words(p, keys.ctypes.data, words.ctypes.data, -1, 5.0, 3) == -2
    assert not os.path.exists(str(tmp_path / "w"))


def test_output_is_complete_for_words_files(tmp_path):
    """the size check 16 + 24 * count: a complete file, one cut at a row boundary, one cut mid-row, a sidecar's magic"""
    L = hesaff_amd.load_library()
    keys = _hand_made_keys(10)
    whole = tmp_path / "whole.words"
    hesaff_amd.write_words(str(whole), keys, np.zeros((10, 2), np.int32), 5.0, 77)
    data = whole.read_bytes()
    assert len(data) == 16 + 24 * 10
    assert L.hesaff_output_is_complete(os.fsencode(str(whole)), OUT_WORDS) == 10
    for name, cut in (("row_boundary", data[:-24]), ("mid_row", data[:-7]), ("magic", b"HESAFFB1" + data[8:]), ("header", data[:12])):
        q = tmp_path / (name + ".words")
        q.write_bytes(cut)
        assert L.hesaff_output_is_complete(os.fsencode(str(q)), OUT_WORDS) == -1, name
    assert L.hesaff_output_is_complete(os.fsencode(str(tmp_path / "none.words")), OUT_WORDS) == -1
    assert L.hesaff_output_is_complete(os.fsencode(str(whole)), 2) == -1   # not a sidecar


def test_entry_points_refuse_a_null_context():
    L = hesaff_amd.load_library()
    k = C.c_int(7); p = C.c_void_p(); n = C.c_int(); tot = C.c_int64(); ms = C.c_float()
    v = V.family("uniform", 2, seed=1)
    out = np.zeros((2, 2), np.int32)
    assert L.hesaff_set_vocabulary(None, 2, v.ctypes.data) == -2 and L.hesaff_set_vocabulary(None, 0, None) == -2
    assert L.hesaff_get_vocabulary_size(None, C.byref(k)) == -2 and k.value == 7
    assert L.hesaff_get_words(None, 0, C.byref(p), C.byref(n)) == -2
    assert L.hesaff_get_words_device(None, C.byref(p), C.byref(tot)) == -2
    assert L.hesaff_assign_words_device(None, 2, None, 128, 0, None) == -2
    assert L.hesaff_stage_assign_words(None, 2, v.ctypes.data, out.ctypes.data) == -2
    assert L.hesaff_get_assign_ms(None, C.byref(ms)) == -2


def test_cli_refuses_a_bad_vocabulary_before_any_image(tmp_path):
    """--vocabulary with a missing, truncated or mis-tagged file: a message on stderr naming the file, exit status 1, nothing on stdout
    and no output file - in the batch form and behind a single image, even when the image itself is unreadable (it is never opened)"""
    if not os.path.exists(EXE):
        pytest.skip("hesaff CLI not built")
    img = str(tmp_path / "band.pgm")
    with open(os.path.join(GOLD, "band_96x96.pgm"), "rb") as f, open(img, "wb") as g:
        g.write(f.read())
    lst = tmp_path / "list.txt"
    lst.write_text(img + "\n")
    whole = V.vocabulary_file(V.family("uniform", 5, seed=2))
    bad = {"missing.bin": None, "cut.bin": whole[:-3], "magic.bin": b"HESAFFW1" + whole[8:], "dim.bin": whole[:8] + (127).to_bytes(4, "little") + whole[12:]}
    for name, data in bad.items():
        v = str(tmp_path / name)
        if data is not None:
            open(v, "wb").write(data)
        for args in ([img, "--vocabulary", v], ["--batch", str(lst), "--vocabulary", v], ["--batch", str(lst), "--vocabulary", v, "--words-only"],
                     [str(tmp_path / "no_such_image.pgm"), "--vocabulary", v]):
            r = subprocess.run([EXE] + args, capture_output=True, text=True)
            assert r.returncode == 1, (args, r.stdout, r.stderr)
            assert r.stderr.startswith("hesaff: cannot read vocabulary '%s'" % v), r.stderr
            assert r.stdout == ""
    for args in ([img, "--vocabulary"], ["--batch", str(lst), "--words-only"], ["--batch", str(lst), "--vocabulary"]):
        r = subprocess.run([EXE] + args, capture_output=True, text=True)
        assert r.returncode == 1 and r.stderr.startswith("hesaff: ") and r.stdout == "", (args, r.stdout, r.stderr)
    for suffix in (".hesaff.sift", ".hesaff.words", ".hesaff.bin"):
        assert not os.path.exists(img + suffix)


def test_words_interface_compiles():
    """tests/native/vocabulary_keys.cpp compiles against hesaff.hpp with -Wall -Werror"""
    import shutil
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    src = os.path.join(ROOT, "tests", "native", "vocabulary_keys.cpp")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
