"""CPU suite of Hamming embedding (hesaff_set_embedding and the symbols declared with it, include/hesaff_amd.h): the C generator of the
default projection against the numpy one and against the definition in Python integers (tests/embedding_ref.py), the host arithmetic
of hesaff_amd/csrc/embed_plan.h (a stand-alone program under AddressSanitizer + UBSan), the two file formats, the refusals that need
no device, and the reference's own consequences: T = 64 is the plain query, and dot never decreases with T.  Nothing here needs a GPU."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests import embedding_ref as E
from tests import index_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("hesaff_embedding_projection", "hesaff_set_embedding", "hesaff_get_embedding", "hesaff_get_signatures", "hesaff_get_signatures_device",
               "hesaff_embed_device", "hesaff_stage_embed", "hesaff_stage_project", "hesaff_train_embedding", "hesaff_train_embedding_device",
               "hesaff_get_embedding_ms", "hesaff_index_build_embedded", "hesaff_index_build_embedded_device", "hesaff_index_query_embedded",
               "hesaff_index_query_embedded_device", "hesaff_index_get_embedded", "hesaff_write_embedding", "hesaff_read_embedding",
               "hesaff_write_signatures", "hesaff_read_signatures", "hesaff_signatures_is_complete")
ARG, IO = -2, -4


def _c_projection(seed):
    P = np.full((64, 128), -128, np.int8)
    assert hesaff_amd.load_library().hesaff_embedding_projection(C.c_uint64(seed), P.ctypes.data) == 0
    return P


@pytest.mark.parametrize("seed", [0, 1, (1 << 64) - 1])
def test_generator_c_numpy_and_definition_agree(seed):
    P = _c_projection(seed)
    assert P.dtype == np.int8 and P.shape == (64, 128)
    assert np.array_equal(P, hesaff_amd.embedding_projection(seed)), "C against numpy"
    assert np.array_equal(P, E.projection(seed)), "C against the definition in Python integers"
    assert not (P == -128).any() and P.min() >= -127
    assert len(np.unique(P)) > 200   # (a byte stream, not a constant)


def test_generator_values_and_refusal():
    # splitmix64 from 0 yields 0xE220A8397B1DCDAF first: its top byte, 226, less 128
    assert _c_projection(0)[0, 0] == 98
    assert not np.array_equal(_c_projection(0), _c_projection(1))
    assert hesaff_amd.load_library().hesaff_embedding_projection(C.c_uint64(0), None) == ARG


def test_embed_plan_arithmetic(tmp_path):
    """tests/native/embed_plan_check.cpp: the bounds on both sides, the generator, the packed projection summed the way the kernel
    sums it (signed bytes plus the bias) against P . d at both ends of the range, the file heads, the layouts disjoint and aligned"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "embed_plan_check")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
           "-o", exe, os.path.join(ROOT, "tests", "native", "embed_plan_check.cpp"), "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "embed_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_new_symbols_are_declared_exported_and_listed():
    L = hesaff_amd.load_library()
    header = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    for s in NEW_SYMBOLS:
        assert s in _binding.ABI_SYMBOLS and hasattr(L, s) and ("int %s(" % s) in header, s
    assert L.hesaff_abi_version() == 8 and "#define HESAFF_ABI_VERSION 8" in header and "#define HESAFF_EMBED_BITS 64" in header
    assert hesaff_amd.EMBED_BITS == 64
    for m in ("set_embedding", "embedding", "signatures", "embed", "train_embedding", "build_embedded_index", "project", "index_embedded"):
        assert callable(getattr(hesaff_amd.HesaffContext, m))
    for f in ("embedding_projection", "read_signatures", "write_signatures", "read_embedding", "write_embedding"):
        assert callable(getattr(hesaff_amd, f))


# ---------------------------------------------------------------- files

def _embedding(k, seed=3):
    rng = np.random.RandomState(seed)
    tau = rng.randint(-(1 << 22), 1 << 22, (k, 64)).astype(np.int32)
    tau[0, 0], tau[-1, -1] = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    return hesaff_amd.embedding_projection(seed), tau


def _read_embedding_rc(path):
    L = hesaff_amd.load_library()
    P = C.c_void_p(); tau = C.c_void_p(); k = C.c_int(7)
    rc = L.hesaff_read_embedding(os.fsencode(path), C.byref(P), C.byref(tau), C.byref(k))
    if rc == 0:
        L.hesaff_free(P); L.hesaff_free(tau)
    else:
        assert P.value is None and tau.value is None and k.value == 0
    return rc


def _read_signatures_rc(path):
    L = hesaff_amd.load_library()
    p = C.c_void_p(); n = C.c_int(7)
    rc = L.hesaff_read_signatures(os.fsencode(path), C.byref(p), C.byref(n))
    if rc == 0:
        L.hesaff_free(p)
    else:
        assert p.value is None and n.value == 0
    return rc


@pytest.mark.parametrize("k", [1, 33, 300])
def test_embedding_file_round_trip(tmp_path, k):
    P, tau = _embedding(k)
    path = str(tmp_path / "he.bin")
    hesaff_amd.write_embedding(path, P, tau)
    raw = open(path, "rb").read()
    assert raw[:8] == b"HESAFFE1" and np.frombuffer(raw[8:24], "<u4").tolist() == [64, 128, k, 0] and len(raw) == 24 + 8192 + 256 * k
    assert raw[24:24 + 8192] == P.tobytes() and raw[24 + 8192:] == tau.astype("<i4").tobytes()
    P2, tau2 = hesaff_amd.read_embedding(path)
    assert P2.dtype == np.int8 and tau2.dtype == np.int32 and np.array_equal(P2, P) and np.array_equal(tau2, tau)
    assert not os.path.exists(path + ".part")


def test_embedding_file_refusals(tmp_path):
    P, tau = _embedding(33)
    path = str(tmp_path / "he.bin")
    hesaff_amd.write_embedding(path, P, tau)
    raw = open(path, "rb").read()

    def rc_of(data):
        q = str(tmp_path / "bad.bin")
        open(q, "wb").write(data)
        return _read_embedding_rc(q)
    assert rc_of(raw) == 0
    assert rc_of(raw[:-1]) == IO and rc_of(raw[:24]) == IO and rc_of(raw[:10]) == IO and rc_of(b"") == IO and rc_of(raw + b"\0") == IO, "truncated or too long"
    assert rc_of(b"HESAFFE2" + raw[8:]) == IO and rc_of(b"HESAFFV1" + raw[8:]) == IO, "a wrong magic"
    u32 = lambda v: np.array([v], "<u4").tobytes()
    assert rc_of(raw[:8] + u32(32) + raw[12:]) == IO, "wrong bits"
    assert rc_of(raw[:12] + u32(64) + raw[16:]) == IO, "wrong dim"
    assert rc_of(raw[:16] + u32(34) + raw[20:]) == IO and rc_of(raw[:16] + u32(0) + raw[20:]) == IO, "k against the size"
    assert rc_of(raw[:20] + u32(1) + raw[24:]) == IO, "reserved"
    assert rc_of(raw[:24 + 100] + b"\x80" + raw[24 + 101:]) == IO, "an entry of P that is -128"
    assert _read_embedding_rc(str(tmp_path / "absent.bin")) == IO
    with pytest.raises(hesaff_amd.HesaffError) as e:
        hesaff_amd.read_embedding(str(tmp_path / "absent.bin"))
    assert e.value.code == IO
    # the writer refuses what the reader would
    L = hesaff_amd.load_library()
    bad = P.copy(); bad[63, 127] = -128
    out = os.fsencode(str(tmp_path / "never.bin"))
    assert L.hesaff_write_embedding(out, 33, bad.ctypes.data, tau.ctypes.data) == ARG
    assert L.hesaff_write_embedding(out, 0, P.ctypes.data, tau.ctypes.data) == ARG and L.hesaff_write_embedding(out, (1 << 20) + 1, P.ctypes.data, tau.ctypes.data) == ARG
    assert L.hesaff_write_embedding(None, 33, P.ctypes.data, tau.ctypes.data) == ARG and L.hesaff_write_embedding(out, 33, None, tau.ctypes.data) == ARG
    assert L.hesaff_write_embedding(out, 33, P.ctypes.data, None) == ARG and not os.path.exists(out)
    with pytest.raises(ValueError):
        hesaff_amd.write_embedding(str(tmp_path / "never.bin"), bad, tau)
    assert L.hesaff_read_embedding(None, None, None, None) == ARG


@pytest.mark.parametrize("n", [0, 1, 221])
def test_signatures_file_round_trip(tmp_path, n):
    rng = np.random.RandomState(n)
    sigs = rng.randint(0, 1 << 32, n).astype(np.uint64) << np.uint64(32) | rng.randint(0, 1 << 32, n).astype(np.uint64)
    if n:
        sigs[0], sigs[-1] = np.uint64(0), np.uint64((1 << 64) - 1)
    path = str(tmp_path / "a.hesaff.sigs")
    hesaff_amd.write_signatures(path, sigs)
    raw = open(path, "rb").read()
    assert raw[:8] == b"HESAFFS1" and np.frombuffer(raw[8:16], "<u4").tolist() == [64, n] and raw[16:] == sigs.astype("<u8").tobytes()
    back = hesaff_amd.read_signatures(path)
    assert back.dtype == np.uint64 and np.array_equal(back, sigs)
    assert hesaff_amd.load_library().hesaff_signatures_is_complete(os.fsencode(path)) == n


def test_signatures_file_refusals(tmp_path):
    sigs = np.arange(5, dtype=np.uint64) * np.uint64(0x0123456789ABCDEF)
    path = str(tmp_path / "a.sigs")
    hesaff_amd.write_signatures(path, sigs)
    raw = open(path, "rb").read()
    L = hesaff_amd.load_library()

    def rc_of(data):
        q = str(tmp_path / "bad.sigs")
        open(q, "wb").write(data)
        rc = _read_signatures_rc(q)
        assert (L.hesaff_signatures_is_complete(os.fsencode(q)) >= 0) == (rc == 0)
        return rc
    u32 = lambda v: np.array([v], "<u4").tobytes()
    assert rc_of(raw) == 0
    assert rc_of(raw[:-1]) == IO and rc_of(raw[:16]) == IO and rc_of(raw[:9]) == IO and rc_of(b"") == IO and rc_of(raw + b"\0" * 8) == IO, "truncated or too long"
    assert rc_of(b"HESAFFW1" + raw[8:]) == IO, "a wrong magic"
    assert rc_of(raw[:8] + u32(32) + raw[12:]) == IO, "wrong bits"
    assert rc_of(raw[:12] + u32(4) + raw[16:]) == IO and rc_of(raw[:12] + u32(6) + raw[16:]) == IO and rc_of(raw[:12] + u32(0xFFFFFFFF) + raw[16:]) == IO, "count against size"
    assert _read_signatures_rc(str(tmp_path / "absent.sigs")) == IO and L.hesaff_signatures_is_complete(os.fsencode(str(tmp_path / "absent.sigs"))) == -1
    assert L.hesaff_read_signatures(None, None, None) == ARG and L.hesaff_signatures_is_complete(None) == -1
    out = os.fsencode(str(tmp_path / "never.sigs"))
    assert L.hesaff_write_signatures(out, None, 3) == ARG and L.hesaff_write_signatures(out, sigs.ctypes.data, -1) == ARG and L.hesaff_write_signatures(None, sigs.ctypes.data, 1) == ARG
    assert not os.path.exists(out)


# ---------------------------------------------------------------- refusals that need no device

def test_refusals_without_a_context():
    """every entry point refuses a NULL context before it touches a device"""
    L = hesaff_amd.load_library()
    P = hesaff_amd.embedding_projection(0)
    tau = np.zeros((1, 64), np.int32)
    one = np.zeros(1, np.int32); sig = np.zeros(1, np.uint64); desc = np.zeros((1, 128), np.uint8); z = np.zeros((1, 64), np.int32)
    im = np.zeros(1, np.int32); sc = np.zeros(1, np.float64); n = C.c_int(); k = C.c_int(); p = C.c_void_p(); t = C.c_int64()
    f = [C.c_float() for _ in range(4)]
    assert L.hesaff_set_embedding(None, P.ctypes.data, tau.ctypes.data) == ARG
    assert L.hesaff_get_embedding(None, C.byref(k), None, None) == ARG
    assert L.hesaff_get_signatures(None, 0, C.byref(p), C.byref(n)) == ARG
    assert L.hesaff_get_signatures_device(None, C.byref(p), C.byref(t)) == ARG
    assert L.hesaff_embed_device(None, 0, None, 128, 0, None, 1, None) == ARG
    assert L.hesaff_stage_embed(None, 1, desc.ctypes.data, one.ctypes.data, 1, sig.ctypes.data) == ARG
    assert L.hesaff_stage_project(None, 1, desc.ctypes.data, P.ctypes.data, z.ctypes.data) == ARG
    assert L.hesaff_train_embedding(None, 1, desc.ctypes.data, one.ctypes.data, 1, 1, P.ctypes.data, tau.ctypes.data, None) == ARG
    assert L.hesaff_train_embedding_device(None, 1, desc.ctypes.data, 128, 0, one.ctypes.data, 1, 1, P.ctypes.data, tau.ctypes.data, None) == ARG
    assert L.hesaff_get_embedding_ms(None, *[C.byref(x) for x in f]) == ARG
    assert L.hesaff_index_build_embedded(None, 1, one.ctypes.data, one.ctypes.data, 1, sig.ctypes.data, 1) == ARG
    assert L.hesaff_index_build_embedded_device(None, 1, one.ctypes.data, None, 1, None, 1) == ARG
    assert L.hesaff_index_query_embedded(None, 1, one.ctypes.data, 1, sig.ctypes.data, 64, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)) == ARG
    assert L.hesaff_index_query_embedded_device(None, 0, None, 1, None, 64, 1, im.ctypes.data, sc.ctypes.data, C.byref(n)) == ARG
    assert L.hesaff_index_get_embedded(None, C.byref(n), None, None, None) == ARG


def test_binding_refuses_malformed_arrays_before_the_library():
    P = hesaff_amd.embedding_projection(0)
    for bad in (P.astype(np.int16), P[:63], P.T, np.where(P == P[0, 0], np.int8(-128), P)):
        with pytest.raises(ValueError):
            _binding._projection_array(np.ascontiguousarray(bad))
    for bad in (np.zeros((3, 63), np.int32), np.zeros((3, 64), np.int64), np.zeros(64, np.int32)):
        with pytest.raises(ValueError):
            _binding._thresholds_array(bad)
    with pytest.raises(ValueError):
        _binding._thresholds_array(np.zeros((3, 64), np.int32), 4)
    with pytest.raises(ValueError):
        _binding._signature_array(np.zeros(3, np.uint64), 4)


# ---------------------------------------------------------------- the reference's own consequences

def _collection(seed, n_images=6, k=11, bits_kept=3):
    """images of words with signatures that differ in few bits, so that every threshold of a sweep changes something"""
    rng = np.random.RandomState(seed)
    images, sigs = [], []
    for i in range(n_images):
        n = 0 if i == 2 else int(rng.randint(1, 30))
        images.append(rng.randint(0, k, n).astype(np.int32))
        flips = rng.randint(0, 64, (n, bits_kept + i))
        g = np.zeros(n, np.uint64)
        for col in flips.T:
            g ^= np.uint64(1) << col.astype(np.uint64)
        sigs.append(g)
    return images, sigs, k


def test_reference_threshold_64_is_the_plain_query():
    images, sigs, k = _collection(1)
    index = R.build(images, k)
    rng = np.random.RandomState(2)
    for q in (0, 1, 3):
        qw = images[q] if q else rng.randint(0, k, 25).astype(np.int32)
        qs = sigs[q] if q else rng.randint(0, 1 << 31, 25).astype(np.uint64)
        want = R.query(index, qw, 4)
        got = E.query(index, images, sigs, qw, qs, 64, 4)
        assert got[0].tolist() == want[0].tolist() and got[4] == want[4]
        assert np.array_equal(got[2], want[2]) and np.array_equal(got[1].view(np.uint64), want[1].view(np.uint64))
        assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64))


def test_reference_dot_never_decreases_with_the_threshold():
    images, sigs, k = _collection(3)
    index = R.build(images, k)
    qw, qs = images[1], sigs[1] ^ np.uint64(5)
    last = None
    grew = 0
    for T in range(65):
        dot = E.query(index, images, sigs, qw, qs, T, 3)[2]
        if last is not None:
            assert (dot >= last).all(), T
            grew += int((dot > last).any())
        last = dot
    assert grew >= 3, "the sweep meets several thresholds that admit more pairs"
    assert E.query(index, images, sigs, qw, qs, 0, 3)[2].sum() < last.sum()


def test_reference_signature_and_median_definitions():
    """bit i is a STRICT compare against tau[word][i]; the lower median of m values is element (m - 1) // 2"""
    P = np.zeros((64, 128), np.int8)
    P[np.arange(64), np.arange(64)] = 1   # z[i] = d[i]
    d = np.arange(128, dtype=np.uint8)[None, :] + 10
    tau = np.zeros((2, 64), np.int32)
    tau[1] = np.arange(64) + 10       # equal: no bit set
    tau[0] = np.arange(64) + 9        # one below: every bit set
    assert int(E.signatures(P, tau, d, [1])[0]) == 0 and int(E.signatures(P, tau, d, [0])[0]) == (1 << 64) - 1
    desc = np.zeros((5, 128), np.uint8)
    desc[:, 0] = [9, 1, 7, 3, 5]
    t, c = E.thresholds(P, desc, [0, 0, 0, 0, 1], 3)
    assert t[0, 0] == 3 and t[1, 0] == 5 and t[2].tolist() == [0] * 64 and c.tolist() == [4, 1, 0]   # sorted 1 3 7 9: element 1
    assert E.popcount(np.array([0, 1, (1 << 64) - 1], np.uint64)).tolist() == [0, 1, 64]
