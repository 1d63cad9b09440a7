"""GPU suite of visual-word assignment (hesaff_set_vocabulary, include/hesaff_amd.h; k_assign_words, kernels_words.h).  The reference is
tests/vocabulary_ref.py: int64 differences and argmin in numpy.  Every comparison is bit for bit - the word, whose ties the reference
alone decides, and the distance."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import FROM_SHAPES, OUT_BIN, OUT_WORDS, _binding
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
E2E_IMAGES = ["band_160x120", "band_96x96", "band_160x120", "tiny_20x15", "band_96x96"]
E2E_KEYS = [221, 74, 221, 0, 74]

_ref = {}


def reference(desc, vocab, tag):
    """V.assign, computed once per tagged (desc, vocab) pair"""
    if tag not in _ref:
        _ref[tag] = V.assign(desc, vocab)
        _ref[tag].setflags(write=False)
    return _ref[tag]


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _same_rows(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d rows differ, first %s: got %s, want %s" % (what, len(bad), len(want), bad[:6].tolist(),
                                                                                  got[bad[:3]].tolist(), want[bad[:3]].tolist())


@pytest.fixture(scope="module")
def vctx():
    """a context of its own with max_batch = 2 (the session's context keeps no vocabulary)"""
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        assert c.vocabulary_size == 0
        yield c
        c.set_vocabulary(None)


@pytest.fixture(scope="module")
def e2e(vctx):
    """the five images, their keys without a vocabulary, and the vocabulary of the end-to-end tests: 150 rows of the images' own
    descriptors (those keys then have dist2 0) among 150 random rows"""
    vctx.set_vocabulary(None)
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    plain = vctx.detect_batch(imgs)
    assert [len(k) for _, k in plain] == E2E_KEYS
    own = np.concatenate([plain[0][1]["desc"], plain[1][1]["desc"]])
    rng = np.random.RandomState(77)
    vocab = rng.randint(0, 256, (300, 128)).astype(np.uint8)
    vocab[rng.permutation(300)[:150]] = own[rng.permutation(len(own))[:150]]
    want = [reference(k["desc"], vocab, "e2e%d" % i) for i, (_, k) in enumerate(plain)]
    assert (want[0][:, 1] == 0).sum() >= 50 and (want[0][:, 1] > 0).sum() >= 50
    return imgs, plain, vocab, want


# ---------------------------------------------------------------- the stage operator

@pytest.mark.gpu
@pytest.mark.parametrize("family", V.FAMILIES)
def test_stage_key_counts(vctx, family):
    """n in {0, 1, 3, 31, 32, 33, 64, 65, 257} against K in {33, 4099}: the tails of a key tile, of a wavefront's 64 keys and of a block's
    256, one word tile with a tail and 129 of them"""
    for K in (33, 4099):
        vocab = V.family(family, K, seed=100 + K)
        desc = V.family(family, 257, seed=7)
        want = reference(desc, vocab, ("counts", family, K))
        vctx.set_vocabulary(vocab)
        assert vctx.vocabulary_size == K
        for n in (0, 1, 3, 31, 32, 33, 64, 65, 257):
            _same_rows(vctx.assign_words(desc[:n]), want[:n], "%s, K = %d, n = %d" % (family, K, n))


@pytest.mark.gpu
@pytest.mark.parametrize("family", V.FAMILIES)
def test_stage_vocabulary_sizes(vctx, family):
    """K in {1, 2, 31, 32, 33, 63, 64, 65, 257, 4099} against n in {65, 257}: tile tails on both sides of 32 and 64.  The binary
    families hold tied minima (bytes in {0, 255} at K = 257: dozens of the keys); the reference alone decides them"""
    desc = V.family(family, 257, seed=8)
    full = V.family(family, 4099, seed=9)
    for K in (1, 2, 31, 32, 33, 63, 64, 65, 257, 4099):
        vocab = np.ascontiguousarray(full[:K])
        want = reference(desc, vocab, ("sizes", family, K))
        vctx.set_vocabulary(vocab)
        for n in (65, 257):
            _same_rows(vctx.assign_words(desc[:n]), want[:n], "%s, K = %d, n = %d" % (family, K, n))
        assert (want[:, 0] < K).all()


@pytest.mark.gpu
def test_stage_constructed_rows(vctx):
    """K = 4099 with rows placed by hand: both ends of the value range, duplicates in the same tile, in a later tile and 100 tiles on,
    and two words at the same distance from a key"""
    vocab = V.family("uniform", 4099, seed=21)
    desc = V.family("uniform", 70, seed=22)
    vocab[7] = 0
    vocab[9] = 255
    vocab[40] = vocab[5]
    vocab[5 + 32 * 100] = vocab[5]
    vocab[1000] = 9
    vocab[2000] = 11
    desc[0] = 0
    desc[1] = 255
    desc[2] = vocab[5]
    desc[3] = 10
    want = V.assign(desc, vocab)
    assert want[0].tolist() == [7, 0] and want[1].tolist() == [9, 0] and want[2].tolist() == [5, 0] and want[3].tolist() == [1000, 128]
    vctx.set_vocabulary(vocab)
    _same_rows(vctx.assign_words(desc), want, "constructed rows")
    # the later word first: the earlier ROW still wins
    vocab[1000], vocab[2000] = 11, 9
    vctx.set_vocabulary(vocab)
    assert vctx.assign_words(desc[3:4]).tolist() == [[1000, 128]]
    # K = 1: the largest distance there is
    vctx.set_vocabulary(np.full((1, 128), 255, np.uint8))
    assert vctx.assign_words(np.zeros((1, 128), np.uint8)).tolist() == [[0, 8323200]]
    vctx.set_vocabulary(np.zeros((1, 128), np.uint8))
    assert vctx.assign_words(np.full((2, 128), 255, np.uint8)).tolist() == [[0, 8323200]] * 2


@pytest.mark.gpu
def test_stage_all_at_once_and_one_per_call(vctx):
    vocab = V.family("uniform", 4099, seed=100 + 4099)
    desc = V.family("uniform", 257, seed=7)
    want = reference(desc, vocab, ("counts", "uniform", 4099))
    vctx.set_vocabulary(vocab)
    _same_rows(vctx.assign_words(desc), want, "all at once")
    single = np.concatenate([vctx.assign_words(desc[i:i + 1]) for i in range(257)])
    _same_rows(single, want, "one key per call")


@pytest.mark.gpu
def test_stage_asymmetric_rows_pin_the_accumulator_map(vctx):
    """key i = byte i at position i mod 128, zero elsewhere; word k = byte 3k + 1 (mod 256) at position k mod 128: which (key, word)
    pair an accumulator element belongs to decides nearly every answer, so a row / column swap or a shifted tile cannot pass"""
    n, K = 200, 300
    desc = np.zeros((n, 128), np.uint8)
    desc[np.arange(n), np.arange(n) % 128] = np.arange(n) % 256
    vocab = np.zeros((K, 128), np.uint8)
    vocab[np.arange(K), np.arange(K) % 128] = (3 * np.arange(K) + 1) % 256
    want = V.assign(desc, vocab)
    swapped, shifted = V.assign(vocab[:n], desc), V.assign(desc, np.roll(vocab, 32, axis=0))
    assert len(np.unique(want[:, 0])) > 60 and (want != swapped).any(axis=1).mean() > 0.4 and (want[:, 0] != shifted[:, 0]).mean() > 0.9
    vctx.set_vocabulary(vocab)
    _same_rows(vctx.assign_words(desc), want, "asymmetric rows")


# ---------------------------------------------------------------- strided source in device memory

@pytest.mark.gpu
def test_strided_and_packed_device_sources(vctx):
    """hesaff_assign_words_device on a [65, 164] tensor (descriptor 36 bytes in, the other bytes 0xFF: they must not be read as
    descriptor) and on the packed [65, 128] tensor: the rows of the stage operator, which are the reference's"""
    import torch
    vocab = V.family("uniform", 4099, seed=100 + 4099)
    desc = V.family("uniform", 257, seed=7)[:65]
    want = reference(V.family("uniform", 257, seed=7), vocab, ("counts", "uniform", 4099))[:65]
    vctx.set_vocabulary(vocab)
    rec = np.full((65, 164), 0xFF, np.uint8)
    rec[:, 36:] = desc
    for src, stride, offset in ((rec, 164, 36), (desc, 128, 0)):
        t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        out = torch.full((65, 2), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        vctx.assign_words_device(t.data_ptr(), 65, stride, offset, out.data_ptr())
        _same_rows(out.cpu().numpy(), want, "stride %d" % stride)
    _same_rows(vctx.assign_words(desc), want, "packed host run")


# ---------------------------------------------------------------- vocabulary state

@pytest.mark.gpu
def test_vocabulary_state_follows_every_set(vctx, e2e):
    imgs, plain, _, _ = e2e
    desc = V.family("uniform", 65, seed=31)
    big, small = V.family("uniform", 300, seed=32), V.family("uniform", 33, seed=33)
    for K, vocab in ((300, big), (33, small), (300, big)):
        vctx.set_vocabulary(vocab)
        assert vctx.vocabulary_size == K
        _same_rows(vctx.assign_words(desc), reference(desc, vocab, ("state", K)), "K = %d" % K)
    (nh, keys), = vctx.detect_batch(imgs[1:2])
    _same_rows(vctx.words(0), reference(keys["desc"], big, "state e2e"), "words after detect_batch")
    assert nh == plain[1][0] and keys.tobytes() == plain[1][1].tobytes()   # the keys do not change by a bit
    vctx.set_vocabulary(None)
    assert vctx.vocabulary_size == 0
    with pytest.raises(hesaff_amd.HesaffError):
        vctx.words(0)
    (nh, keys), = vctx.detect_batch(imgs[1:2])
    assert keys.tobytes() == plain[1][1].tobytes()
    with pytest.raises(hesaff_amd.HesaffError):
        vctx.words(0)


# ---------------------------------------------------------------- end to end

def _check_images(vctx, results, e2e, what):
    imgs, plain, vocab, want = e2e
    for i, ((_, keys), (nh, pk)) in enumerate(zip(results, plain)):
        assert keys.tobytes() == pk.tobytes(), "%s: keys of image %d" % (what, i)
        got = vctx.words(i)
        assert len(got) == E2E_KEYS[i]
        _same_rows(got, want[i], "%s: image %d" % (what, i))
    with pytest.raises(hesaff_amd.HesaffError):
        vctx.words(len(imgs))
    with pytest.raises(hesaff_amd.HesaffError):
        vctx.words(-1)


@pytest.mark.gpu
def test_end_to_end_detect_batch(vctx, e2e):
    """five images of two sizes interleaved, max_batch = 2: the regrouping by geometry and a chunk boundary both lie between the
    caller's indices.  words(i) is the reference on keys of image i; the image without keys has count 0 and a NULL pointer"""
    imgs, plain, vocab, want = e2e
    vctx.set_vocabulary(vocab)
    res = vctx.detect_batch(imgs)
    _check_images(vctx, res, e2e, "detect_batch")
    p = ctypes.c_void_p(1); n = ctypes.c_int(-1)
    assert vctx.L.hesaff_get_words(vctx.h, 3, ctypes.byref(p), ctypes.byref(n)) == 0 and n.value == 0 and p.value is None


@pytest.mark.gpu
def test_end_to_end_other_host_entry_points(vctx, e2e):
    imgs, plain, vocab, want = e2e
    vctx.set_vocabulary(vocab)
    regions = vctx.detect_regions(imgs)
    _check_images(vctx, [(len(r), k) for r, k in regions], e2e, "detect_regions")
    _check_images(vctx, vctx.detect_batch_f32([im.astype(np.float32) for im in imgs]), e2e, "detect_batch_f32")
    shapes = [r[r["outcome"] >= 1] for r, _ in regions]
    described = vctx.describe_regions(imgs, shapes, FROM_SHAPES)
    _check_images(vctx, [(len(r), k) for r, k in described], e2e, "describe_regions")


@pytest.mark.gpu
def test_end_to_end_callback(vctx, e2e):
    """detect_batch_cb: the getter is called inside the sink, for the images of the chunk being delivered; afterwards the rows are gone"""
    imgs, plain, vocab, want = e2e
    vctx.set_vocabulary(vocab)
    seen = {}

    def sink(indices, out):
        for i, (nh, keys) in zip(indices, out):
            assert keys.tobytes() == plain[i][1].tobytes()
            seen[i] = vctx.words(i)
        return 0
    vctx.detect_batch_cb(imgs, sink)
    assert sorted(seen) == [0, 1, 2, 3, 4]
    for i in range(5):
        _same_rows(seen[i], want[i], "sink: image %d" % i)
    with pytest.raises(hesaff_amd.HesaffError):
        vctx.words(0)


@pytest.mark.gpu
def test_end_to_end_device_resident(e2e):
    import torch
    from tests.test_gpu_parity import _device_keys
    imgs, plain, vocab, want = e2e
    img = imgs[0]
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_vocabulary(vocab)
        with pytest.raises(hesaff_amd.HesaffError):
            c.words_device()
        t = torch.from_numpy(np.stack([img] * 3)).cuda()
        torch.cuda.synchronize()
        ch, cd, dkeys, total = c.detect_batch_device(t.data_ptr(), 3, img.shape[1], img.shape[0])
        assert cd.tolist() == [221] * 3 and total == 663
        keys = _device_keys(dkeys, total)
        ptr, rows = c.words_device()
        assert rows == total
        got = torch.empty((total, 2), dtype=torch.int32, device="cuda")
        hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
        assert hip.hipMemcpy(ctypes.c_void_p(got.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(total * 8), 3) == 0
        got = got.cpu().numpy()
        for b in range(3):
            assert keys[221 * b:221 * (b + 1)].tobytes() == plain[0][1].tobytes()
            _same_rows(got[221 * b:221 * (b + 1)], want[0], "device-resident, image %d" % b)
        # the key array itself as a strided source
        out = torch.full((total, 2), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c.assign_words_device(dkeys, total, 164, 36, out.data_ptr())
        assert np.array_equal(out.cpu().numpy(), got)
        with pytest.raises(hesaff_amd.HesaffError):
            c.words(0)   # the last call was not a host call


@pytest.mark.gpu
def test_end_to_end_with_orientation_peaks_and_rootsift(e2e):
    """dominant orientation, two keys per region, RootSIFT bytes: one row per KEY, the reference on those keys' bytes"""
    imgs, plain, vocab, _ = e2e
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        c.set_orientation("dominant")
        c.set_orientation_count(2)
        c.set_descriptor("rootsift")
        base = c.detect_batch(imgs)
        c.set_vocabulary(vocab)
        res = c.detect_batch(imgs)
        assert len(res[0][1]) > 100 and (res[0][1]["a12"] != 0).any()   # turned frames
        for i, ((nh, keys), (_, bk)) in enumerate(zip(res, base)):
            assert keys.tobytes() == bk.tobytes()
            got = c.words(i)
            assert len(got) == len(keys)
            _same_rows(got, reference(keys["desc"], vocab, "peaks%d" % i), "peaks + rootsift: image %d" % i)


# ---------------------------------------------------------------- files, CLI, C++

def _copies(tmp_path):
    paths = []
    for j, n in enumerate(E2E_IMAGES):
        paths.append(str(tmp_path / ("%d_%s.pgm" % (j, n))))
        shutil.copyfile(os.path.join(GOLD, n + ".pgm"), paths[-1])
    return paths


def _want_words_file(bin_path, want, K):
    rows = hesaff_amd.read_bin(bin_path)
    xyabc = np.stack([rows[f] for f in ("x", "y", "a", "b", "c")], axis=1) if len(rows) else np.zeros((0, 5), np.float32)
    return V.words_file(xyabc, want, K)


@pytest.mark.gpu
def test_process_files_writes_words_files(vctx, e2e, tmp_path):
    imgs, plain, vocab, want = e2e
    paths = _copies(tmp_path)
    vctx.set_vocabulary(vocab)
    vctx.set_output_format(OUT_BIN | OUT_WORDS)
    try:
        st = vctx.process_files(paths)
        expect = []
        for i, (p, s) in enumerate(zip(paths, st)):
            assert s[0] == 0 and s[3] == E2E_KEYS[i], (p, s)
            assert not os.path.exists(p + ".hesaff.sift")
            expect.append(_want_words_file(p + ".hesaff.bin", want[i], 300))
            assert open(p + ".hesaff.words", "rb").read() == expect[i], p
            vs, rows = hesaff_amd.read_words(p + ".hesaff.words")
            assert vs == 300 and np.array_equal(rows["word"], want[i][:, 0].astype(np.uint32))
        # the words file alone, under the caller's names
        vctx.set_output_format(OUT_WORDS)
        outs = [str(tmp_path / ("out%d" % i)) for i in range(5)]
        st = vctx.process_files(paths, outs)
        for i, o in enumerate(outs):
            assert st[i][0] == 0 and open(o, "rb").read() == expect[i]
            assert not os.path.exists(o + ".words") and not os.path.exists(o + ".bin")
        # combined, under the caller's names: ".words" appended
        vctx.set_output_format(OUT_BIN | OUT_WORDS)
        outs2 = [str(tmp_path / ("both%d" % i)) for i in range(5)]
        st = vctx.process_files(paths, outs2)
        for i, o in enumerate(outs2):
            assert st[i][0] == 0 and open(o + ".words", "rb").read() == expect[i]
            assert open(o, "rb").read() == open(paths[i] + ".hesaff.bin", "rb").read()
        # resume: complete outputs are skipped, a missing or cut words file is made again
        os.remove(paths[1] + ".hesaff.words")
        with open(paths[2] + ".hesaff.words", "r+b") as f:
            f.truncate(16 + 24 * 100 + 5)
        vctx.set_resume(True)
        st = vctx.process_files(paths)
        assert [s[1] for s in st] == [5, 3, 3, 5, 5], st   # HESAFF_FILE_SKIPPED, HESAFF_FILE_WRITTEN
        assert [s[3] for s in st] == E2E_KEYS
        for i, p in enumerate(paths):
            assert open(p + ".hesaff.words", "rb").read() == expect[i]
    finally:
        vctx.set_resume(False)
        vctx.set_output_format(1)


@pytest.mark.gpu
def test_cli_writes_words_files(e2e, tmp_path):
    imgs, plain, vocab, want = e2e
    paths = _copies(tmp_path)
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    mr = hesaff_amd.default_params().mrSize
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")

    def expected(i):
        ref = str(tmp_path / "ref.bin")
        hesaff_amd.write_bin(ref, plain[i][1], mr)
        return _want_words_file(ref, want[i], 300)
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for i, p in enumerate(paths):
        assert open(p + ".hesaff.words", "rb").read() == expected(i), p
        assert open(p + ".hesaff.sift", "rb").read() == hesaff_amd.format_sift(plain[i][1], mr)
        os.remove(p + ".hesaff.words"); os.remove(p + ".hesaff.sift")
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile, "--words-only"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for i, p in enumerate(paths):
        assert open(p + ".hesaff.words", "rb").read() == expected(i), p
        assert not os.path.exists(p + ".hesaff.sift")
        os.remove(p + ".hesaff.words")
    r = subprocess.run([EXE, paths[0], "--vocabulary", vfile], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(paths[0] + ".hesaff.words", "rb").read() == expected(0)
    assert open(paths[0] + ".hesaff.sift", "rb").read() == hesaff_amd.format_sift(plain[0][1], mr)
    vs, rows = hesaff_amd.read_words(paths[0] + ".hesaff.words")
    assert vs == 300 and len(rows) == 221


@pytest.mark.gpu
def test_cpp_detector_with_vocabulary(e2e, tmp_path):
    """tests/native/vocabulary_keys.cpp: setVocabulary, words() and exportWords through hesaff.hpp hold what the Python path holds"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, plain, vocab, want = e2e
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    exe = str(tmp_path / "vocabulary_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "vocabulary_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    out = str(tmp_path / "cpp.words")
    r = subprocess.run([exe, vfile, os.path.join(GOLD, "band_96x96.pgm"), out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    nh, keys = plain[1]
    assert lines[0] == "N %d %d 1" % (nh, len(keys)), lines[0]
    assert lines[1:] == ["W %d %d %s" % (w[0], w[1], k.tobytes().hex()) for w, k in zip(want[1], keys)]
    py = str(tmp_path / "py.words")
    hesaff_amd.write_words(py, keys, want[1], hesaff_amd.default_params().mrSize, 300)
    assert open(out, "rb").read() == open(py, "rb").read()


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_leave_the_context_usable(vctx, e2e):
    imgs, plain, vocab, want = e2e
    L, h = vctx.L, vctx.h
    vctx.set_vocabulary(vocab)
    k = ctypes.c_int(); p = ctypes.c_void_p(); n = ctypes.c_int(); tot = ctypes.c_int64(); ms = ctypes.c_float()
    desc = np.ascontiguousarray(plain[1][1]["desc"])
    out = np.zeros((len(desc), 2), np.int32)

    def still_works():
        assert vctx.vocabulary_size == 300
        (nh, keys), = vctx.detect_batch(imgs[1:2])
        assert keys.tobytes() == plain[1][1].tobytes()
        _same_rows(vctx.words(0), want[1], "after a refusal")
    ARG = -2
    # the vocabulary itself
    assert L.hesaff_set_vocabulary(h, -1, vocab.ctypes.data) == ARG
    assert L.hesaff_set_vocabulary(h, (1 << 20) + 1, vocab.ctypes.data) == ARG
    assert L.hesaff_set_vocabulary(h, 5, None) == ARG
    for bad in (vocab.astype(np.int32), vocab[:, :64], vocab[::2], vocab.T, np.zeros((0, 128), np.uint8), vocab.tolist()):
        with pytest.raises(ValueError):
            vctx.set_vocabulary(bad)
    still_works()
    # getters' out pointers
    assert L.hesaff_get_vocabulary_size(h, None) == ARG
    assert L.hesaff_get_words(h, 0, None, ctypes.byref(n)) == ARG and L.hesaff_get_words(h, 0, ctypes.byref(p), None) == ARG
    assert L.hesaff_get_words_device(h, None, ctypes.byref(tot)) == ARG and L.hesaff_get_words_device(h, ctypes.byref(p), None) == ARG
    assert L.hesaff_get_assign_ms(h, None) == ARG
    # images outside the last call's
    assert L.hesaff_get_words(h, 1, ctypes.byref(p), ctypes.byref(n)) == ARG
    assert L.hesaff_get_words(h, -1, ctypes.byref(p), ctypes.byref(n)) == ARG
    assert L.hesaff_get_words_device(h, ctypes.byref(p), ctypes.byref(tot)) == ARG   # the last call was a host call
    # strides and offsets (checked before any pointer is touched)
    import torch
    t = torch.zeros((4, 164), dtype=torch.uint8, device="cuda")
    o = torch.zeros((4, 2), dtype=torch.int32, device="cuda")
    for stride, offset in ((127, 0), (124, 0), (164, -4), (164, 40), (128, 4), (166, 36), (164, 38), (164, 37)):
        assert L.hesaff_assign_words_device(h, 4, ctypes.c_void_p(t.data_ptr()), stride, offset, ctypes.c_void_p(o.data_ptr())) == ARG, (stride, offset)
    assert L.hesaff_assign_words_device(h, -1, ctypes.c_void_p(t.data_ptr()), 164, 36, ctypes.c_void_p(o.data_ptr())) == ARG
    assert L.hesaff_assign_words_device(h, 4, None, 164, 36, ctypes.c_void_p(o.data_ptr())) == ARG
    assert L.hesaff_assign_words_device(h, 4, ctypes.c_void_p(t.data_ptr()), 164, 36, None) == ARG
    assert L.hesaff_stage_assign_words(h, -1, desc.ctypes.data, out.ctypes.data) == ARG
    assert L.hesaff_stage_assign_words(h, 4, None, out.ctypes.data) == ARG and L.hesaff_stage_assign_words(h, 4, desc.ctypes.data, None) == ARG
    assert int(o.cpu().abs().sum()) == 0
    still_works()
    # everything that needs a vocabulary, without one
    vctx.set_vocabulary(None)
    try:
        assert L.hesaff_get_words(h, 0, ctypes.byref(p), ctypes.byref(n)) == ARG
        assert L.hesaff_get_words_device(h, ctypes.byref(p), ctypes.byref(tot)) == ARG
        assert L.hesaff_assign_words_device(h, 4, ctypes.c_void_p(t.data_ptr()), 164, 36, ctypes.c_void_p(o.data_ptr())) == ARG
        assert L.hesaff_stage_assign_words(h, len(desc), desc.ctypes.data, out.ctypes.data) == ARG and not out.any()
        assert L.hesaff_get_assign_ms(h, ctypes.byref(ms)) == 0 and ms.value == 0.0
        vctx.set_output_format(OUT_WORDS)
        st = (_binding.FileStatus * 1)()
        path = (ctypes.c_char_p * 1)(os.fsencode(os.path.join(GOLD, "band_96x96.pgm")))
        assert L.hesaff_process_files(h, 1, path, None, 0, 0, st) == ARG
        assert "vocabulary" in L.hesaff_last_error(h).decode()
        assert not os.path.exists(os.path.join(GOLD, "band_96x96.pgm.hesaff.words"))
    finally:
        vctx.set_output_format(1)
    (nh, keys), = vctx.detect_batch(imgs[1:2])
    assert keys.tobytes() == plain[1][1].tobytes()
    vctx.set_vocabulary(vocab)
    still_works()


@pytest.mark.gpu
def test_assign_ms_is_the_event_time_of_the_launch(vctx, e2e):
    imgs, plain, vocab, want = e2e
    vctx.set_vocabulary(vocab)
    vctx.set_profiling(0)
    vctx.detect_batch(imgs[:1])
    assert vctx.assign_ms == 0.0
    vctx.set_profiling(1)
    try:
        vctx.detect_batch(imgs[:1])
        ms = vctx.assign_ms
        print("assign_ms for 221 keys, K = 300: %.4f" % ms)
        assert 0.0 < ms < 1000.0
        vctx.detect_batch(imgs[3:4])   # no keys: no launch
        assert vctx.assign_ms == 0.0
    finally:
        vctx.set_profiling(0)
