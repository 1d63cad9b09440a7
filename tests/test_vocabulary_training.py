"""GPU suite of vocabulary training (hesaff_train_vocabulary, include/hesaff_amd.h; kernels_train.h).  The reference is
tests/vocabulary_training_ref.py: the definition in numpy.  Every comparison is bit for bit - rows, distortions, empty counts and the
number of iterations run."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from tests import vocabulary_ref as V
from tests import vocabulary_training_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
E2E_IMAGES = ["band_160x120", "band_96x96", "band_160x120", "tiny_20x15", "band_96x96"]
E2E_KEYS = [221, 74, 221, 0, 74]
ARG = -2

_ref = {}


def reference(tag, desc, k, iterations, init=None):
    """T.train, computed once per tag and left unchanged"""
    if tag not in _ref:
        _ref[tag] = T.train(desc, k, iterations, init)
        for a in _ref[tag]:
            a.setflags(write=False)
    return _ref[tag]


def _same(got, want, what):
    names = ("rows", "distortion", "empty")
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, g.shape, w.dtype, w.shape)
    assert got[1].tolist() == want[1].tolist(), (what, "distortion")
    assert got[2].tolist() == want[2].tolist(), (what, "empty")
    bad = np.nonzero((got[0] != want[0]).any(axis=1))[0]
    assert len(bad) == 0, "%s: %d of %d rows differ, first %s" % (what, len(bad), len(want[0]), bad[:8].tolist())


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def tctx():
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        yield c


@pytest.fixture(scope="module")
def e2e(tctx):
    """the five images and their keys (no vocabulary set)"""
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    plain = tctx.detect_batch(imgs)
    assert [len(k) for _, k in plain] == E2E_KEYS
    keys = np.concatenate([k for _, k in plain])
    return imgs, plain, keys


# ---------------------------------------------------------------- the accumulation operator

def _check_accumulate(tctx, desc, words, K, what):
    sums, counts = tctx.accumulate_words(desc, words, K)
    want_s, want_c = T.accumulate(desc, words, K)
    assert sums.dtype == np.uint32 and sums.shape == (K, 128) and counts.dtype == np.uint32 and counts.shape == (K,)
    assert counts.tolist() == want_c.tolist(), what
    bad = np.nonzero((sums != want_s).any(axis=1))[0]
    assert len(bad) == 0, "%s: sums of %d words differ, first %s" % (what, len(bad), bad[:8].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 2, 33, 1000, 4099])
def test_accumulate_shapes_and_word_patterns(tctx, K):
    """n in {1, 63, 64, 65, 257, 4099} - the tails of a half-wave's 32 positions, of a wave's 64 and of a block's 256; at 4099 a
    half-wave walks two chunks of 32 - against every word pattern: all keys in word 0, all in word K - 1, ascending, descending,
    shuffled, one key per word where n = K, and words that leave most rows empty.  K = 1, 2, 33: 64 sub-counters per word, K = 1000:
    8, K = 4099: one"""
    full = V.family("uniform", 4099, seed=51)
    rng = np.random.RandomState(52 + K)
    for n in (1, 63, 64, 65, 257, 4099):
        desc = full[:n]
        asc = (np.arange(n, dtype=np.int64) * K // n).astype(np.int32)
        few = np.array(sorted({0, K // 2, K - 1}), np.int32)
        patterns = {"word 0": np.zeros(n, np.int32), "word K-1": np.full(n, K - 1, np.int32), "ascending": asc, "descending": asc[::-1].copy(),
                    "shuffled": rng.randint(0, K, n).astype(np.int32), "mostly empty": few[rng.randint(0, len(few), n)]}
        if n == K:
            patterns["one key per word"] = np.arange(K, dtype=np.int32)
            patterns["one key per word, shuffled"] = rng.permutation(K).astype(np.int32)
        for name, words in patterns.items():
            _check_accumulate(tctx, desc, words, K, "n = %d, K = %d, %s" % (n, K, name))


@pytest.mark.gpu
def test_accumulate_largest_bytes_and_run_boundaries(tctx):
    """4099 keys of all-255 bytes in one word: 1 045 245 per column.  Runs that change word at positions 63, 64 and 65 (and 31, 32, 33:
    the half-waves'), between neighbouring words and between words 4000 rows apart, on the binary families' bytes too"""
    desc = np.full((4099, 128), 255, np.uint8)
    words = np.full(4099, 17, np.int32)
    sums, counts = tctx.accumulate_words(desc, words, 33)
    assert counts[17] == 4099 and counts.sum() == 4099 and (sums[17] == 1045245).all() and sums.sum() == 1045245 * 128
    # n = 16387: the longest walk, eight chunks of 32 positions per half-wave, with a tail
    big = V.family("uniform", 16387, seed=54)
    rng = np.random.RandomState(55)
    for K in (1, 33, 1000, 4099):
        _check_accumulate(tctx, big, rng.randint(0, K, 16387).astype(np.int32), K, "n = 16387, K = %d, shuffled" % K)
        _check_accumulate(tctx, big, (np.arange(16387, dtype=np.int64) * K // 16387).astype(np.int32), K, "n = 16387, K = %d, ascending" % K)
    for family in V.FAMILIES:
        d = V.family(family, 257, seed=53)
        for cut in (31, 32, 33, 63, 64, 65, 127, 128, 129):
            for a, b, K in ((0, 1, 2), (5, 6, 33), (3, 4003, 4099)):
                w = np.full(257, b, np.int32)
                w[:cut] = a
                _check_accumulate(tctx, d, w, K, "%s: words %d -> %d at position %d" % (family, a, b, cut))
                _check_accumulate(tctx, d[:cut + 1], w[:cut + 1], K, "%s: one key behind position %d" % (family, cut))


# ---------------------------------------------------------------- training

@pytest.mark.gpu
@pytest.mark.parametrize("family", V.FAMILIES)
def test_training_on_the_families(tctx, family):
    """n = 257, K in {1, 2, 33, 65}, T = 1 and T = 4.  K is no multiple of 32: from iteration 2 on the assignment runs on the vocabulary
    the device packed itself, pad rows included"""
    desc = V.family(family, 257, seed=41)
    for K in (1, 2, 33, 65):
        for iters in (1, 4):
            want = reference(("family", family, K, iters), desc, K, iters)
            _same(tctx.train_vocabulary(desc, K, iters), want, "%s, K = %d, T = %d" % (family, K, iters))


@pytest.mark.gpu
def test_training_with_more_words_than_keys(tctx):
    """K = 4099 with an explicit init and n = 257: most words are empty and keep their rows"""
    desc = V.family("uniform", 257, seed=41)
    init = V.family("uniform", 4099, seed=42)
    want = reference("more words", desc, 4099, 3, init)
    assert want[2][0] >= 4099 - 257
    got = tctx.train_vocabulary(desc, 4099, 3, init=init)
    _same(got, want, "K = 4099, n = 257")
    untouched = np.setdiff1d(np.arange(4099), V.assign(desc, init)[:, 0])
    assert len(untouched) >= 4099 - 257 and np.array_equal(got[0][untouched[:50]], init[untouched[:50]])


@pytest.mark.gpu
def test_training_on_the_clustered_set(tctx):
    """33 centres in 20 .. 235, noise +-12, n = 4099, K = 33, T = 10: the reference stops after 8 iterations with 2 words empty"""
    desc = T.clustered()
    want = reference("clustered", desc, 33, 10)
    assert len(want[1]) == 8 and want[2][-1] == 2
    _same(tctx.train_vocabulary(desc, 33, 10), want, "clustered")


@pytest.mark.gpu
def test_fixed_points(tctx):
    """5 distinct rows, each 13 times.  K = 5: the sampled rows are the five, so one iteration with distortion 0.  K = 7: two sampled
    rows are duplicates of lower ones, their words stay empty and keep the rows they were given"""
    rows = V.family("uniform", 5, seed=61)
    desc = np.tile(rows, (13, 1))
    words, dist, empty = tctx.train_vocabulary(desc, 5, 10)
    assert dist.tolist() == [0] and empty.tolist() == [0] and sorted(map(bytes, words)) == sorted(map(bytes, rows))
    _same((words, dist, empty), reference("fixed 5", desc, 5, 10), "K = 5")
    got = tctx.train_vocabulary(desc, 7, 10)
    _same(got, reference("fixed 7", desc, 7, 10), "K = 7")
    assert got[1].tolist() == [0] and got[2].tolist() == [2] and np.array_equal(got[0], T.sample(desc, 7))


@pytest.mark.gpu
def test_sampled_and_explicit_initial_rows_agree(tctx):
    desc = V.family("uniform", 257, seed=41)
    for K in (33, 257):
        a = tctx.train_vocabulary(desc, K, 3)
        b = tctx.train_vocabulary(desc, K, 3, init=T.sample(desc, K))
        _same(a, b, "K = %d" % K)
        _same(a, reference(("family", "uniform", K, 3), desc, K, 3), "K = %d against the reference" % K)


@pytest.mark.gpu
def test_host_and_device_sources_agree(tctx):
    """a packed [n, 128] tensor and a [n, 164] tensor with the descriptor 36 bytes in and 0xFF around it (never read as descriptor):
    the rows of the host form, which are the reference's"""
    import torch
    desc = V.family("uniform", 257, seed=41)
    want = reference(("family", "uniform", 33, 4), desc, 33, 4)
    _same(tctx.train_vocabulary(desc, 33, 4), want, "host")
    rec = np.full((257, 164), 0xFF, np.uint8)
    rec[:, 36:] = desc
    for src, stride, offset in ((desc, 128, 0), (rec, 164, 36)):
        t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        torch.cuda.synchronize()
        _same(tctx.train_vocabulary_device(t.data_ptr(), 257, stride, offset, 33, 4), want, "stride %d" % stride)
        init = V.family("uniform", 33, seed=43)
        _same(tctx.train_vocabulary_device(t.data_ptr(), 257, stride, offset, 33, 2, init=init), reference("dev init", desc, 33, 2, init), "stride %d, init" % stride)
        assert np.array_equal(t.cpu().numpy(), src)   # the source is only read


# ---------------------------------------------------------------- end to end

@pytest.mark.gpu
def test_end_to_end_on_the_keys_of_images(tctx, e2e):
    """the keys of the five interleaved images as a key array in device memory (stride 164, offset 36), K = 33, T = 3: the reference on
    the host keys.  Installed with set_vocabulary, the words of a detection are the reference's assignment under the trained rows"""
    import torch
    imgs, plain, keys = e2e
    desc = np.ascontiguousarray(keys["desc"])
    want = reference("e2e", desc, 33, 3)
    t = torch.from_numpy(np.frombuffer(keys.tobytes(), np.uint8).reshape(len(keys), 164).copy()).cuda()
    torch.cuda.synchronize()
    got = tctx.train_vocabulary_device(t.data_ptr(), len(keys), 164, 36, 33, 3)
    _same(got, want, "key array")
    assert tctx.vocabulary_size == 0   # training set nothing
    try:
        tctx.set_vocabulary(got[0])
        res = tctx.detect_batch(imgs)
        for i, ((_, k), (_, pk)) in enumerate(zip(res, plain)):
            assert k.tobytes() == pk.tobytes()
            assert np.array_equal(tctx.words(i), V.assign(pk["desc"], want[0])), "image %d" % i
    finally:
        tctx.set_vocabulary(None)


@pytest.mark.gpu
def test_end_to_end_device_resident_keys_in_place(e2e):
    """detect_batch_device leaves the keys on the device; training reads the descriptors where they are"""
    import torch
    from tests.test_gpu_parity import _device_keys
    imgs, plain, _ = e2e
    img = imgs[0]
    with hesaff_amd.HesaffContext(device=0) as c:
        t = torch.from_numpy(np.stack([img] * 3)).cuda()
        torch.cuda.synchronize()
        ch, cd, dkeys, total = c.detect_batch_device(t.data_ptr(), 3, img.shape[1], img.shape[0])
        assert total == 663
        keys = _device_keys(dkeys, total)
        got = c.train_vocabulary_device(dkeys, total, 164, 36, 33, 3)
        _same(got, reference("e2e resident", np.ascontiguousarray(keys["desc"]), 33, 3), "keys in place")
        assert _device_keys(dkeys, total).tobytes() == keys.tobytes()


@pytest.mark.gpu
def test_cli_trains_a_vocabulary(e2e, tmp_path):
    """hesaff --batch list --train-vocabulary vocab.bin --words 33 --iterations 3: the file's bytes are the reference's on the keys of
    the list in list order; one line per iteration on stdout; no per-image file"""
    imgs, plain, keys = e2e
    paths = []
    for j, n in enumerate(E2E_IMAGES):
        paths.append(str(tmp_path / ("%d_%s.pgm" % (j, n))))
        shutil.copyfile(os.path.join(GOLD, n + ".pgm"), paths[-1])
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    out = str(tmp_path / "vocab.bin")
    want = reference("e2e", np.ascontiguousarray(keys["desc"]), 33, 3)
    r = subprocess.run([EXE, "--batch", str(lst), "--train-vocabulary", out, "--words", "33", "--iterations", "3"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == V.vocabulary_file(want[0])
    lines = r.stdout.strip().split("\n")
    assert lines[:len(want[1])] == ["iteration %d: distortion %d, %d empty words" % (t + 1, d, e) for t, (d, e) in enumerate(zip(want[1], want[2]))]
    assert sorted(os.listdir(str(tmp_path))) == sorted([os.path.basename(p) for p in paths] + ["list.txt", "vocab.bin"])
    r = subprocess.run([EXE, "--batch", str(lst), "--train-vocabulary", out, "--words", "1000"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "590 keys" in r.stderr, r.stderr


@pytest.mark.gpu
def test_cpp_detector_trains_a_vocabulary(e2e, tmp_path):
    """tests/native/train_vocabulary_keys.cpp: trainVocabulary through hesaff.hpp holds what the Python path holds"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, plain, _ = e2e
    exe = str(tmp_path / "train_vocabulary_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "train_vocabulary_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    out = str(tmp_path / "cpp.bin")
    r = subprocess.run([exe, os.path.join(GOLD, "band_160x120.pgm"), "33", "3", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want = reference("cpp", np.ascontiguousarray(plain[0][1]["desc"]), 33, 3)
    assert r.stdout.strip().split("\n") == ["T %d" % len(want[1])] + ["I %d %d" % (d, e) for d, e in zip(want[1], want[2])]
    assert open(out, "rb").read() == V.vocabulary_file(want[0])


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_leave_the_context_and_its_vocabulary_alone(tctx, e2e):
    import torch
    imgs, plain, _ = e2e
    L, h = tctx.L, tctx.h
    own = V.family("uniform", 40, seed=71)
    tctx.set_vocabulary(own)
    own_words = V.assign(plain[1][1]["desc"], own)
    desc = V.family("uniform", 64, seed=72)
    init = V.family("uniform", 8, seed=73)
    out = np.full((8, 128), 7, np.uint8)
    dist = np.full(4, 7, np.int64); empty = np.full(4, 7, np.int32); done = ctypes.c_int(7)
    t = torch.from_numpy(desc).cuda()
    torch.cuda.synchronize()
    dp, op = ctypes.c_void_p(t.data_ptr()), out.ctypes.data
    rest = (dist.ctypes.data, empty.ctypes.data, ctypes.byref(done))

    def still_works():
        assert tctx.vocabulary_size == 40
        (nh, keys), = tctx.detect_batch(imgs[1:2])
        assert keys.tobytes() == plain[1][1].tobytes() and np.array_equal(tctx.words(0), own_words)
    try:
        host, dev = L.hesaff_train_vocabulary, L.hesaff_train_vocabulary_device
        # NULL arrays
        assert host(h, 64, None, 8, init.ctypes.data, 2, op, *rest) == ARG and host(h, 64, desc.ctypes.data, 8, init.ctypes.data, 2, None, *rest) == ARG
        assert dev(h, 64, None, 128, 0, 8, init.ctypes.data, 2, op, *rest) == ARG and dev(h, 64, dp, 128, 0, 8, init.ctypes.data, 2, None, *rest) == ARG
        # n, k, iterations
        for n, k, iters, ini in ((0, 8, 2, init), (-1, 8, 2, init), (64, 0, 2, init), (64, -1, 2, init), (64, (1 << 20) + 1, 2, init), (64, 8, 0, init),
                                 (64, 8, -1, init), (7, 8, 2, None), (64, 65, 2, None)):
            ip = ini.ctypes.data if ini is not None else None
            assert host(h, n, desc.ctypes.data, k, ip, iters, op, *rest) == ARG, (n, k, iters)
            assert dev(h, n, dp, 128, 0, k, ip, iters, op, *rest) == ARG, (n, k, iters)
        # the source rules of hesaff_assign_words_device
        for stride, offset in ((127, 0), (124, 0), (164, -4), (164, 40), (128, 4), (166, 36), (164, 38), (164, 37)):
            assert dev(h, 4, dp, stride, offset, 2, init.ctypes.data, 2, op, *rest) == ARG, (stride, offset)
        assert dev(h, 4, ctypes.c_void_p(t.data_ptr() + 2), 128, 0, 2, init.ctypes.data, 2, op, *rest) == ARG
        assert (out == 7).all() and (dist == 7).all() and (empty == 7).all() and done.value == 7
        for bad in (init[:7], init.astype(np.int8), init[:, :64]):
            with pytest.raises(ValueError):
                tctx.train_vocabulary(desc, 8, 2, init=bad)
        for bad in (desc.astype(np.int32), desc[:, :64], desc.reshape(-1)):
            with pytest.raises(ValueError):
                tctx.train_vocabulary(bad, 8, 2)
        still_works()
        # the stage operator: NULL arrays, counts, and a word outside 0 .. k - 1 (found on the host)
        acc = L.hesaff_stage_accumulate_words
        words = np.zeros(64, np.int32)
        sums = np.full((8, 128), 7, np.uint32); counts = np.full(8, 7, np.uint32)
        sp, cp = sums.ctypes.data, counts.ctypes.data
        assert acc(h, 64, None, words.ctypes.data, 8, sp, cp) == ARG and acc(h, 64, desc.ctypes.data, None, 8, sp, cp) == ARG
        assert acc(h, 64, desc.ctypes.data, words.ctypes.data, 8, None, cp) == ARG and acc(h, 64, desc.ctypes.data, words.ctypes.data, 8, sp, None) == ARG
        for n, k in ((0, 8), (-1, 8), (64, 0), (64, (1 << 20) + 1)):
            assert acc(h, n, desc.ctypes.data, words.ctypes.data, k, sp, cp) == ARG, (n, k)
        for at, w in ((0, -1), (63, 8), (31, 1 << 30)):
            words[:] = 0
            words[at] = w
            assert acc(h, 64, desc.ctypes.data, words.ctypes.data, 8, sp, cp) == ARG, (at, w)
        assert (sums == 7).all() and (counts == 7).all()
        ms = ctypes.c_float()
        assert L.hesaff_get_training_ms(h, None, ctypes.byref(ms), ctypes.byref(ms)) == ARG
        still_works()
        # and a good call between them changes nothing of the context's own either
        _same(tctx.train_vocabulary(desc, 8, 2, init=init), reference("refusals", desc, 8, 2, init), "a good call")
        still_works()
    finally:
        tctx.set_vocabulary(None)


@pytest.mark.gpu
def test_training_ms_are_event_times(tctx):
    desc = T.clustered()
    tctx.set_profiling(1)
    try:
        tctx.train_vocabulary(desc, 33, 2)
        ms = tctx.training_ms
        print("training_ms (assign, accumulate, update) for 4099 keys, K = 33, 2 iterations:", ms)
        assert all(0.0 < v < 1000.0 for v in ms)
    finally:
        tctx.set_profiling(0)
    tctx.train_vocabulary(desc, 33, 1)
    assert tctx.training_ms == (0.0, 0.0, 0.0)
