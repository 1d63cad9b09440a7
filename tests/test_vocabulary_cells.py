"""GPU suite of vocabulary cells (hesaff_set_vocabulary_cells, include/hesaff_amd.h; k_assign_words_cells, kernels_cells.h).  The
reference is tests/vocabulary_cells_ref.py: the numpy assignment against the coarse rows, then against the rows of the cell.  Every
comparison is bit for bit - the word, whose ties the reference alone decides, and the distance."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import OUT_BIN, OUT_WORDS
from tests import vocabulary_cells_ref as R
from tests import vocabulary_ref as V
from tests import vocabulary_training_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
E2E_IMAGES = ["band_160x120", "band_96x96", "band_160x120", "tiny_20x15", "band_96x96"]
E2E_KEYS = [221, 74, 221, 0, 74]
ARG = -2


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


def const_rows(values):
    return np.stack([np.full(128, v, np.uint8) for v in values])


@pytest.fixture(scope="module")
def cctx():
    """a context of its own with max_batch = 2 (the session's context keeps neither a vocabulary nor a layer)"""
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        assert c.vocabulary_size == 0 and c.vocabulary_cells() == 0
        yield c
        c.set_vocabulary(None)


def run(c, desc, vocab, coarse, first, what):
    """set the vocabulary and the layer, assign through the stage operator, compare with the reference; -> the reference rows"""
    c.set_vocabulary(vocab)
    c.set_vocabulary_cells(coarse, first)
    assert c.vocabulary_cells() == len(coarse) and c.vocabulary_size == len(vocab)
    want = R.assign_cells(desc, vocab, coarse, first)
    _same_rows(c.assign_words(desc), want, what)
    return want


# ---------------------------------------------------------------- the stage operator

@pytest.mark.gpu
@pytest.mark.parametrize("family", V.FAMILIES)
def test_key_counts_in_every_family(cctx, family):
    """n in {0, 1, 63, 64, 65, 257}, K = 257 in five cells whose borders lie inside tiles: the tails of an item and of a block"""
    vocab = V.family(family, 257, seed=301)
    coarse = V.family(family, 5, seed=302)
    first = [0, 31, 70, 71, 200, 257]
    desc = V.family(family, 257, seed=303)
    cctx.set_vocabulary(vocab)
    cctx.set_vocabulary_cells(coarse, first)
    want = R.assign_cells(desc, vocab, coarse, first)
    for n in (0, 1, 63, 64, 65, 257):
        _same_rows(cctx.assign_words(desc[:n]), want[:n], "%s, n = %d" % (family, n))
    assert ((want[:, 0] >= 0) & (want[:, 0] < 257)).all()


@pytest.mark.gpu
def test_one_cell_is_the_flat_assignment_and_every_row_a_cell(cctx):
    vocab = V.family("uniform", 321, seed=311)
    desc = V.family("uniform", 257, seed=312)
    want = run(cctx, desc, vocab, V.family("uniform", 1, seed=313), [0, 321], "C = 1")
    cctx.set_vocabulary_cells(None)
    assert cctx.vocabulary_cells() == 0
    flat = cctx.assign_words(desc)
    _same_rows(flat, want, "C = 1 against the flat kernel of the same context")
    _same_rows(flat, V.assign(desc, vocab), "the flat kernel")
    # C = K: the word is the cell, the coarse rows decide alone
    vocab = V.family("uniform", 65, seed=314)
    coarse = V.family("uniform", 65, seed=315)
    want = run(cctx, desc, vocab, coarse, list(range(66)), "C = K")
    assert np.array_equal(want[:, 0], V.assign(desc, coarse)[:, 0]) and (want != V.assign(desc, vocab)).any()


@pytest.mark.gpu
def test_cell_boundaries_at_tile_edges(cctx):
    """a border at rows 31 / 32 / 33 and 63 / 64 / 65, one at a time and all at once; a cell inside one tile, rows [5, 9)"""
    vocab = V.family("uniform", 130, seed=321)
    desc = V.family("uniform", 130, seed=322)
    for b in (31, 32, 33, 63, 64, 65):
        run(cctx, desc, vocab, V.family("uniform", 2, seed=323), [0, b, 130], "border at %d" % b)
    run(cctx, desc, vocab, V.family("uniform", 7, seed=324), [0, 31, 32, 33, 63, 64, 65, 130], "borders all at once")
    want = run(cctx, desc, vocab, V.family("uniform", 3, seed=325), [0, 5, 9, 130], "a cell inside one tile")
    assert ((want[:, 0] >= 5) & (want[:, 0] < 9)).sum() >= 10


@pytest.mark.gpu
def test_a_cell_of_100_tiles_and_a_cell_without_keys(cctx):
    K = 50 + 3200 + 40
    vocab = V.family("uniform", K, seed=331)
    desc = V.family("uniform", 257, seed=332)
    # coarse rows 0 and 2 are far from every uniform key; row 1 takes them all: 257 keys in one cell are five items
    coarse = np.concatenate([const_rows([0]), V.family("uniform", 1, seed=333), const_rows([255])])
    want = run(cctx, desc, vocab, coarse, [0, 50, 3250, K], "all keys in the cell of 100 tiles")
    assert ((want[:, 0] >= 50) & (want[:, 0] < 3250)).all()
    flat = V.assign(desc, vocab)
    assert (flat[:, 0] < 50).any() or (flat[:, 0] >= 3250).any()   # the layer ignored would show
    assert (want != flat).any()


@pytest.mark.gpu
def test_one_key_per_cell(cctx):
    """65 cells of three rows, key i equal to coarse row i: 65 items of one key each, more waves in the grid than items"""
    desc = V.family("uniform", 65, seed=341)
    vocab = V.family("uniform", 195, seed=342)
    first = [3 * i for i in range(66)]
    want = run(cctx, desc, vocab, desc.copy(), first, "one key per cell")
    assert np.array_equal(want[:, 0] // 3, np.arange(65))


@pytest.mark.gpu
def test_rows_outside_the_cell_never_win(cctx):
    """the mask: a row at distance 0 at first[c] - 1, in the tile of the cell's first row, and another at first[c + 1], in the tile of
    its last row; the flat nearest row of every key lies in another cell"""
    vocab = V.family("uniform", 200, seed=351)
    key = V.family("uniform", 1, seed=352)
    desc = np.repeat(key, 70, axis=0)
    coarse = np.concatenate([const_rows([0]), key, const_rows([255])])
    for lo, hi in ((40, 90), (33, 63), (5, 9), (64, 96), (1, 199)):
        v = vocab.copy()
        v[lo - 1] = key[0]
        v[hi] = key[0]
        want = run(cctx, desc, v, coarse, [0, lo, hi, 200], "zero-distance rows at %d and %d" % (lo - 1, hi))
        assert (want[:, 0] >= lo).all() and (want[:, 0] < hi).all() and (want[:, 1] > 0).all()
        assert V.assign(desc[:1], v)[0].tolist() == [lo - 1, 0]


@pytest.mark.gpu
def test_ties_and_the_extreme_distance(cctx):
    vocab = V.family("uniform", 130, seed=361)
    desc = V.family("uniform", 70, seed=362)
    # duplicate rows inside a cell: the lower row; equal coarse rows: the lower cell
    vocab[45] = vocab[41]
    vocab[100] = vocab[41]
    desc[0] = vocab[41]
    g = V.family("uniform", 1, seed=363)
    coarse = np.concatenate([const_rows([0]), g, g, const_rows([255])])
    want = run(cctx, desc, vocab, coarse, [0, 35, 70, 110, 130], "ties")
    assert want[0].tolist() == [41, 0] and ((want[:, 0] >= 35) & (want[:, 0] < 70)).all()
    # 128 * 255^2 inside an edge tile: the key is all 0 and falls into the cell whose rows, [5, 9), are all 255
    vocab[5:9] = 255
    coarse = np.concatenate([const_rows([200]), const_rows([0]), const_rows([255])])
    want = run(cctx, np.zeros((3, 128), np.uint8), vocab, coarse, [0, 5, 9, 130], "the extreme distance")
    assert want.tolist() == [[5, 8323200]] * 3


@pytest.mark.gpu
def test_strided_device_source(cctx):
    """hesaff_assign_words_device on a [65, 164] tensor, the descriptor 36 bytes in and 0xFF around it, and on the packed tensor"""
    import torch
    vocab = V.family("uniform", 257, seed=371)
    coarse = V.family("uniform", 5, seed=372)
    first = [0, 31, 70, 71, 200, 257]
    desc = V.family("uniform", 65, seed=373)
    want = run(cctx, desc, vocab, coarse, first, "host run")
    rec = np.full((65, 164), 0xFF, np.uint8)
    rec[:, 36:] = desc
    for src, stride, offset in ((rec, 164, 36), (desc, 128, 0)):
        t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
        out = torch.full((65, 2), -1, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        cctx.assign_words_device(t.data_ptr(), 65, stride, offset, out.data_ptr())
        _same_rows(out.cpu().numpy(), want, "stride %d" % stride)


@pytest.mark.gpu
def test_layer_state_and_timers(cctx):
    """hesaff_set_vocabulary drops the layer; a layer replaces a layer; the three event times add up to no more than the whole"""
    vocab = V.family("uniform", 257, seed=381)
    desc = V.family("uniform", 257, seed=382)
    run(cctx, desc, vocab, V.family("uniform", 5, seed=383), [0, 31, 70, 71, 200, 257], "five cells")
    run(cctx, desc, vocab, V.family("uniform", 2, seed=384), [0, 100, 257], "then two")
    cctx.set_vocabulary(vocab)
    assert cctx.vocabulary_cells() == 0
    _same_rows(cctx.assign_words(desc), V.assign(desc, vocab), "flat after set_vocabulary")
    assert cctx.assign_cells_ms == (0.0, 0.0, 0.0)
    cctx.set_vocabulary_cells(V.family("uniform", 2, seed=384), [0, 100, 257])
    cctx.set_profiling(1)
    try:
        cctx.assign_words(desc)
        parts, whole = cctx.assign_cells_ms, cctx.assign_ms
        print("assign through 2 cells, 257 keys: coarse %.4f, group %.4f, fine %.4f, whole %.4f ms" % (parts + (whole,)))
        assert all(p > 0.0 for p in parts) and sum(parts) <= whole * 1.001 + 1e-3
        cctx.set_vocabulary_cells(None)
        cctx.assign_words(desc)
        assert cctx.assign_cells_ms == (0.0, 0.0, 0.0) and cctx.assign_ms > 0.0
    finally:
        cctx.set_profiling(0)


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def e2e(cctx):
    """the five images, their keys without a vocabulary, and a layer: 300 rows, half of them the images' own descriptors, sorted by the
    reference into the cells of eight of those descriptors"""
    cctx.set_vocabulary(None)
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    plain = cctx.detect_batch(imgs)
    assert [len(k) for _, k in plain] == E2E_KEYS
    own = np.concatenate([plain[0][1]["desc"], plain[1][1]["desc"]])
    rng = np.random.RandomState(77)
    rows = rng.randint(0, 256, (300, 128)).astype(np.uint8)
    rows[rng.permutation(300)[:150]] = own[rng.permutation(len(own))[:150]]
    vocab, _, coarse, first = R.build_cells(rows, own[rng.permutation(len(own))[:8]])
    assert len(coarse) >= 4
    want = [R.assign_cells(k["desc"], vocab, coarse, first) for _, k in plain]
    flat = V.assign(plain[0][1]["desc"], vocab)
    assert (want[0] != flat).any(), "the layer ignored would pass"
    return imgs, plain, vocab, coarse, first, want


def _set(c, e2e):
    imgs, plain, vocab, coarse, first, want = e2e
    c.set_vocabulary(vocab)
    c.set_vocabulary_cells(coarse, first)


@pytest.mark.gpu
def test_end_to_end_detect_batch(cctx, e2e):
    """five images of two sizes interleaved, max_batch = 2: words(i) is the reference on the keys of image i"""
    imgs, plain, vocab, coarse, first, want = e2e
    _set(cctx, e2e)
    res = cctx.detect_batch(imgs)
    for i, ((_, keys), (_, pk)) in enumerate(zip(res, plain)):
        assert keys.tobytes() == pk.tobytes(), i
        _same_rows(cctx.words(i), want[i], "detect_batch: image %d" % i)


@pytest.mark.gpu
def test_end_to_end_device_resident(e2e):
    import torch
    from tests.test_gpu_parity import _device_keys
    imgs, plain, vocab, coarse, first, want = e2e
    img = imgs[0]
    with hesaff_amd.HesaffContext(device=0) as c:
        _set(c, e2e)
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


@pytest.mark.gpu
def test_end_to_end_with_two_keys_per_region(e2e):
    """dominant orientation, two keys per region: one row per KEY, the reference on those keys' bytes"""
    imgs, plain, vocab, coarse, first, _ = e2e
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        c.set_orientation("dominant")
        c.set_orientation_count(2)
        base = c.detect_batch(imgs)
        _set(c, e2e)
        res = c.detect_batch(imgs)
        assert len(res[0][1]) > 221
        for i, ((nh, keys), (_, bk)) in enumerate(zip(res, base)):
            assert keys.tobytes() == bk.tobytes()
            _same_rows(c.words(i), R.assign_cells(keys["desc"], vocab, coarse, first), "two keys per region: image %d" % i)


def _copies(tmp_path):
    paths = []
    for j, n in enumerate(E2E_IMAGES):
        paths.append(str(tmp_path / ("%d_%s.pgm" % (j, n))))
        shutil.copyfile(os.path.join(GOLD, n + ".pgm"), paths[-1])
    return paths


def _want_words_file(tmp_path, keys, want, K):
    ref = str(tmp_path / "ref.bin")
    hesaff_amd.write_bin(ref, keys, hesaff_amd.default_params().mrSize)
    rows = hesaff_amd.read_bin(ref)
    xyabc = np.stack([rows[f] for f in ("x", "y", "a", "b", "c")], axis=1) if len(rows) else np.zeros((0, 5), np.float32)
    return V.words_file(xyabc, want, K)


@pytest.mark.gpu
def test_process_files_and_the_cli_write_the_cells_words(cctx, e2e, tmp_path):
    imgs, plain, vocab, coarse, first, want = e2e
    paths = _copies(tmp_path)
    expect = [_want_words_file(tmp_path, plain[i][1], want[i], 300) for i in range(5)]
    _set(cctx, e2e)
    cctx.set_output_format(OUT_BIN | OUT_WORDS)
    try:
        st = cctx.process_files(paths)
    finally:
        cctx.set_output_format(1)
    for i, p in enumerate(paths):
        assert st[i][0] == 0 and st[i][3] == E2E_KEYS[i]
        assert open(p + ".hesaff.words", "rb").read() == expect[i], p
        os.remove(p + ".hesaff.words")
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    hesaff_amd.write_vocabulary_cells(vfile + ".cells", coarse, first)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile, "--cells", vfile + ".cells", "--words-only"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for i, p in enumerate(paths):
        assert open(p + ".hesaff.words", "rb").read() == expect[i], p
        os.remove(p + ".hesaff.words")
    r = subprocess.run([EXE, paths[0], "--vocabulary", vfile, "--cells", vfile + ".cells"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(paths[0] + ".hesaff.words", "rb").read() == expect[0]


# ---------------------------------------------------------------- building and training

@pytest.mark.gpu
def test_build_vocabulary_cells(cctx):
    for K in (33, 257):
        words = V.family("uniform", K, seed=400 + K)
        for C in (1, 4, 33):
            coarse = V.family("uniform", C, seed=410 + C)
            if C > 1:
                coarse[1] = 255   # twice as far from a uniform row as another uniform row is: attracts none
            want = R.build_cells(words, coarse)
            got = cctx.build_vocabulary_cells(words, coarse)
            assert len(want[2]) < C or C == 1
            for g, w, name in zip(got, want, ("words", "order", "coarse", "first")):
                assert g.dtype == w.dtype and np.array_equal(g, w), (K, C, name)
    with pytest.raises(hesaff_amd.HesaffError):
        cctx.build_vocabulary_cells(V.family("uniform", 3, seed=1), V.family("uniform", 4, seed=2))   # more cells than rows


@pytest.fixture(scope="module")
def clustered():
    desc = T.clustered()
    g = T.train(desc, 4, 3)[0]
    v0, _, coarse, first = R.build_cells(T.sample(desc, 33), g)
    return desc, v0, coarse, first


@pytest.mark.gpu
@pytest.mark.parametrize("iterations", (1, 4))
def test_train_vocabulary_cells(cctx, clustered, iterations):
    import torch
    desc, v0, coarse, first = clustered
    want = R.train_cells(desc, v0, coarse, first, iterations)
    got = cctx.train_vocabulary_cells(desc, v0, coarse, first, iterations)
    for g, w, name in zip(got, want, ("rows", "distortion", "empty")):
        assert g.dtype == w.dtype and np.array_equal(g, w), (name, g, w)
    assert (np.diff(got[1]) <= 0).all()
    t = torch.from_numpy(desc).cuda()
    torch.cuda.synchronize()
    dev = cctx.train_vocabulary_cells_device(t.data_ptr(), len(desc), 128, 0, v0, coarse, first, iterations)
    assert all(np.array_equal(a, b) for a, b in zip(dev, got))
    # one cell: flat training from the same rows
    init = T.sample(desc, 33)
    one = cctx.train_vocabulary_cells(desc, init, V.family("low", 1, seed=1), [0, 33], iterations)
    flat = T.train(desc, 33, iterations, init=init)
    assert all(np.array_equal(a, b) for a, b in zip(one, flat))


@pytest.mark.gpu
def test_the_composite_and_the_cli_train_mode(cctx, e2e, tmp_path):
    imgs, plain = e2e[0], e2e[1]
    desc = np.ascontiguousarray(np.concatenate([k["desc"] for _, k in plain]))
    want = R.train_cell_vocabulary(desc, 33, 4, 4, 3)
    got = cctx.train_cell_vocabulary(desc, 33, 4, 4, 3)
    for g, w, name in zip(got, want, ("rows", "coarse", "first", "distortion", "empty")):
        assert np.array_equal(g, w), name
    with pytest.raises(ValueError):
        cctx.train_cell_vocabulary(desc, 3, 4, 1, 1)
    paths = _copies(tmp_path)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    out = str(tmp_path / "vocab.bin")
    r = subprocess.run([EXE, "--batch", str(lst), "--train-vocabulary", out, "--words", "33", "--cells", "4", "--iterations", "4", "--coarse-iterations", "3"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(out, "rb").read() == V.vocabulary_file(want[0])
    assert open(out + ".cells", "rb").read() == R.cells_file(want[1], want[2])


@pytest.mark.gpu
def test_cpp_detector_with_cells(tmp_path):
    """tests/native/vocabulary_cells_keys.cpp: the members of hesaff.hpp run the composite and assign through the layer it made"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "vocabulary_cells_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "vocabulary_cells_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    out = str(tmp_path / "vocab.bin")
    r = subprocess.run([exe, os.path.join(GOLD, "band_160x120.pgm"), "33", "4", "3", out], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    with hesaff_amd.HesaffContext(device=0) as c:
        (_, keys), = c.detect_batch([hesaff_amd.read_pnm(os.path.join(GOLD, "band_160x120.pgm"))])
    desc = np.ascontiguousarray(keys["desc"])
    words, coarse, first, dist, empty = R.train_cell_vocabulary(desc, 33, 4, 3, 3)
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "C %d" % len(coarse)
    assert lines[1:1 + len(dist)] == ["I %d %d" % (d, e) for d, e in zip(dist, empty)]
    assert lines[1 + len(dist):] == ["W %d %d" % (w, d) for w, d in R.assign_cells(desc, words, coarse, first)]
    assert open(out, "rb").read() == V.vocabulary_file(words) and open(out + ".cells", "rb").read() == R.cells_file(coarse, first)


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_leave_the_context_and_the_layer_as_they_were(cctx, e2e):
    imgs, plain, vocab, coarse, first, want = e2e
    L, h = cctx.L, cctx.h
    f = np.asarray(first, np.uint32)
    C = len(coarse)

    def still_works():
        assert cctx.vocabulary_size == 300 and cctx.vocabulary_cells() == C
        (nh, keys), = cctx.detect_batch(imgs[1:2])
        assert keys.tobytes() == plain[1][1].tobytes()
        _same_rows(cctx.words(0), want[1], "after a refusal")
    # no vocabulary: nothing to lay cells over
    cctx.set_vocabulary(None)
    assert L.hesaff_set_vocabulary_cells(h, C, coarse.ctypes.data, f.ctypes.data) == ARG
    assert L.hesaff_set_vocabulary_cells(h, 0, None, None) == ARG
    (nh, keys), = cctx.detect_batch(imgs[1:2])
    assert keys.tobytes() == plain[1][1].tobytes() and cctx.vocabulary_cells() == 0
    _set(cctx, e2e)
    still_works()
    many = V.family("uniform", 301, seed=5)
    assert L.hesaff_set_vocabulary_cells(h, -1, coarse.ctypes.data, f.ctypes.data) == ARG
    assert L.hesaff_set_vocabulary_cells(h, 301, many.ctypes.data, np.arange(302, dtype=np.uint32).ctypes.data) == ARG
    assert L.hesaff_set_vocabulary_cells(h, C, None, f.ctypes.data) == ARG
    assert L.hesaff_set_vocabulary_cells(h, C, coarse.ctypes.data, None) == ARG
    for bad in (f + 1, np.concatenate([f[:-1], [299]]), np.concatenate([f[:1], f[:1], f[2:]]) if C > 1 else f + 1, np.concatenate([f[:1], f[2:3], f[1:2], f[3:]])):
        b = np.ascontiguousarray(bad, dtype=np.uint32)
        assert len(b) == C + 1 and L.hesaff_set_vocabulary_cells(h, C, coarse.ctypes.data, b.ctypes.data) == ARG, bad
    assert L.hesaff_get_vocabulary_cells(h, None) == ARG
    ms = ctypes.c_float()
    assert L.hesaff_get_assign_cells_ms(h, None, ctypes.byref(ms), ctypes.byref(ms)) == ARG
    for bad_first in ([0, 300], list(first[:-1]) + [301]):
        with pytest.raises((ValueError, hesaff_amd.HesaffError)):
            cctx.set_vocabulary_cells(coarse, bad_first)
    still_works()
    # training and building: a NULL array, a first that is no layer over the rows, counts outside the bounds
    desc = np.ascontiguousarray(plain[1][1]["desc"])
    rows = np.ascontiguousarray(vocab[:8]); g = np.ascontiguousarray(coarse[:2]); f2 = np.array([0, 3, 8], np.uint32)
    out = np.full((8, 128), 7, np.uint8)
    call = lambda n, d, k, init, c, gg, ff, it, o: L.hesaff_train_vocabulary_cells(h, n, d, k, init, c, gg, ff, it, o, None, None, None)
    ok = (len(desc), desc.ctypes.data, 8, rows.ctypes.data, 2, g.ctypes.data, f2.ctypes.data, 1, out.ctypes.data)
    for i, v in ((0, 0), (0, (1 << 24) + 1), (1, None), (2, 0), (3, None), (4, 0), (4, 9), (5, None), (6, None), (7, 0), (8, None)):
        args = list(ok); args[i] = v
        assert call(*args) == ARG, (i, v)
    assert call(*(ok[:6] + (np.array([0, 3, 9], np.uint32).ctypes.data,) + ok[7:])) == ARG
    assert (out == 7).all()
    kept = ctypes.c_int(7)
    order = np.zeros(8, np.int32); g_out = np.zeros((2, 128), np.uint8); f_out = np.zeros(3, np.uint32)
    bargs = (8, rows.ctypes.data, 2, g.ctypes.data, out.ctypes.data, order.ctypes.data, g_out.ctypes.data, f_out.ctypes.data, ctypes.byref(kept))
    for i, v in ((0, 0), (0, (1 << 20) + 1), (1, None), (2, 0), (2, 9), (3, None), (4, None), (5, None), (6, None), (7, None), (8, None)):
        args = list(bargs); args[i] = v
        assert L.hesaff_build_vocabulary_cells(h, *args) == ARG, (i, v)
    assert (out == 7).all() and kept.value == 7
    still_works()
