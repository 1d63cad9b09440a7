"""GPU suite of vocabulary probes (hesaff_set_vocabulary_probes, include/hesaff_amd.h; k_probe_cells, k_assign_words_cells<true> and
k_merge_probes, kernels_cells.h).  The reference is tests/vocabulary_probes_ref.py, whose fixed ends and properties
tests/test_vocabulary_probes_host.py holds.  Every comparison is bit for bit - the cells and the word, whose ties the reference alone
decides, and the distances."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import OUT_BIN, OUT_WORDS
from tests import vocabulary_cells_ref as R
from tests import vocabulary_probes_ref as P
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
E2E_IMAGES = ["band_160x120", "band_96x96", "band_160x120", "tiny_20x15", "band_96x96"]
E2E_KEYS = [221, 74, 221, 0, 74]
FIRST = [0, 31, 70, 71, 200, 257]
ARG = -2


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _same(got, want, what):
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.nonzero((got != want).any(axis=1))[0] if want.size else []
    assert len(bad) == 0, "%s: %d of %d rows differ, first %s: got %s, want %s" % (what, len(bad), len(want), list(bad[:6]), got[bad[:3]].tolist(),
                                                                                  want[bad[:3]].tolist())


def const_rows(values):
    return np.stack([np.full(128, v, np.uint8) for v in values])


@pytest.fixture(scope="module")
def pctx():
    """a context of its own with max_batch = 2; every test leaves it with one probe"""
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        assert c.vocabulary_size == 0 and c.vocabulary_cells() == 0 and c.vocabulary_probes() == 1
        yield c
        c.set_vocabulary(None)


def run(c, desc, vocab, coarse, first, probes, what):
    """set the vocabulary, the layer and the probe count; the stage operators against the reference; -> the reference rows"""
    c.set_vocabulary(vocab)
    c.set_vocabulary_cells(coarse, first)
    c.set_vocabulary_probes(probes)
    try:
        assert c.vocabulary_probes() == probes and c.vocabulary_cells() == len(coarse)
        want = P.assign_probes(desc, vocab, coarse, first, probes)
        _same(c.assign_words(desc), want, what)
        wc, wd = P.probe_cells(desc, coarse, probes)
        gc, gd = c.probe_cells(desc)
        _same(gc, wc, what + ": probed cells")
        _same(gd, wd, what + ": distances to the coarse rows")
    finally:
        c.set_vocabulary_probes(1)
    return want


# ---------------------------------------------------------------- the stage operators

@pytest.mark.gpu
@pytest.mark.parametrize("family", V.FAMILIES)
def test_probe_and_key_counts_in_every_family(pctx, family):
    """P in {1, 2, 3, 5, 8} x n in {0, 1, 63, 64, 65, 257}, K = 257 in five cells whose borders lie inside tiles: the tails of an item
    where n P crosses multiples of 64; P = 1 against the context before probes were set, P >= C against its own flat kernel"""
    vocab = V.family(family, 257, seed=301)
    coarse = V.family(family, 5, seed=302)
    desc = V.family(family, 257, seed=303)
    pctx.set_vocabulary(vocab)
    flat = pctx.assign_words(desc)
    _same(flat, V.assign(desc, vocab), "the flat kernel")
    pctx.set_vocabulary_cells(coarse, FIRST)
    before = pctx.assign_words(desc)   # (one probe: the default, or what the test before left)
    _same(before, R.assign_cells(desc, vocab, coarse, FIRST), "one probe")
    try:
        for probes in (1, 2, 3, 5, 8):
            pctx.set_vocabulary_probes(probes)
            want = P.assign_probes(desc, vocab, coarse, FIRST, probes)
            wc, wd = P.probe_cells(desc, coarse, probes)
            for n in (0, 1, 63, 64, 65, 257):
                what = "%s, P = %d, n = %d" % (family, probes, n)
                _same(pctx.assign_words(desc[:n]), want[:n], what)
                gc, gd = pctx.probe_cells(desc[:n])
                _same(gc, wc[:n], what + ": cells")
                _same(gd, wd[:n], what + ": coarse distances")
            if probes == 1:
                _same(want, before, "P = 1 is the layer alone")
            if probes >= 5:
                _same(want, flat, "P >= C is the flat assignment")
    finally:
        pctx.set_vocabulary_probes(1)


@pytest.mark.gpu
def test_coarse_ties_are_probed_in_ascending_cell(pctx):
    desc = V.family("uniform", 70, seed=401)
    # 70 identical coarse rows - three tiles, the last with pad rows - over 140 rows: the probes are cells 0 .. 7
    vocab = V.family("uniform", 140, seed=402)
    coarse = np.repeat(V.family("uniform", 1, seed=403), 70, axis=0)
    pctx.set_vocabulary(vocab)
    pctx.set_vocabulary_cells(coarse, list(range(0, 141, 2)))
    pctx.set_vocabulary_probes(8)
    try:
        cells, dist2 = pctx.probe_cells(desc)
        assert cells.tolist() == [list(range(8))] * 70 and (dist2 == dist2[:, :1]).all()
    finally:
        pctx.set_vocabulary_probes(1)
    want = run(pctx, desc, vocab, coarse, list(range(0, 141, 2)), 8, "70 identical coarse rows")
    assert (want[:, 0] < 16).all()
    # equal coarse rows at 3 / 4 (the two half-lanes of a column), 31 / 32 (a tile border) and 63 / 64, each the nearest of some keys
    coarse = V.family("uniform", 70, seed=404)
    for j, a in enumerate((3, 31, 63)):
        coarse[a + 1] = coarse[a]
        desc[10 * j:10 * j + 10] = coarse[a]
    for probes in (2, 3):
        run(pctx, desc, vocab, coarse, list(range(0, 141, 2)), probes, "equal coarse rows in pairs, P = %d" % probes)
    cells, _ = P.probe_cells(desc, coarse, 2)
    for a in (3, 31, 63):
        assert (cells == [a, a + 1]).all(axis=1).sum() >= 10, a


@pytest.mark.gpu
def test_fewer_cells_than_probes_and_pad_rows_of_the_coarse_layer(pctx):
    vocab = V.family("uniform", 130, seed=411)
    desc = V.family("uniform", 130, seed=412)
    want = run(pctx, desc, vocab, V.family("uniform", 3, seed=413), [0, 40, 90, 130], 8, "C = 3, P = 8")
    _same(want, V.assign(desc, vocab), "C < P is flat")
    # C = 33: the second coarse tile holds one row and 31 pad rows; every probe is a cell
    coarse = V.family("uniform", 33, seed=414)
    first = [0] + list(range(2, 65, 2)) + [130]
    want = run(pctx, desc, vocab, coarse, first, 8, "C = 33, P = 8")
    cells, dist2 = P.probe_cells(desc, coarse, 8)
    assert cells.max() == 32 and (cells == 32).sum() >= 10 and dist2.max() < 1 << 23
    # the far coarse rows are still probed when they are all that is left: C = 33, keys next to cell 32
    run(pctx, np.repeat(coarse[32:], 5, axis=0), vocab, coarse, first, 8, "keys on the last coarse row")


@pytest.mark.gpu
def test_a_zero_distance_row_wins_exactly_when_its_cell_is_probed(pctx):
    """coarse rows constant at 100 / 110 / 120 / 130, keys constant at 104: the ranks of the cells are 0, 1, 2, 3 by construction"""
    coarse = const_rows([100, 110, 120, 130])
    desc = const_rows([104] * 65)
    first = [0, 30, 33, 70, 96]
    for p in range(4):
        vocab = V.family("uniform", 96, seed=420 + p)
        row = first[p + 1] - 1
        vocab[row] = 104
        for probes in (1, 2, 3, 4, 8):
            want = run(pctx, desc, vocab, coarse, first, probes, "zero-distance row in the cell of rank %d, P = %d" % (p, probes))
            assert (want[0].tolist() == [row, 0]) == (probes > p), (p, probes, want[0])
            if probes <= p:   # never found: the word lies in a probed cell
                assert want[0, 1] > 0 and want[0, 0] < first[probes]


@pytest.mark.gpu
def test_a_fine_tie_across_probed_cells_goes_to_the_lower_row(pctx):
    coarse = const_rows([130, 120, 110, 100])   # the ranks of the cells are 3, 2, 1, 0: cell 3 is the nearest
    desc = const_rows([104] * 65)
    first = [0, 30, 33, 70, 96]
    vocab = V.family("uniform", 96, seed=431)
    vocab[80] = 104   # in the rank-0 cell, a high row
    vocab[40] = 104   # the same bytes in the rank-1 cell, a lower row
    assert run(pctx, desc, vocab, coarse, first, 1, "P = 1")[0].tolist() == [80, 0]
    for probes in (2, 3, 4):
        assert run(pctx, desc, vocab, coarse, first, probes, "P = %d" % probes)[64].tolist() == [40, 0]
    vocab[5] = 104    # and in the rank-3 cell
    assert run(pctx, desc, vocab, coarse, first, 3, "three of four")[0].tolist() == [40, 0]
    assert run(pctx, desc, vocab, coarse, first, 4, "all four")[0].tolist() == [5, 0]


@pytest.mark.gpu
def test_cell_borders_inside_tiles_with_two_probes(pctx):
    """the edge mask and the merge meet: borders at 31 / 32 / 33 and a cell [5, 9)"""
    vocab = V.family("uniform", 130, seed=441)
    desc = V.family("uniform", 130, seed=442)
    run(pctx, desc, vocab, V.family("uniform", 4, seed=443), [0, 31, 32, 33, 130], 2, "borders at 31, 32, 33")
    want = run(pctx, desc, vocab, V.family("uniform", 3, seed=444), [0, 5, 9, 130], 2, "a cell inside one tile")
    assert ((want[:, 0] >= 5) & (want[:, 0] < 9)).sum() >= 3
    # rows at distance 0 just outside the probed cells, in their edge tiles: never won
    key = V.family("uniform", 1, seed=445)
    v = vocab.copy()
    v[4] = key[0]; v[40] = key[0]
    coarse = np.concatenate([const_rows([0]), key, key, const_rows([255])])
    want = run(pctx, np.repeat(key, 70, axis=0), v, coarse, [0, 5, 9, 40, 130], 2, "zero-distance rows at 4 and 40")
    assert (want[:, 0] >= 5).all() and (want[:, 0] < 40).all() and (want[:, 1] > 0).all()


@pytest.mark.gpu
def test_the_extreme_distance(pctx):
    """dist2 = 128 * 255^2 = 8 323 200 to the coarse rows and to the word"""
    vocab = V.family("uniform", 130, seed=451)
    vocab[0:7] = 255
    coarse = const_rows([255, 255, 255])   # all as far from the zero key as a row can be: cells 0 and 1 are probed, [0, 4) and [4, 7)
    desc = np.zeros((3, 128), np.uint8)
    first = [0, 4, 7, 130]
    want = run(pctx, desc, vocab, coarse, first, 2, "the extreme distance")
    assert want.tolist() == [[0, 8323200]] * 3
    assert V.assign(desc, vocab)[0, 1] < 8323200   # a nearer row lies in the cell that is not probed
    pctx.set_vocabulary_probes(2)
    try:
        gc, gd = pctx.probe_cells(desc)
        assert gc.tolist() == [[0, 1]] * 3 and gd.tolist() == [[8323200, 8323200]] * 3
    finally:
        pctx.set_vocabulary_probes(1)


@pytest.mark.gpu
def test_strided_device_source(pctx):
    """hesaff_assign_words_device on a [65, 164] tensor, the descriptor 36 bytes in and 0xFF around it, and on the packed tensor"""
    import torch
    vocab = V.family("uniform", 257, seed=371)
    coarse = V.family("uniform", 5, seed=372)
    desc = V.family("uniform", 65, seed=373)
    want = run(pctx, desc, vocab, coarse, FIRST, 3, "host run")
    assert (want != R.assign_cells(desc, vocab, coarse, FIRST)).any()
    rec = np.full((65, 164), 0xFF, np.uint8)
    rec[:, 36:] = desc
    pctx.set_vocabulary_probes(3)
    try:
        for src, stride, offset in ((rec, 164, 36), (desc, 128, 0)):
            t = torch.from_numpy(np.ascontiguousarray(src)).cuda()
            out = torch.full((65, 2), -1, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            pctx.assign_words_device(t.data_ptr(), 65, stride, offset, out.data_ptr())
            _same(out.cpu().numpy(), want, "stride %d" % stride)
    finally:
        pctx.set_vocabulary_probes(1)


@pytest.mark.gpu
def test_setting_state_timers_and_refusals(pctx):
    """probes set before a layer exists; set_vocabulary drops the layer and keeps P; every refusal leaves setting and results alone"""
    L, h = pctx.L, pctx.h
    vocab = V.family("uniform", 257, seed=381)
    coarse = V.family("uniform", 5, seed=383)
    desc = V.family("uniform", 257, seed=382)
    flat = V.assign(desc, vocab)
    want3 = P.assign_probes(desc, vocab, coarse, FIRST, 3)
    assert (want3 != flat).any() and (want3 != R.assign_cells(desc, vocab, coarse, FIRST)).any()
    pctx.set_vocabulary(None)
    pctx.set_vocabulary_probes(3)
    try:
        assert pctx.vocabulary_probes() == 3
        with pytest.raises(hesaff_amd.HesaffError):
            pctx.probe_cells(desc)   # no layer
        pctx.set_vocabulary(vocab)
        assert pctx.vocabulary_probes() == 3
        _same(pctx.assign_words(desc), flat, "no layer: the flat search, whatever P")
        pctx.set_vocabulary_cells(coarse, FIRST)
        assert pctx.vocabulary_probes() == 3
        _same(pctx.assign_words(desc), want3, "P set before the layer")
        for bad in (0, 9, -1, 1 << 20):
            assert L.hesaff_set_vocabulary_probes(h, bad) == ARG
            with pytest.raises(hesaff_amd.HesaffError):
                pctx.set_vocabulary_probes(bad)
        assert L.hesaff_get_vocabulary_probes(h, None) == ARG
        cells = np.full((257, 3), 7, np.int32); dist2 = np.full((257, 3), 7, np.int32)
        d, cp, dp = desc.ctypes.data, cells.ctypes.data, dist2.ctypes.data
        for args in ((-1, d, cp, dp), (257, None, cp, dp), (257, d, None, dp), (257, d, cp, None), ((1 << 24) // 3 + 1, d, cp, dp)):
            assert L.hesaff_stage_probe_cells(h, *args) == ARG, args
        assert L.hesaff_stage_probe_cells(h, 0, None, None, None) == 0
        assert (cells == 7).all() and (dist2 == 7).all() and pctx.vocabulary_probes() == 3
        _same(pctx.assign_words(desc), want3, "after the refusals")
        # the three event times: the P' search, the grouping, the cells with the merge
        pctx.set_profiling(1)
        try:
            pctx.assign_words(desc)
            parts, whole = pctx.assign_cells_ms, pctx.assign_ms
            print("assign through 5 cells, 3 probes, 257 keys: coarse %.4f, group %.4f, fine %.4f, whole %.4f ms" % (parts + (whole,)))
            assert all(p > 0.0 for p in parts) and sum(parts) <= whole * 1.001 + 1e-3
        finally:
            pctx.set_profiling(0)
        pctx.set_vocabulary(vocab)
        assert pctx.vocabulary_cells() == 0 and pctx.vocabulary_probes() == 3
        _same(pctx.assign_words(desc), flat, "set_vocabulary dropped the layer")
        pctx.set_vocabulary_cells(coarse, FIRST)
        _same(pctx.assign_words(desc), want3, "and kept the probes")
        pctx.set_vocabulary_cells(None)
        assert pctx.vocabulary_probes() == 3
        assert L.hesaff_stage_probe_cells(h, 257, d, cp, dp) == ARG and (cells == 7).all()
    finally:
        pctx.set_vocabulary_probes(1)


# ---------------------------------------------------------------- end to end

@pytest.fixture(scope="module")
def e2e(pctx):
    """the five images, their keys without a vocabulary, and a layer: 300 rows, half of them the images' own descriptors, sorted by the
    reference into the cells of eight of those descriptors; the words under two probes"""
    pctx.set_vocabulary(None)
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    plain = pctx.detect_batch(imgs)
    assert [len(k) for _, k in plain] == E2E_KEYS
    own = np.concatenate([plain[0][1]["desc"], plain[1][1]["desc"]])
    rng = np.random.RandomState(77)
    rows = rng.randint(0, 256, (300, 128)).astype(np.uint8)
    rows[rng.permutation(300)[:150]] = own[rng.permutation(len(own))[:150]]
    vocab, _, coarse, first = R.build_cells(rows, own[rng.permutation(len(own))[:8]])
    assert len(coarse) >= 4
    want = [P.assign_probes(k["desc"], vocab, coarse, first, 2) for _, k in plain]
    one = R.assign_cells(plain[0][1]["desc"], vocab, coarse, first)
    flat = V.assign(plain[0][1]["desc"], vocab)
    assert (want[0] != one).any() and (want[0] != flat).any(), "the probes ignored, or the layer, would pass"
    return imgs, plain, vocab, coarse, first, want


def _set(c, e2e, probes=2):
    imgs, plain, vocab, coarse, first, want = e2e
    c.set_vocabulary(vocab)
    c.set_vocabulary_cells(coarse, first)
    c.set_vocabulary_probes(probes)


@pytest.mark.gpu
def test_end_to_end_detect_batch(pctx, e2e):
    """five images of two sizes interleaved, max_batch = 2: words(i) is the reference on the keys of image i"""
    imgs, plain, vocab, coarse, first, want = e2e
    _set(pctx, e2e)
    try:
        res = pctx.detect_batch(imgs)
        for i, ((_, keys), (_, pk)) in enumerate(zip(res, plain)):
            assert keys.tobytes() == pk.tobytes(), i
            _same(pctx.words(i), want[i], "detect_batch: image %d" % i)
    finally:
        pctx.set_vocabulary_probes(1)


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
            _same(c.words(i), P.assign_probes(keys["desc"], vocab, coarse, first, 2), "two keys per region: image %d" % i)


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
def test_process_files_and_the_cli_write_the_probed_words(pctx, e2e, tmp_path):
    imgs, plain, vocab, coarse, first, want = e2e
    paths = _copies(tmp_path)
    expect = [_want_words_file(tmp_path, plain[i][1], want[i], 300) for i in range(5)]
    _set(pctx, e2e)
    pctx.set_output_format(OUT_BIN | OUT_WORDS)
    try:
        st = pctx.process_files(paths)
    finally:
        pctx.set_output_format(1)
        pctx.set_vocabulary_probes(1)
    for i, p in enumerate(paths):
        assert st[i][0] == 0 and st[i][3] == E2E_KEYS[i]
        assert open(p + ".hesaff.words", "rb").read() == expect[i], p
        os.remove(p + ".hesaff.words")
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    hesaff_amd.write_vocabulary_cells(vfile + ".cells", coarse, first)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    r = subprocess.run([EXE, "--batch", str(lst), "--vocabulary", vfile, "--cells", vfile + ".cells", "--probes", "2", "--words-only"], capture_output=True,
                       text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    for i, p in enumerate(paths):
        assert open(p + ".hesaff.words", "rb").read() == expect[i], p
        os.remove(p + ".hesaff.words")
    r = subprocess.run([EXE, paths[0], "--vocabulary", vfile, "--cells", vfile + ".cells", "--probes", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert open(paths[0] + ".hesaff.words", "rb").read() == expect[0]
    # the C++ member: tests/native/vocabulary_probes_keys.cpp
    if shutil.which("g++") is None:
        return
    exe = str(tmp_path / "vocabulary_probes_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "vocabulary_probes_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, paths[0], vfile, vfile + ".cells", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip().split("\n") == ["P 2"] + ["W %d %d" % (w, d) for w, d in want[0]]
