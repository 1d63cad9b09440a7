"""hesaff_set_keypoint_grid: with a keypoint limit N, the N // (R * C) strongest eligible Hessian keypoints of every cell of an R x C
grid over the image are kept on the device, in the reference's order, ties at a cell's cut to the earlier keypoint
(include/hesaff_amd.h).  Everything a kept keypoint becomes - its hesaff_region record, its row of keys - is what the unlimited run
makes of it, bit for bit; only `key` is renumbered.

Expected values come from the oracle's per-keypoint dumps (tests/golden/*_stages.npz, tests._oracle.OracleRun) and the one numpy
reference of the rule below (`grid_cells`, `grid_select`), never from the limited path.  The CPU tests check the reference itself,
what the fixtures can tell apart (so that a wrong rule cannot pass the GPU tests), the cell arithmetic the device runs (a stand-alone
program under the host sanitizers), the argument errors and the CLI's refusals; the GPU tests (marked) the selection through every
entry point."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests.test_detection_mask import eligible, left_half, subset_of_own
from hesaff_amd.synth import band_noise_image
from tests.test_keypoint_limit import (GOLDEN, GOLDEN_COUNTS, SMALL_BANDS, Expect, _golden_expect, _golden_image, _oracle_expect,
                                       _tiled_image, select)
from tests.test_regions import check_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NATIVE_SRC = os.path.join(ROOT, "tests", "native", "keypoint_grid.cpp")
CELL_CHECK_SRC = os.path.join(ROOT, "tests", "native", "grid_cell_check.cpp")


# ------------------------------------------------------- THE reference of the rule -------------------------------------------------------

def pixels(v, size):
    """clamp((int)(v + 0.5f), 0, size - 1): the add in binary32, the conversion truncating (the masks' rule)"""
    return np.clip((np.asarray(v, np.float32) + np.float32(0.5)).astype(np.int32), 0, size - 1).astype(np.int64)


def grid_cells(x, y, W, H, R, C):
    """cell index cr * C + cc of every keypoint: cr = ((row + 1) * R - 1) // H, cc = ((col + 1) * C - 1) // W"""
    return ((pixels(y, H) + 1) * R - 1) // H * C + ((pixels(x, W) + 1) * C - 1) // W


def grid_select(response, cells, R, C, n, ok=None):
    """Indices, in list order, of the keypoints the rule keeps: of the eligible ones (ok; None: all) the n // (R * C) strongest of
    every cell, ties at a cell's cut to the earlier keypoint.  n = 0: every eligible keypoint; R * C = 1: the plain limit."""
    response = np.asarray(response, np.float32)
    idx = np.arange(len(response)) if ok is None else np.nonzero(ok)[0]
    if n == 0 or len(idx) == 0:
        return idx
    quota = n // (R * C)
    cells = np.asarray(cells)[idx]
    kept = [idx[cells == k][select(response[idx[cells == k]], quota)] for k in range(R * C)]
    return np.sort(np.concatenate(kept))


def cells_by_division(x, y, W, H, R, C):
    """what row * R / H would give"""
    return pixels(y, H) * R // H * C + pixels(x, W) * C // W


def cells_truncating(x, y, W, H, R, C):
    """what a rule that forgot the + 0.5 would give"""
    col = np.clip(np.asarray(x, np.float32).astype(np.int32), 0, W - 1).astype(np.int64)
    row = np.clip(np.asarray(y, np.float32).astype(np.int32), 0, H - 1).astype(np.int64)
    return ((row + 1) * R - 1) // H * C + ((col + 1) * C - 1) // W


def expect_kept(e, shape, R, C, n, mask=None):
    """list indices of Expect e's keypoints that the rule keeps on an image of `shape` (H, W)"""
    H, W = shape[:2]
    ok = None if mask is None else eligible(e.hf[:, 0], e.hf[:, 1], mask)
    return grid_select(e.response, grid_cells(e.hf[:, 0], e.hf[:, 1], W, H, R, C), R, C, n, ok)


def check_kept(e, regions, keys, idx, what):
    """regions / keys of a run against the keypoints idx of Expect e"""
    hf, hi, U, ai, src, want_keys = e.subset(idx)
    assert len(regions) == len(idx), (what, len(regions), len(idx))
    if len(idx):
        check_regions(regions, hf, hi, U, ai, src, what)
    assert len(keys) == len(want_keys), (what, len(keys), len(want_keys))
    assert keys.tobytes() == want_keys.tobytes(), what + ": key bytes differ from the unlimited keys of the kept keypoints"


class gridded:
    """`with gridded(ctx, R, C, n):` - limit and grid on a shared context, 0 and 1 x 1 again afterwards"""

    def __init__(self, c, R, C_, n):
        self.c, self.R, self.C, self.n = c, R, C_, n

    def __enter__(self):
        self.c.set_keypoint_limit(self.n)
        self.c.set_keypoint_grid(self.R, self.C)
        return self.c

    def __exit__(self, *a):
        self.c.set_keypoint_grid(1, 1)
        self.c.set_keypoint_limit(0)


def _stages(name):
    return np.load(os.path.join(GOLD, name + "_stages.npz"))


def _tie_quotas(response, cells, ncell):
    """the quotas Q whose cut falls, in some cell, inside a group of bit-equal |response|"""
    a = np.abs(np.asarray(response, np.float32)).view(np.uint32).astype(np.int64)
    out = set()
    for k in range(ncell):
        s = np.sort(a[cells == k])[::-1]
        out.update(q for q in range(1, len(s)) if s[q - 1] == s[q])
    return sorted(out)


# ------------------------------------------------------------------ CPU ------------------------------------------------------------------

GOLDEN_CASES = ((2, 3, 6), (2, 3, 30), (3, 5, 15), (3, 5, 75), (5, 7, 35), (8, 8, 64), (8, 8, 320), (1, 64, 64), (64, 1, 64), (4, 4, 10 ** 6))


def test_reference_on_a_hand_made_list():
    """Ties inside a cell, ties across cells, an empty cell, a clamped coordinate - on a 12 x 10 image under a 2 x 3 grid (cells of
    4 columns x 5 rows)."""
    W, H, R, C_ = 12, 10, 2, 3
    #            0     1     2     3     4     5     6     7     8      9    10
    x = [0.0, 3.49, 3.5, 5.0, 1.0, 11.0, 9.0, 2.0, 40.0, 6.0, 0.2]
    y = [0.0, 1.0, 4.49, 4.5, 2.0, 9.0, 7.0, 4.0, -3.0, 9.4, 3.0]
    r = [3.0, -3.0, 3.0, 5.0, -3.0, 1.0, -2.0, 7.0, 3.0, -5.0, 3.0]
    cells = grid_cells(x, y, W, H, R, C_)
    assert cells.tolist() == [0, 0, 1, 4, 0, 5, 5, 0, 2, 4, 0]          # 3.5 rounds into the next column of cells, 4.5 into the next row
    assert 3 not in cells                                               # an empty cell
    # cell 0 holds 0, 1, 4, 7, 10 with |r| = 3, 3, 3, 7, 3: the cut of Q = 2 and Q = 3 falls inside the tie, the earlier ones win
    assert grid_select(r, cells, R, C_, 6).tolist() == [2, 3, 6, 7, 8]            # Q = 1: the strongest of every occupied cell
    assert grid_select(r, cells, R, C_, 12).tolist() == [0, 2, 3, 5, 6, 7, 8, 9]  # Q = 2: 7 and the first 3.0 of cell 0
    assert grid_select(r, cells, R, C_, 18).tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 9]
    assert grid_select(r, cells, R, C_, 23).tolist() == [0, 1, 2, 3, 5, 6, 7, 8, 9]   # integer division: still Q = 3
    assert grid_select(r, cells, R, C_, 24).tolist() == [0, 1, 2, 3, 4, 5, 6, 7, 8, 9]
    assert grid_select(r, cells, R, C_, 10 ** 6).tolist() == list(range(11))
    # the tie across cells (3.0 in cells 0, 1 and 2) is no tie: every cell has its own cut; unused quota is not handed on
    assert len(grid_select(r, cells, R, C_, 12)) == 8 < 12
    # a mask first: without keypoints 7 and 0 the first 3.0 left in cell 0 is keypoint 1
    ok = np.ones(11, bool); ok[[0, 7]] = False
    assert grid_select(r, cells, R, C_, 6, ok).tolist() == [1, 2, 3, 6, 8]
    # no limit: the grid is inert; one cell: the plain limit
    assert grid_select(r, cells, R, C_, 0).tolist() == list(range(11)) and grid_select(r, cells, R, C_, 0, ok).tolist() == [1, 2, 3, 4, 5, 6, 8, 9, 10]
    assert grid_select(r, np.zeros(11, int), 1, 1, 4).tolist() == select(r, 4).tolist() == [0, 3, 7, 9]
    # the cell ranges are OpenCV's: 77 rows in 4 cells are [0, 19) [19, 38) [38, 57) [57, 77), which row * 4 // 77 does not give
    rows = np.arange(77)
    cr = ((rows + 1) * 4 - 1) // 77
    assert [int(np.nonzero(cr == k)[0][0]) for k in range(4)] == [0 * 77 // 4, 1 * 77 // 4, 2 * 77 // 4, 3 * 77 // 4] == [0, 19, 38, 57]
    assert (cr != rows * 4 // 77).sum() == 3


def test_fixture_preconditions():
    """What the committed dumps can tell apart, so that a wrong rule cannot pass the GPU tests: on band_131x77 and band_96x96, under
    the tested grids 3 x 5 and 5 x 7, the range rule puts keypoints into other cells than row * R / H, rounding into other cells
    than truncating, the grid with rows and columns swapped selects differently, and for every tested N of those grids the kept set
    differs from the global top-K of the same size."""
    facts = {}
    for name in ("band_131x77", "band_96x96"):
        hf = _stages(name)["hess_f"]
        H, W = _golden_image(name).shape
        x, y, r = hf[:, 0], hf[:, 1], hf[:, 4]
        for R, C_, n in GOLDEN_CASES:
            cells = grid_cells(x, y, W, H, R, C_)
            kept = grid_select(r, cells, R, C_, n)
            by_div = int((cells != cells_by_division(x, y, W, H, R, C_)).sum())
            trunc = int((cells != cells_truncating(x, y, W, H, R, C_)).sum())
            swapped = R * C_ <= 64 and grid_select(r, grid_cells(x, y, W, H, C_, R), C_, R, n).tolist() != kept.tolist()
            not_top = kept.tolist() != select(r, len(kept)).tolist()
            facts[name, R, C_, n] = (len(kept), by_div, trunc, swapped, not_top)
            if (R, C_) in ((3, 5), (5, 7)):
                assert by_div >= 1 and trunc >= 1 and swapped and not_top and 0 < len(kept) < len(r), (name, R, C_, n, facts[name, R, C_, n])
    print(facts)
    assert facts["band_131x77", 3, 5, 15][:3] == (15, 7, 6) and facts["band_131x77", 5, 7, 35][:3] == (34, 17, 11)
    assert facts["band_96x96", 3, 5, 75][1:3] == (8, 6) and facts["band_96x96", 5, 7, 35][1:3] == (19, 10)
    # the issue's figure: band_131x77 under 4 x 4, 14 of 165 keypoints change cell between the two rules
    hf = _stages("band_131x77")["hess_f"]
    assert int((grid_cells(hf[:, 0], hf[:, 1], 131, 77, 4, 4) != cells_by_division(hf[:, 0], hf[:, 1], 131, 77, 4, 4)).sum()) == 14 and len(hf) == 165
    # and band_160x120 at N = 80 under 4 x 4 against the global top-80: 17 in, 17 out
    hf = _stages("band_160x120")["hess_f"]
    kept = grid_select(hf[:, 4], grid_cells(hf[:, 0], hf[:, 1], 160, 120, 4, 4), 4, 4, 80)
    assert len(kept) == 80 and len(set(kept.tolist()) ^ set(select(hf[:, 4], 80).tolist())) == 34


def test_cell_arithmetic_under_sanitizers(tmp_path):
    """tests/native/grid_cell_check.cpp, a stand-alone program under AddressSanitizer + UBSan: the device's cell function
    (hesaff_amd/csrc/select_grid.h) for every col of every W in 1..300 and W = 65535 and every C in 1..64 - c*W/C <= col < (c+1)*W/C,
    monotone, no intermediate outside int32."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "grid_cell_check")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                        "-fno-omit-frame-pointer", "-o", exe, CELL_CHECK_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ, UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    want = sum(range(1, 301)) * 64 + 65535 * 64
    assert r.stdout.strip() == "checked=%d differ_77_4=3 ok" % want, r.stdout


def test_entry_points_refuse_a_null_context():
    L = hesaff_amd.load_library()
    r, c = C.c_int(77), C.c_int(78)
    assert L.hesaff_set_keypoint_grid(None, 2, 3) == -2 and L.hesaff_set_keypoint_grid(None, 1, 1) == -2
    assert L.hesaff_set_keypoint_grid(None, 0, 0) == -2
    assert L.hesaff_get_keypoint_grid(None, C.byref(r), C.byref(c)) == -2 and (r.value, c.value) == (77, 78)
    assert L.hesaff_get_keypoint_grid(None, None, None) == -2
    assert "hesaff_set_keypoint_grid" in _binding.ABI_SYMBOLS and "hesaff_get_keypoint_grid" in _binding.ABI_SYMBOLS
    assert L.hesaff_abi_version() == _binding.ABI_VERSION == 8


@pytest.mark.parametrize("args", [["--max-keypoints", "60", "--grid", v] for v in ("", "x", "2", "2x", "x3", "0x3", "3x0", "-2x3", "2x3x", "2x3 ", "2X3", "9x9",
                                                                                   "65x1", "1x65", "99999999999x1", "2.0x3")]
                         + [["--grid", "2x3"], ["--grid", "2x3", "--max-keypoints", "0"], ["--max-keypoints", "5", "--grid", "2x3"],
                            ["--grid", "8x8", "--max-keypoints", "63"], ["--max-keypoints", "60", "--grid"]],
                         ids=lambda a: " ".join(a))
def test_cli_refuses_a_bad_grid_before_any_device(tmp_path, args):
    lst = tmp_path / "list.txt"
    lst.write_text(os.path.join(GOLD, "band_96x96.pgm") + "\n")
    r = subprocess.run([EXE, "--batch", str(lst)] + args, capture_output=True, text=True)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stderr.startswith("hesaff: usage: hesaff --batch <list file>") and r.stderr.rstrip().endswith("[--orientation up|dominant] [--grid RxC]"), r.stderr
    assert r.stdout == ""
    assert not os.path.exists(os.path.join(GOLD, "band_96x96.pgm.hesaff.sift"))


def test_single_image_usage_does_not_mention_the_flag():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0 and "grid" not in r.stdout


def test_set_keypoint_grid_interface_compiles():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", NATIVE_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(NATIVE_SRC).read()
    assert "setKeypointGrid(" in src and "setKeypointLimit(" in src and "setHessianKeypointCallback" in src and "setAffineShapeCallback" in src


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("R,C_,n", GOLDEN_CASES, ids=lambda v: str(v))
def test_golden_fixtures_mixed_sizes_one_call(ctx, R, C_, n):
    """The five golden fixtures (154, 165, 354, 1 and 0 Hessian keypoints; thin_12x40 is narrower than a 64-column grid) in ONE
    detect_regions call, detect_batch beside it: every record, every key byte and count_hessian."""
    ex = _golden_expect(ctx)
    imgs = [_golden_image(name) for name in GOLDEN]
    with gridded(ctx, R, C_, n):
        assert ctx.keypoint_limit == n and ctx.keypoint_grid == (R, C_)
        res = ctx.detect_regions(imgs)
        batch = ctx.detect_batch(imgs)
    assert ctx.keypoint_limit == 0 and ctx.keypoint_grid == (1, 1)
    counts = []
    for name, img, e, (regions, keys), (n_hess, keys_b) in zip(GOLDEN, imgs, ex, res, batch):
        idx = expect_kept(e, img.shape, R, C_, n)
        check_kept(e, regions, keys, idx, "%s %dx%d N=%d" % (name, R, C_, n))
        assert n_hess == len(idx) <= n // (R * C_) * R * C_ and keys_b.tobytes() == keys.tobytes(), name
        counts.append(n_hess)
    assert counts[3:] == [1, 0] and (counts == list(GOLDEN_COUNTS)) == (n == 10 ** 6), counts


@pytest.mark.gpu
@pytest.mark.parametrize("n", (1, 7, 154, 10 ** 6))
def test_one_by_one_grid_is_the_plain_limit(ctx, n):
    """set_keypoint_grid(1, 1) with a limit: the bytes of the limit alone (which tests/test_keypoint_limit.py pins)."""
    imgs = [_golden_image(name) for name in GOLDEN]
    ctx.set_keypoint_limit(n)
    try:
        want = ctx.detect_regions(imgs)
        ctx.set_keypoint_grid(1, 1)
        got = ctx.detect_regions(imgs)
    finally:
        ctx.set_keypoint_limit(0)
    assert [len(r) for r, _ in want] == [min(n, c) for c in GOLDEN_COUNTS]
    for (r, k), (rw, kw) in zip(got, want):
        assert r.tobytes() == rw.tobytes() and k.tobytes() == kw.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("R,C_,n_quotas", ((1, 3, 42), (2, 1, 101), (1, 2, 64)), ids=("1x3", "2x1", "1x2"))
def test_ties_at_a_cells_cut(ctx, oracle, R, C_, n_quotas):
    """The 2 x 3 tiling of a 48 x 48 image repeats every keypoint away from the seams; grids 1 x 3, 2 x 1 and 1 x 2 hold several
    copies per cell, so cells have groups of bit-equal |response|.  For the first 15 quotas Q whose cut falls inside such a group
    in some cell, with N = Q * R * C: the earlier keypoints of the group are the ones kept."""
    img = _tiled_image()
    assert img.shape == (96, 144)
    e = _oracle_expect(oracle, "tiled", img)
    cells = grid_cells(e.hf[:, 0], e.hf[:, 1], 144, 96, R, C_)
    quotas = _tie_quotas(e.response, cells, R * C_)
    print("tiled image, %d x %d: %d keypoints %s per cell, %d quotas cut a tied group: %s ..." % (R, C_, e.n, np.bincount(cells).tolist(), len(quotas), quotas[:15]))
    assert len(quotas) == n_quotas
    try:
        for q in quotas[:15]:
            ctx.set_keypoint_limit(q * R * C_)
            ctx.set_keypoint_grid(R, C_)
            (regions, keys), = ctx.detect_regions([img])
            idx = expect_kept(e, img.shape, R, C_, q * R * C_)
            # the cut is inside a tie: some dropped keypoint has the |response| bits of a kept one of its cell
            dropped = np.setdiff1d(np.arange(e.n), idx)
            a = np.abs(e.response).view(np.uint32)
            assert any(((a[idx] == a[d]) & (cells[idx] == cells[d]) & (idx < d)).any() for d in dropped), q
            check_kept(e, regions, keys, idx, "tiled %dx%d Q=%d" % (R, C_, q))
    finally:
        ctx.set_keypoint_grid(1, 1)
        ctx.set_keypoint_limit(0)


@pytest.mark.gpu
def test_ties_across_the_chunks_of_a_segment(ctx, oracle):
    """A 3 x 3 tiling of an 80 x 80 image has 1123 keypoints - two 1024-keypoint chunks of the ordered pass - and copies of one
    keypoint on both sides of the chunk boundary.  Under 1 x 2, for the first 10 quotas at which a cell's cut falls between two
    bit-equal keypoints of different chunks: the count of threshold keys carried from the first chunk decides, and the earlier
    keypoint is the one kept."""
    img = np.tile(band_noise_image(80, 80, seed=11, bands=SMALL_BANDS), (3, 3))
    e = _oracle_expect(oracle, "tiled 3x3", img)
    assert e.n == 1123
    cells = grid_cells(e.hf[:, 0], e.hf[:, 1], 240, 240, 1, 2)
    a = np.abs(e.response).view(np.uint32)
    tested = 0
    try:
        for q in _tie_quotas(e.response, cells, 2):
            idx = expect_kept(e, img.shape, 1, 2, 2 * q)
            dropped = np.setdiff1d(np.arange(e.n), idx)
            if not any(((a[idx] == a[d]) & (cells[idx] == cells[d]) & (idx // 1024 < d // 1024)).any() for d in dropped):
                continue
            ctx.set_keypoint_limit(2 * q)
            ctx.set_keypoint_grid(1, 2)
            (regions, keys), = ctx.detect_regions([img])
            check_kept(e, regions, keys, idx, "3 x 3 tiling, 1x2 Q=%d" % q)
            tested += 1
            if tested == 10:
                break
    finally:
        ctx.set_keypoint_grid(1, 1)
        ctx.set_keypoint_limit(0)
    assert tested == 10


@pytest.fixture(scope="module")
def ctx_chunks():
    """a context of its own with max_batch = 2: lists split into chunks"""
    p = hesaff_amd.default_params(); p.max_batch = 2
    c = hesaff_amd.HesaffContext(p, device=0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("q", (1, 255, 256, 257, 1023, 1024, 1025))
@pytest.mark.parametrize("R,C_", ((1, 2), (2, 3), (8, 8)), ids=("1x2", "2x3", "8x8"))
def test_long_segments_and_chunk_boundaries(ctx_chunks, oracle, R, C_, q):
    """probe_vga (4763 Hessian keypoints: several 1024-keypoint chunks of the ordered pass per image; about 2400 per cell of 1 x 2,
    so a cell's carried count crosses chunks) in a list of alternating sizes through max_batch = 2, by detect_regions, detect_batch
    and detect_batch_cb; and alone through the device entry point."""
    import torch
    from tests.test_gpu_parity import _device_keys
    names = ("probe_vga", "band_160x120", "probe_vga", "tiny_20x15", "probe_vga")
    imgs = {name: _golden_image(name) for name in set(names)}
    ex = {name: _oracle_expect(oracle, name, imgs[name]) for name in imgs}
    assert ex["probe_vga"].n == 4763
    lst = [imgs[name] for name in names]
    n = q * R * C_
    c = ctx_chunks
    with gridded(c, R, C_, n):
        res = c.detect_regions(lst)
        batch = c.detect_batch(lst)
        streamed = {}
        c.detect_batch_cb(lst, lambda idx, out: streamed.update(zip(idx, out)) and None)
        vga = imgs["probe_vga"]
        t = torch.from_numpy(vga[None]).cuda()
        ch, cd, dkeys, total = c.detect_batch_device(t.data_ptr(), 1, vga.shape[1], vga.shape[0])
        dev_keys = _device_keys(dkeys, total)
    assert sorted(streamed) == list(range(len(names)))
    kept = {name: expect_kept(ex[name], imgs[name].shape, R, C_, n) for name in imgs}
    for i, (name, (regions, keys), (n_hess, keys_b)) in enumerate(zip(names, res, batch)):
        what = "image %d (%s) %dx%d Q=%d" % (i, name, R, C_, q)
        check_kept(ex[name], regions, keys, kept[name], what)
        assert n_hess == len(regions) and keys_b.tobytes() == keys.tobytes(), what + ": detect_batch"
        assert streamed[i][0] == n_hess and streamed[i][1].tobytes() == keys.tobytes(), what + ": detect_batch_cb"
    want = ex["probe_vga"].subset(kept["probe_vga"])[5]
    assert int(ch[0]) == len(kept["probe_vga"]) and int(cd[0]) == total == len(want)
    assert dev_keys.tobytes() == want.tobytes(), "detect_batch_device %dx%d Q=%d" % (R, C_, q)


def _triangle(shape):
    """non-zero on and above the diagonal of the image: whole cells of a grid empty, the cells on the diagonal cut"""
    H, W = shape[:2]
    r, c = np.indices((H, W))
    return ((c >= r * W // H) * 255).astype(np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("n", (16, 64, 160, 10 ** 6))
def test_masks_compose(ctx, n):
    """band_160x120 under a 4 x 4 grid with the left-half mask (the right eight cells empty) and with a triangle (six cells empty,
    four cut), in one call beside the unmasked image: mask first, then the grid, against the reference over the eligible keypoints."""
    e = _golden_expect(ctx)[2]
    img = _golden_image("band_160x120")
    masks = [left_half(img.shape), _triangle(img.shape), None]
    cells = grid_cells(e.hf[:, 0], e.hf[:, 1], 160, 120, 4, 4)
    per_cell = [np.bincount(cells[eligible(e.hf[:, 0], e.hf[:, 1], m)], minlength=16) for m in masks[:2]]
    full = np.bincount(cells, minlength=16)
    assert (per_cell[0] == 0).sum() == 8 and (per_cell[1] == 0).sum() >= 3 and ((per_cell[1] > 0) & (per_cell[1] < full)).sum() >= 3
    with gridded(ctx, 4, 4, n):
        res = ctx.detect_regions([img] * 3, masks=masks)
        batch = ctx.detect_batch([img] * 3, masks=masks)
    for m, (regions, keys), (n_hess, keys_b) in zip(masks, res, batch):
        idx = expect_kept(e, img.shape, 4, 4, n, m)
        check_kept(e, regions, keys, idx, "band_160x120 4x4 N=%d" % n)
        assert n_hess == len(idx) and keys_b.tobytes() == keys.tobytes()
    if n == 64:   # the mask acts first: not the masked subset of the unmasked grid selection
        ok = eligible(e.hf[:, 0], e.hf[:, 1], masks[1])
        unmasked_then_mask = [i for i in expect_kept(e, img.shape, 4, 4, n) if ok[i]]
        assert unmasked_then_mask != expect_kept(e, img.shape, 4, 4, n, masks[1]).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("R,C_,n", ((2, 3, 60), (1, 3, 51)))
def test_float_planes(ctx, oracle, R, C_, n):
    """detect_regions_f32 on the grey plane of the tiled image: the records and keys of the 8-bit call with the same grid."""
    img = _tiled_image()
    e = _oracle_expect(oracle, "tiled", img)
    with gridded(ctx, R, C_, n):
        (r8, k8), = ctx.detect_regions([img])
        (rf, kf), = ctx.detect_regions_f32([oracle.gray_from_u8(img)])
        (nf, kbf), = ctx.detect_batch_f32([oracle.gray_from_u8(img)])
    check_kept(e, rf, kf, expect_kept(e, img.shape, R, C_, n), "tiled f32 %dx%d N=%d" % (R, C_, n))
    assert rf.tobytes() == r8.tobytes() and kf.tobytes() == k8.tobytes() == kbf.tobytes() and nf == len(rf)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(fast=2), dict(upscaleInputImage=1)], ids=lambda kw: ",".join("%s=%d" % kv for kv in kw.items()))
def test_other_parameter_sets(kw):
    """fast = 2 and upscaleInputImage = 1 (the grid lies over the image at the caller's size): with N = 60 under 3 x 5 the result
    is the subset, by the reference, of that context's own unlimited detect_regions output (which the existing tests pin)."""
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    img = _golden_image("band_160x120")
    H, W = img.shape
    with hesaff_amd.HesaffContext(p, device=0) as c:
        (r0, k0), = c.detect_regions([img])
        c.set_keypoint_limit(60)
        c.set_keypoint_grid(3, 5)
        (r, k), = c.detect_regions([img])
    assert len(r0) > 100
    idx = grid_select(r0["response"], grid_cells(r0["x"], r0["y"], W, H, 3, 5), 3, 5, 60)
    want, want_keys = subset_of_own(r0, k0, idx)
    assert 30 < len(idx) <= 60 and idx.tolist() != select(r0["response"], len(idx)).tolist()
    assert r.tobytes() == want.tobytes(), kw
    assert k.tobytes() == want_keys.tobytes() and 0 < len(k) <= 60, kw


@pytest.mark.gpu
def test_setters_are_consistent_on_a_live_context(ctx):
    """The grid is refused when 0 < N < R * C, the limit under a set grid likewise, out-of-range grids always; a refused call
    changes nothing; a grid with limit 0 gives the unlimited bytes."""
    L, h = ctx.L, ctx.h
    img = _golden_image("band_160x120")
    e = _golden_expect(ctx)[2]
    state = lambda: (ctx.keypoint_limit, ctx.keypoint_grid)
    assert state() == (0, (1, 1))
    try:
        for rows, cols in ((0, 1), (1, 0), (-1, -1), (65, 1), (1, 65), (8, 9), (9, 8), (2 ** 16, 2 ** 16), (2 ** 31 - 1, 2)):
            assert L.hesaff_set_keypoint_grid(h, rows, cols) == -2 and state() == (0, (1, 1)), (rows, cols)
        r = C.c_int(5)
        assert L.hesaff_get_keypoint_grid(h, None, C.byref(r)) == -2 and L.hesaff_get_keypoint_grid(h, C.byref(r), None) == -2 and r.value == 5
        # limit first, then a grid with more cells than it
        ctx.set_keypoint_limit(10)
        assert L.hesaff_set_keypoint_grid(h, 3, 4) == -2 and state() == (10, (1, 1))
        with pytest.raises(hesaff_amd.HesaffError) as err:
            ctx.set_keypoint_grid(4, 4)
        assert err.value.code == -2 and state() == (10, (1, 1))
        ctx.set_keypoint_grid(2, 5)
        assert state() == (10, (2, 5))
        # the limit under a set grid: below the cells refused, 0 and >= cells accepted
        assert L.hesaff_set_keypoint_limit(h, 9) == -2 and L.hesaff_set_keypoint_limit(h, 1) == -2 and L.hesaff_set_keypoint_limit(h, -1) == -2
        assert state() == (10, (2, 5))
        (regions, keys), = ctx.detect_regions([img])
        check_kept(e, regions, keys, expect_kept(e, img.shape, 2, 5, 10), "after the refusals")
        ctx.set_keypoint_limit(0)
        assert state() == (0, (2, 5))
        # limit 0: any grid may be set, and it is inert
        ctx.set_keypoint_grid(8, 8)
        (regions, keys), = ctx.detect_regions([img])
        assert len(regions) == 354 and keys.tobytes() == e.keys.tobytes()
        check_kept(e, regions, keys, np.arange(354), "limit 0 under 8 x 8")
        assert L.hesaff_set_keypoint_limit(h, 63) == -2 and state() == (0, (8, 8))
        ctx.set_keypoint_limit(64)
        assert state() == (64, (8, 8))
    finally:
        ctx.set_keypoint_grid(1, 1)
        ctx.set_keypoint_limit(0)
    assert state() == (0, (1, 1))


@pytest.mark.gpu
def test_grid_leaves_no_state_behind():
    """grid and limit, run, 1 x 1 and 0, run: byte-identical to a context that never had either."""
    imgs = [_golden_image(name) for name in GOLDEN]
    with hesaff_amd.HesaffContext(device=0) as fresh:
        want = fresh.detect_regions(imgs)
    with hesaff_amd.HesaffContext(device=0) as c:
        assert c.keypoint_grid == (1, 1)
        c.keypoint_limit = 30
        c.keypoint_grid = (2, 3)
        lim = c.detect_regions(imgs)
        c.set_keypoint_grid(1, 1)
        c.set_keypoint_limit(0)
        got = c.detect_regions(imgs)
    assert [len(r) for r, _ in lim] == [30, 30, 30, 1, 0]
    for (r, k), (rw, kw) in zip(got, want):
        assert r.tobytes() == rw.tobytes() and k.tobytes() == kw.tobytes()
    assert [len(r) for r, _ in got] == list(GOLDEN_COUNTS)


@pytest.mark.gpu
def test_describe_regions_and_stage_operators_are_not_gridded(ctx):
    """With limit 16 under a 4 x 4 grid, describe_regions(FROM_POINTS) of all 354 unlimited records of band_160x120 returns 354
    regions and the unlimited keys, and hesaff_stage_hessian_keypoints still returns all 354."""
    img = _golden_image("band_160x120")
    e = _golden_expect(ctx)[2]
    (r0, k0), = ctx.detect_regions([img])
    assert len(r0) == 354 and k0.tobytes() == e.keys.tobytes()
    with gridded(ctx, 4, 4, 16):
        (rg, _), = ctx.detect_regions([img])
        (rd, kd), = ctx.describe_regions([img], [r0], hesaff_amd.FROM_POINTS)
        f, i, count = ctx.hessian_keypoints(img)
    assert len(rg) == 16
    assert len(rd) == 354 and rd.tobytes() == r0.tobytes() and kd.tobytes() == k0.tobytes()
    assert count == 354 and f[:, :5].view(np.uint32).tolist() == e.hf[:, :5].view(np.uint32).tolist()


@pytest.mark.gpu
def test_files_and_cli(ctx, tmp_path):
    """`hesaff --batch list --max-keypoints 60 --grid 2x3 --output both`: every .hesaff.sift is hesaff_format_sift of the expected
    keys, every .hesaff.bin hesaff_write_bin's bytes, and the counts on stdout are the expected ones."""
    ex = _golden_expect(ctx)[:3]
    paths = []
    for name in GOLDEN[:3]:
        paths.append(str(tmp_path / (name + ".pgm")))
        shutil.copy(os.path.join(GOLD, name + ".pgm"), paths[-1])
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    r = subprocess.run([EXE, "--batch", str(lst), "--max-keypoints", "60", "--grid", "2x3", "--output", "both"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 4, r.stdout
    tot_d = 0
    for name, path, e, line in zip(GOLDEN, paths, ex, lines):
        idx = expect_kept(e, _golden_image(name).shape, 2, 3, 60)
        want = e.subset(idx)[5]
        assert len(idx) == 60 and 0 < len(want) < 60 and idx.tolist() != select(e.response, 60).tolist()
        assert line == "%s: Detected 60 keypoints and %d affine shapes" % (path, len(want)), line
        assert open(path + ".hesaff.sift", "rb").read() == hesaff_amd.format_sift(want, ctx.params.mrSize), path
        ref_bin = str(tmp_path / "want.bin")
        hesaff_amd.write_bin(ref_bin, want, ctx.params.mrSize)
        assert open(path + ".hesaff.bin", "rb").read() == open(ref_bin, "rb").read(), path
        tot_d += len(want)
    assert re.fullmatch(r"Detected 180 keypoints and %d affine shapes in 3 images in [0-9.e+-]+ sec\." % tot_d, lines[3]), lines[3]


@pytest.mark.gpu
def test_cpp_detector_with_a_grid(ctx, tmp_path):
    """tests/native/keypoint_grid.cpp: setKeypointLimit(24) and setKeypointGrid(2, 3) on band_131x77 with both callbacks installed -
    the selected keypoints' responses in order, and as many affine callbacks and keys as the fixture's dumps say for them."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "keypoint_grid")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, NATIVE_SRC, "-L" + lib_dir, "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, "24", "2", "3", os.path.join(GOLD, "band_131x77.pgm")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    e = _golden_expect(ctx)[1]
    idx = expect_kept(e, (77, 131), 2, 3, 24)
    assert len(idx) == 24 and idx.tolist() != select(e.response, 24).tolist()
    n_affine = int(e.ai[idx, 0].sum())
    n_keys = int(np.isin(idx, e.key_src).sum())
    lines = r.stdout.strip().split("\n")
    assert [ln for ln in lines if ln.startswith("R ")] == ["R %08x" % v for v in e.response[idx].view(np.uint32)]
    assert lines[-2] == "C 24 %d" % n_affine and lines[-1] == "N 24 %d %d" % (n_keys, n_keys), lines[-2:]
    assert 0 < n_keys <= n_affine < 24
    # the setter's refusals reach the caller as std::invalid_argument: more cells than the limit
    r = subprocess.run([exe, "5", "2", "3", os.path.join(GOLD, "band_131x77.pgm")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and r.stderr.startswith("keypoint_grid: keypoint grid needs"), (r.stdout, r.stderr)
