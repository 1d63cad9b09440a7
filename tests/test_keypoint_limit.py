"""hesaff_set_keypoint_limit: per image, the N Hessian keypoints of greatest |response| are kept on the device, in the reference's
order, ties at the cut to the earlier keypoint (include/hesaff_amd.h).  Everything a kept keypoint becomes - its hesaff_region
record, its row of keys - is what the unlimited run makes of it, bit for bit; only `key` is renumbered.

Expected values come from the oracle's per-keypoint dumps (tests/golden/*_stages.npz, tests._oracle.OracleRun) and the one numpy
selection below, never from the limited path itself.  The CPU tests check the argument errors, the CLI's refusals and that
hesaff.hpp's setter compiles; the GPU tests (marked) the selection through every entry point."""
import ctypes as C
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from hesaff_amd.synth import band_noise_image
from tests.test_regions import check_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NATIVE_SRC = os.path.join(ROOT, "tests", "native", "keypoint_limit.cpp")
SMALL_BANDS = ((1.5, 40.0), (3.0, 40.0), (6.0, 50.0))
GOLDEN = ("band_96x96", "band_131x77", "band_160x120", "tiny_20x15", "thin_12x40")
GOLDEN_COUNTS = (154, 165, 354, 1, 0)


def select(response, n):
    """THE reference selection: indices of the n strongest keypoints, in list order; ties at the cut go to the earlier one."""
    return np.sort(np.argsort(-np.abs(np.asarray(response, np.float32)), kind="stable")[:n])


def select_signed(response, n):
    """what a selection that forgot the absolute value would keep"""
    return np.sort(np.argsort(-np.asarray(response, np.float32), kind="stable")[:n])


class Expect:
    """The per-keypoint dumps of one image (hess_f, hess_i, aff_U, aff_i, key_src) and its unlimited keys."""

    def __init__(self, hess_f, hess_i, aff_U, aff_i, key_src, keys):
        self.hf, self.hi, self.U, self.ai = hess_f, hess_i, aff_U, aff_i
        self.key_src = np.asarray(key_src, np.int64)
        self.keys = np.ascontiguousarray(keys, dtype=hesaff_amd.KEYPOINT_DTYPE)
        assert len(self.key_src) == len(self.keys) and (np.diff(self.key_src) > 0).all()
        self.n = len(hess_f)
        self.response = np.ascontiguousarray(hess_f[:, 4]) if self.n else np.zeros(0, np.float32)

    @classmethod
    def from_stages(cls, name, keys):
        st = np.load(os.path.join(GOLD, name + "_stages.npz"))
        return cls(st["hess_f"], st["hess_i"], st["aff_U"], st["aff_i"], st["key_src"], keys)

    @classmethod
    def from_oracle(cls, o):
        hf, hi = o.hessian()
        U, ai = o.affine()
        g, t, d = o.keys()
        keys = np.zeros(len(g), hesaff_amd.KEYPOINT_DTYPE)
        for j, name in enumerate(("x", "y", "s", "a11", "a12", "a21", "a22", "response")):
            keys[name] = g[:, j]
        keys["type"] = t
        keys["desc"] = d
        return cls(hf, hi, U, ai, o.key_sources(), keys)

    def subset(self, sel):
        """-> (hess_f, hess_i, aff_U, aff_i, key_src over the kept keypoints, keys rows of the kept, described keypoints)"""
        sel = np.asarray(sel, np.int64)
        described = np.isin(sel, self.key_src)
        return (self.hf[sel], self.hi[sel], self.U[sel], self.ai[sel], np.nonzero(described)[0],
                self.keys[np.searchsorted(self.key_src, sel[described])])

    def check(self, regions, keys, n_limit, what):
        """regions / keys of a limited run against the subset the reference selection names"""
        sel = select(self.response, n_limit)
        hf, hi, U, ai, src, want_keys = self.subset(sel)
        assert len(regions) == min(n_limit, self.n), (what, len(regions), n_limit, self.n)
        if len(sel):
            check_regions(regions, hf, hi, U, ai, src, what)
        assert len(keys) == len(want_keys), (what, len(keys), len(want_keys))
        assert keys.tobytes() == want_keys.tobytes(), what + ": key bytes differ from the unlimited keys of the selected keypoints"
        return sel


class limited:
    """`with limited(ctx, n):` - the limit on a shared context, 0 again afterwards"""

    def __init__(self, c, n):
        self.c, self.n = c, n

    def __enter__(self):
        self.c.set_keypoint_limit(self.n)
        return self.c

    def __exit__(self, *a):
        self.c.set_keypoint_limit(0)


def _golden_image(name):
    return hesaff_amd.read_pnm(os.path.join(GOLD, name + ".pgm"))


@functools.lru_cache(maxsize=None)
def _tiled_image():
    return np.tile(band_noise_image(48, 48, seed=7, bands=SMALL_BANDS), (2, 3))


_EXPECT = {}


def _oracle_expect(oracle, key, img):
    """Expect of an image by OracleRun, computed once per session"""
    if key not in _EXPECT:
        _EXPECT[key] = Expect.from_oracle(oracle.OracleRun(oracle.gray_from_u8(img)))
    return _EXPECT[key]


def _golden_expect(ctx):
    """Expect of the five golden fixtures: the committed stage dumps, keys from detect_batch at limit 0 (pinned to the fixtures by
    the existing tests), computed once per session"""
    if "golden" not in _EXPECT:
        assert ctx.keypoint_limit == 0
        batch = ctx.detect_batch([_golden_image(n) for n in GOLDEN])
        ex = [Expect.from_stages(n, keys) for n, (_, keys) in zip(GOLDEN, batch)]
        assert tuple(e.n for e in ex) == GOLDEN_COUNTS and tuple(nh for nh, _ in batch) == GOLDEN_COUNTS
        _EXPECT["golden"] = ex
    return _EXPECT["golden"]


def _tie_cuts(response):
    """-> (the N whose cut falls inside a group of bit-equal |response|, sizes of the tied groups, the N inside the largest group)"""
    a = np.abs(np.asarray(response, np.float32)).view(np.uint32)
    order = np.argsort(-a.astype(np.int64), kind="stable")
    s = a[order]
    cuts = [n for n in range(1, len(s)) if s[n - 1] == s[n]]
    vals, counts = np.unique(a, return_counts=True)
    groups = counts[counts > 1]
    big = vals[np.argmax(counts)]
    pos = np.nonzero(s == big)[0]   # ranks of the largest group's members: a cut after the first .. before the last is inside it
    return cuts, groups, [int(p) + 1 for p in pos[:-1]]


# ------------------------------------------------------------------ CPU ------------------------------------------------------------------

def test_setters_refuse_a_null_context():
    L = hesaff_amd.load_library()
    n = C.c_int(77)
    assert L.hesaff_set_keypoint_limit(None, 5) == -2
    assert L.hesaff_set_keypoint_limit(None, 0) == -2
    assert L.hesaff_set_keypoint_limit(None, -1) == -2
    assert L.hesaff_get_keypoint_limit(None, C.byref(n)) == -2 and n.value == 77
    assert "hesaff_set_keypoint_limit" in _binding.ABI_SYMBOLS and "hesaff_get_keypoint_limit" in _binding.ABI_SYMBOLS


@pytest.mark.parametrize("value", ["-1", "x", "", "12x", "99999999999"])
def test_cli_refuses_a_bad_limit_before_any_device(tmp_path, value):
    lst = tmp_path / "list.txt"
    lst.write_text("")
    r = subprocess.run([EXE, "--batch", str(lst), "--max-keypoints", value], capture_output=True, text=True)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stderr.startswith("hesaff: usage: hesaff --batch <list file>") and "[--max-keypoints N]" in r.stderr, r.stderr
    assert r.stdout == ""
    # the flag belongs to the batch form: without a value it is refused too
    assert subprocess.run([EXE, "--batch", str(lst), "--max-keypoints"], capture_output=True, text=True).returncode == 1


def test_single_image_usage_does_not_mention_the_flag():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0 and "max-keypoints" not in r.stdout


def test_set_keypoint_limit_interface_compiles():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", NATIVE_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_reference_selection_breaks_ties_towards_the_earlier_keypoint():
    r = np.array([1.0, -3.0, 3.0, 2.0, -3.0, 0.5], np.float32)
    assert select(r, 1).tolist() == [1] and select(r, 2).tolist() == [1, 2] and select(r, 3).tolist() == [1, 2, 4]
    assert select(r, 4).tolist() == [1, 2, 3, 4] and select(r, 100).tolist() == [0, 1, 2, 3, 4, 5] and select(r, 0).tolist() == []
    cuts, groups, inside = _tie_cuts(r)
    assert cuts == [1, 2] and groups.tolist() == [3] and inside == [1, 2]


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

GOLDEN_LIMITS = (1, 7, 153, 154, 155, 165, 353, 354, 355, 10 ** 6)


@pytest.mark.gpu
def test_golden_preconditions(ctx):
    """For every band image some tested N selects differently by |response| than by signed response: a sign bug cannot pass."""
    for name, e in zip(GOLDEN[:3], _golden_expect(ctx)[:3]):
        assert (e.response < 0).mean() > 0.5, name
        assert any(select(e.response, n).tolist() != select_signed(e.response, n).tolist() for n in GOLDEN_LIMITS), name


@pytest.mark.gpu
@pytest.mark.parametrize("n_limit", GOLDEN_LIMITS)
def test_golden_fixtures_mixed_sizes_one_call(ctx, n_limit):
    """The five golden fixtures (154, 165, 354, 1 and 0 Hessian keypoints; three octaves, all three types) in ONE detect_regions
    call: every record and every key byte of every image, and count_hessian == min(N, n)."""
    ex = _golden_expect(ctx)
    imgs = [_golden_image(n) for n in GOLDEN]
    with limited(ctx, n_limit):
        assert ctx.keypoint_limit == n_limit
        res = ctx.detect_regions(imgs)
        batch = ctx.detect_batch(imgs)
    assert ctx.keypoint_limit == 0
    for name, e, (regions, keys), (n_hess, keys_b) in zip(GOLDEN, ex, res, batch):
        e.check(regions, keys, n_limit, "%s N=%d" % (name, n_limit))
        assert n_hess == min(n_limit, e.n) and keys_b.tobytes() == keys.tobytes(), name


@pytest.mark.gpu
def test_ties_at_the_cut(ctx, oracle):
    """A 2 x 3 tiling repeats every keypoint away from the seams: groups of bit-equal |response|.  Every N whose cut falls inside
    such a group (the first 40) and every N inside the largest group: the earlier keypoints of the group are the ones kept."""
    img = _tiled_image()
    assert img.shape == (96, 144)
    e = _oracle_expect(oracle, "tiled", img)
    cuts, groups, inside_largest = _tie_cuts(e.response)
    print("tiled image: %d Hessian keypoints, %d tied groups, largest %d; cuts inside a group: %s ..." % (e.n, len(groups), groups.max(), cuts[:12]))
    assert len(groups) >= 10 and groups.max() >= 3
    limits = sorted(set(cuts[:40]) | set(inside_largest))
    assert len(limits) >= 10
    try:
        for n_limit in limits:
            ctx.set_keypoint_limit(n_limit)
            (regions, keys), = ctx.detect_regions([img])
            e.check(regions, keys, n_limit, "tiled N=%d" % n_limit)
    finally:
        ctx.set_keypoint_limit(0)


@pytest.fixture(scope="module")
def ctx_chunks():
    """a context of its own with max_batch = 2: lists split into chunks"""
    p = hesaff_amd.default_params(); p.max_batch = 2
    c = hesaff_amd.HesaffContext(p, device=0)
    yield c
    c.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n_limit", (1, 255, 256, 257, 1000, 4762, 4763))
def test_several_passes_per_image_and_chunk_boundaries(ctx_chunks, oracle, n_limit):
    """probe_vga (4763 Hessian keypoints, five octaves, no ties: several block-sized passes per image) in a list of alternating
    sizes through max_batch = 2, by detect_regions, detect_batch and detect_batch_cb; and alone through the device entry point."""
    import torch
    from tests.test_gpu_parity import _device_keys
    names = ("probe_vga", "band_160x120", "probe_vga", "tiny_20x15", "probe_vga")
    imgs = {n: _golden_image(n) for n in set(names)}
    ex = {n: _oracle_expect(oracle, n, imgs[n]) for n in imgs}
    assert ex["probe_vga"].n == 4763 and len(ex["probe_vga"].keys) == 4183 and len(_tie_cuts(ex["probe_vga"].response)[0]) == 0
    lst = [imgs[n] for n in names]
    c = ctx_chunks
    with limited(c, n_limit):
        res = c.detect_regions(lst)
        batch = c.detect_batch(lst)
        streamed = {}
        c.detect_batch_cb(lst, lambda idx, out: streamed.update(zip(idx, out)) and None)
        vga = imgs["probe_vga"]
        t = torch.from_numpy(vga[None]).cuda()
        ch, cd, dkeys, total = c.detect_batch_device(t.data_ptr(), 1, vga.shape[1], vga.shape[0])
        dev_keys = _device_keys(dkeys, total)
    assert sorted(streamed) == list(range(len(names)))
    for i, (name, (regions, keys), (n_hess, keys_b)) in enumerate(zip(names, res, batch)):
        what = "image %d (%s) N=%d" % (i, name, n_limit)
        ex[name].check(regions, keys, n_limit, what)
        assert n_hess == len(regions) and keys_b.tobytes() == keys.tobytes(), what + ": detect_batch"
        assert streamed[i][0] == n_hess and streamed[i][1].tobytes() == keys.tobytes(), what + ": detect_batch_cb"
    want = ex["probe_vga"].subset(select(ex["probe_vga"].response, n_limit))[5]
    assert int(ch[0]) == min(n_limit, 4763) and int(cd[0]) == total == len(want)
    assert dev_keys.tobytes() == want.tobytes(), "detect_batch_device N=%d" % n_limit


@pytest.mark.gpu
@pytest.mark.parametrize("n_limit", (10, 17, 100))
def test_float_planes(ctx, oracle, n_limit):
    """detect_regions_f32 on the grey plane of the tiled image: the records and keys of the 8-bit call with the same limit."""
    img = _tiled_image()
    e = _oracle_expect(oracle, "tiled", img)
    with limited(ctx, n_limit):
        (r8, k8), = ctx.detect_regions([img])
        (rf, kf), = ctx.detect_regions_f32([oracle.gray_from_u8(img)])
        (nf, kbf), = ctx.detect_batch_f32([oracle.gray_from_u8(img)])
    e.check(rf, kf, n_limit, "tiled f32 N=%d" % n_limit)
    assert rf.tobytes() == r8.tobytes() and kf.tobytes() == k8.tobytes() == kbf.tobytes() and nf == len(rf)


@pytest.mark.gpu
def test_limit_leaves_no_state_behind():
    """limit, run, 0, run: byte-identical to a context that never had a limit."""
    imgs = [_golden_image(n) for n in GOLDEN]
    with hesaff_amd.HesaffContext(device=0) as fresh:
        want = fresh.detect_regions(imgs)
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_keypoint_limit(7)
        lim = c.detect_regions(imgs)
        c.set_keypoint_limit(0)
        got = c.detect_regions(imgs)
    assert [len(r) for r, _ in lim] == [min(7, n) for n in GOLDEN_COUNTS]
    for (r, k), (rw, kw) in zip(got, want):
        assert r.tobytes() == rw.tobytes() and k.tobytes() == kw.tobytes()
    assert [len(r) for r, _ in got] == list(GOLDEN_COUNTS)


@pytest.mark.gpu
def test_describe_regions_and_stage_operators_are_not_limited(ctx):
    """With a limit of 5 set, describe_regions(FROM_POINTS) of all 354 unlimited records of band_160x120 returns 354 regions and the
    unlimited keys, and hesaff_stage_hessian_keypoints still returns all 354."""
    img = _golden_image("band_160x120")
    e = _golden_expect(ctx)[2]
    (r0, k0), = ctx.detect_regions([img])
    assert len(r0) == 354 and k0.tobytes() == e.keys.tobytes()
    with limited(ctx, 5):
        (r5, _), = ctx.detect_regions([img])
        (rd, kd), = ctx.describe_regions([img], [r0], hesaff_amd.FROM_POINTS)
        f, i, count = ctx.hessian_keypoints(img)
    assert len(r5) == 5
    assert len(rd) == 354 and rd.tobytes() == r0.tobytes() and kd.tobytes() == k0.tobytes()
    assert count == 354 and f[:, :5].view(np.uint32).tolist() == e.hf[:, :5].view(np.uint32).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(fast=2), dict(upscaleInputImage=1)], ids=lambda kw: ",".join("%s=%d" % kv for kv in kw.items()))
def test_other_parameter_sets(kw):
    """fast = 2 and upscaleInputImage = 1: with N = 50 the result is the subset, by the reference selection, of that context's own
    limit-0 detect_regions output (which the existing tests pin)."""
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    img = _golden_image("band_160x120")
    with hesaff_amd.HesaffContext(p, device=0) as c:
        (r0, k0), = c.detect_regions([img])
        c.set_keypoint_limit(50)
        (r, k), = c.detect_regions([img])
    assert len(r0) > 100
    sel = select(r0["response"], 50)
    want = r0[sel].copy()
    described = want["outcome"] == 2
    want_keys = k0[want["key"][described]]
    want["key"][described] = np.arange(int(described.sum()), dtype=np.int32)
    assert r.tobytes() == want.tobytes(), kw
    assert k.tobytes() == want_keys.tobytes() and 0 < len(k) <= 50, kw


@pytest.mark.gpu
def test_files_and_cli(ctx, tmp_path):
    """`hesaff --batch list --max-keypoints 40 --output both`: every .hesaff.sift is hesaff_format_sift of the expected keys, every
    .hesaff.bin hesaff_write_bin's bytes, and the counts on stdout are the expected ones."""
    ex = _golden_expect(ctx)[:3]
    paths = []
    for name in GOLDEN[:3]:
        paths.append(str(tmp_path / (name + ".pgm")))
        shutil.copy(os.path.join(GOLD, name + ".pgm"), paths[-1])
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    r = subprocess.run([EXE, "--batch", str(lst), "--max-keypoints", "40", "--output", "both"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(lines) == 4, r.stdout
    tot_d = 0
    for path, e, line in zip(paths, ex, lines):
        want = e.subset(select(e.response, 40))[5]
        assert 0 < len(want) < 40
        assert line == "%s: Detected 40 keypoints and %d affine shapes" % (path, len(want)), line
        assert open(path + ".hesaff.sift", "rb").read() == hesaff_amd.format_sift(want, ctx.params.mrSize), path
        ref_bin = str(tmp_path / "want.bin")
        hesaff_amd.write_bin(ref_bin, want, ctx.params.mrSize)
        assert open(path + ".hesaff.bin", "rb").read() == open(ref_bin, "rb").read(), path
        tot_d += len(want)
    assert re.fullmatch(r"Detected 120 keypoints and %d affine shapes in 3 images in [0-9.e+-]+ sec\." % tot_d, lines[3]), lines[3]


@pytest.mark.gpu
def test_cpp_detector_with_a_limit(ctx, tmp_path):
    """tests/native/keypoint_limit.cpp: setKeypointLimit(20) on band_96x96 with both callbacks installed - 20 Hessian callbacks, the
    selected keypoints' responses in order, and as many affine callbacks and keys as the fixture's dumps say for those 20."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "keypoint_limit")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, NATIVE_SRC, "-L" + lib_dir, "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, "20", os.path.join(GOLD, "band_96x96.pgm")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    e = _golden_expect(ctx)[0]
    sel = select(e.response, 20)
    n_affine = int(e.ai[sel, 0].sum())
    n_keys = int(np.isin(sel, e.key_src).sum())
    lines = r.stdout.strip().split("\n")
    assert [ln for ln in lines if ln.startswith("R ")] == ["R %08x" % v for v in e.response[sel].view(np.uint32)]
    assert lines[-2] == "C 20 %d" % n_affine and lines[-1] == "N 20 %d %d" % (n_keys, n_keys), lines[-2:]
    assert 0 < n_keys <= n_affine < 20
