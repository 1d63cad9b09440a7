"""The descriptor chain after k_sift_quantize was folded into k_sift_hist, and the group pipeline's order of submission.

CPU half (no mark): the oracle alone proves that the constructed patches hit what they claim (a clipped histogram next to an
unclipped one, an all-zero vector), and form_groups that the batch of the rotation test wraps the three patch slots.
GPU half (pytest.mark.gpu): the patches through the production kernels (hesaff_stage_sift, hesaff_stage_sift_alive) against the
oracle's descriptor stage, every byte; batches whose groups wrap the slots, and a batch that ends in a single small group, against
the same images run one per call, every record byte.  (Inside one batch the greedy form_groups never leaves a small image a group of
its own, so that case is the mixed-size host call, where the small image is a batch of its own.)"""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import stage_inputs as si

gpu = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_BIN = F(0.2)   # the default hesaff_params.maxBinValue (siftdesc.h:27)


# ----------------------------------------------------------------------------------------------------------------------
# the nine patches
# ----------------------------------------------------------------------------------------------------------------------

def _first_normalize_vec(hist):
    """siftdesc.cpp:83-96 in float32: sequential sum of squares, 1.0f / sqrt, product."""
    s = F(0)
    for x in hist:
        s = F(s + F(x * x))
    with np.errstate(divide="ignore", invalid="ignore"):
        fac = F(F(1) / np.sqrt(s))
        return (hist * fac).astype(F)


@functools.lru_cache(maxsize=None)
def _candidates():
    """(patches, oracle histograms, oracle bytes, clipped flags) of the ordinary and saturating families and the constant 77."""
    from tests import _oracle
    oh = _oracle.OracleHandle()
    flat_names = si.flat_names()
    const = si.flat()[flat_names.index("const:77.0")]
    patches = np.concatenate([si.ordinary()[:40], si.saturating(), const[None]])
    res = [oh.sift_parts(p) for p in patches]
    hist = np.stack([r[1] for r in res]); desc = np.stack([r[2] for r in res])
    with np.errstate(invalid="ignore"):
        clipped = np.array([bool((_first_normalize_vec(h) > MAX_BIN).any()) for h in hist])
    return patches, hist, desc, clipped


@functools.lru_cache(maxsize=None)
def nine():
    """Nine patches and the oracle's bytes: [0] clips, [1] does not, [2] is constant (vector all zero), then clipped and unclipped
    ones in turn; a wavefront of k_sift_hist (four keypoints) thus always holds both kinds."""
    patches, hist, desc, clipped = _candidates()
    zero = len(patches) - 1
    yes = [i for i in np.flatnonzero(clipped) if i != zero]
    no = [i for i in np.flatnonzero(~clipped) if i != zero and hist[i].any()]
    assert len(yes) >= 4 and len(no) >= 4, (len(yes), len(no))
    idx = [yes[0], no[0], zero, yes[1], no[1], yes[2], no[2], yes[3], no[3]]
    p = patches[idx].copy(); d = desc[idx].copy(); c = clipped[idx].copy()
    for a in (p, d, c):
        a.setflags(write=False)
    return p, d, c


def test_the_nine_patches_hit_what_they_claim():
    """[0] has a bin above maxBinValue after the first normalizeVec (the `changed` path): the clipped bins are 0.2 times a second factor
    of at least 1, so some byte is at least (int)(512 * 0.2) = 102.  [1] has none: it is only scaled, no byte above 102.  [2] has an
    all-zero histogram, whose norm is 0: 0 * inf = NaN in every bin, and the reference's NaN test yields all-zero bytes."""
    patches, hist, desc, clipped = _candidates()
    p, d, c = nine()
    assert c.tolist() == [True, False, False, True, False, True, False, True, False]
    zero = len(patches) - 1
    assert not hist[zero].any() and not d[2].any()
    assert d[0].max() >= 102 and d[0].any() and d[1].any()
    assert d[1].max() <= 102   # an unclipped vector is only scaled: no bin above 0.2 * 512
    assert len({bytes(r) for r in d}) == 9


def _group_lines(counts, tmp_path):
    exe = str(tmp_path / "group_count")
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "group_count.cpp")], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe] + [str(int(v)) for v in counts], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr[-2000:]
    return [tuple(int(v) for v in ln.split()) for ln in r.stdout.splitlines()]


def test_group_count_of_dense_batches(tmp_path):
    """form_groups on the keypoint counts the rotation tests rely on: 12 images of 110 000 Hessian keypoints form six groups of two
    (the limit is 300 000 for a batch below 4.8 M) and five of them [2, 2, 1].  An image of 500 keypoints behind four dense ones
    joins the second group (the greedy rule): a small image is a group of its own only as a batch of its own."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    g = _group_lines([110000] * 12, tmp_path)
    assert len(g) == 6 and all(hi - lo == 220000 for lo, hi in g)
    assert [hi - lo for lo, hi in _group_lines([110000] * 5, tmp_path)] == [220000, 220000, 110000]
    assert [hi - lo for lo, hi in _group_lines([110000] * 4 + [500], tmp_path)] == [220000, 220500]


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the fused histogram + quantisation
# ----------------------------------------------------------------------------------------------------------------------

@gpu
@pytest.mark.parametrize("n", [1, 3, 4, 5, 9])
def test_fused_histogram_and_quantisation_for_group_remainders(ctx, n):
    """The first n of the nine patches through the production kernels: every descriptor byte the oracle's (groups of four keypoints per
    wavefront and their remainders; n = 1 is the clipped patch alone, n = 3 ends in the all-zero vector)."""
    p, d, _ = nine()
    got = ctx.sift(p[:n])
    assert np.array_equal(got, d[:n]), np.flatnonzero((got != d[:n]).any(axis=1)).tolist()


@gpu
@pytest.mark.parametrize("dead", [(0,), (2,), (3,), (4, 6), (0, 1, 2, 3), (8,)])
def test_dead_keypoints_write_nothing(ctx, dead):
    """alive = 0 at the first, a middle and the last position of a group of four (and in the second group, a whole group, the
    remainder group): the rows of dead keypoints keep the caller's bytes, every other row is the oracle's."""
    p, d, _ = nine()
    alive = np.ones(9, np.int32); alive[list(dead)] = 0
    got = ctx.sift_alive(p, alive, fill=0xAB)
    want = d.copy(); want[list(dead)] = 0xAB
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()


@gpu
@pytest.mark.parametrize("n", [1, 3, 65])
def test_dead_keypoints_write_nothing_at_odd_counts(ctx, n):
    """The nine patches repeated to n keypoints, every third dead from the second on (n = 1: none): counts at which the operator's
    arrays - patches, flags, descriptors, gradient pairs - are multiples of nothing.  The same reference, the same comparison."""
    p, d, _ = nine()
    idx = np.arange(n) % 9
    alive = np.ones(n, np.int32); alive[1::3] = 0
    got = ctx.sift_alive(p[idx], alive, fill=0xAB)
    want = d[idx].copy(); want[alive == 0] = 0xAB
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()


@gpu
def test_clipped_next_to_unclipped_in_every_order(ctx):
    """A wavefront renormalises when any of its four keypoints clipped; the others must come out untouched by it.  All 16 patterns of
    clipped / unclipped over a group of four, and the all-zero vector at each position among clipped ones."""
    p, d, c = nine()
    yes, no, zero = np.flatnonzero(c), [1, 4, 6, 8], 2
    idx = []
    for m in range(16):
        idx += [(yes if (m >> j) & 1 else no)[j] for j in range(4)]
    for pos in range(4):
        idx += [zero if j == pos else yes[j] for j in range(4)]
    idx = np.array(idx)
    got = ctx.sift(p[idx])
    assert np.array_equal(got, d[idx]), np.flatnonzero((got != d[idx]).any(axis=1)).tolist()


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the group pipeline
# ----------------------------------------------------------------------------------------------------------------------

UHD_W, UHD_H = 3840, 2160
N_UHD = 12


def _device_records(dkeys, total):
    import ctypes
    import torch
    import hesaff_amd
    buf = torch.empty(max(total, 1) * 164, dtype=torch.uint8, device="cuda")
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    if total:
        assert hip.hipMemcpy(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(dkeys), ctypes.c_size_t(total * 164), 3) == 0
    return np.frombuffer(buf.cpu().numpy().tobytes()[: total * 164], dtype=hesaff_amd.KEYPOINT_DTYPE)


@pytest.fixture(scope="module")
def uhd():
    """12 dense UHD images, a 13th that is flat but for one 256 x 256 tile of the first, a context for batches of 12, and every
    image's result from a call of its own: (imgs [13, H, W] on the device, ctx, [(count_hessian, records)] * 13)."""
    import torch
    import hesaff_amd
    from hesaff_amd.synth import band_noise_batch_torch
    imgs = torch.empty((N_UHD + 1, UHD_H, UHD_W), dtype=torch.uint8, device="cuda")
    imgs[:N_UHD] = band_noise_batch_torch(N_UHD, UHD_H, UHD_W, seed=777, device="cuda")
    imgs[N_UHD] = 128
    imgs[N_UHD, 900:1156, 1700:1956] = imgs[0, 900:1156, 1700:1956]
    torch.cuda.synchronize()
    p = hesaff_amd.default_params(); p.max_batch = N_UHD
    c = hesaff_amd.HesaffContext(p, device=0)
    single = []
    for b in range(N_UHD + 1):
        ch, cd, dk, total = c.detect_batch_device(imgs[b].data_ptr(), 1, UHD_W, UHD_H)
        assert total == int(cd[0])
        single.append((int(ch[0]), _device_records(dk, total).copy()))
    yield imgs, c, single
    c.close()
    del imgs
    torch.cuda.empty_cache()


def _assert_batch_equals_singles(c, imgs, order, single, what):
    import torch
    batch = imgs[order].contiguous()
    torch.cuda.synchronize()
    ch, cd, dk, total = c.detect_batch_device(batch.data_ptr(), len(order), UHD_W, UHD_H)
    keys = _device_records(dk, total)
    assert ch.tolist() == [single[b][0] for b in order], what
    assert cd.tolist() == [len(single[b][1]) for b in order], what
    starts = np.concatenate([[0], np.cumsum(cd)])
    for j, b in enumerate(order):
        assert keys[starts[j]:starts[j + 1]].tobytes() == single[b][1].tobytes(), "%s: records of image %d (position %d)" % (what, b, j)
    return ch


@gpu
@pytest.mark.parametrize("level", [0, 2])
def test_slots_rotate_over_six_groups(uhd, tmp_path, level):
    """One batch of 12 dense UHD images: form_groups makes at least four groups of their Hessian counts (six, at about 117 k keypoints
    an image), so every patch slot is written a second time while the descriptors of the group before are still to run.  Per-image
    counts and every record byte equal the same images run one per call; with the stage timers off and on."""
    imgs, c, single = uhd
    counts = [single[b][0] for b in range(N_UHD)]
    if shutil.which("g++") is not None:
        assert len(_group_lines(counts, tmp_path)) >= 4, counts
    assert min(counts) > 75000 and max(counts) < 150000, counts   # 300 000 per group: two or three images each, four groups at least
    c.set_profiling(level)
    try:
        _assert_batch_equals_singles(c, imgs, list(range(N_UHD)), single, "profiling %d" % level)
    finally:
        c.set_profiling(0)


@gpu
@pytest.mark.parametrize("order", [(3, 4, 5, 6, 7), (3, 4, 5, 6, N_UHD), (N_UHD, 3, 4)], ids=["one-image-last", "tile-last", "tile-first"])
def test_short_last_groups(uhd, tmp_path, order):
    """Batches that end in a short group: five dense UHD images (groups [2, 2, 1]: one image's descriptor chain behind a full patch
    stage), four and behind them one whose only texture is a 256 x 256 tile (a few hundred keypoints, which join the second group),
    and the tile image in front.  Records equal the single-image runs."""
    imgs, c, single = uhd
    order = list(order)
    counts = [single[b][0] for b in order]
    assert 50 < single[N_UHD][0] < 5000, single[N_UHD][0]
    if shutil.which("g++") is not None and order == [3, 4, 5, 6, 7]:
        g = _group_lines(counts, tmp_path)
        assert len(g) >= 3 and g[-1][1] - g[-1][0] == counts[-1], g
    _assert_batch_equals_singles(c, imgs, order, single, "order %s" % order)


@gpu
def test_small_image_behind_uhd_images_in_one_host_call(uhd):
    """hesaff_detect_batch with two UHD images and one 256 x 256 image behind them (images of different sizes are grouped internally:
    the small one is a batch, and a group, of its own): every image's records equal those of a call with that image alone."""
    imgs, c, single = uhd
    small = np.ascontiguousarray(imgs[0, 900:1156, 1700:1956].cpu().numpy())
    big = [imgs[b].cpu().numpy() for b in (7, 8)]
    alone = c.detect_batch([small])[0]
    alone = (alone[0], alone[1].copy())
    assert len(alone[1]) > 50
    res = c.detect_batch(big + [small])
    for (n_hess, keys), b in zip(res[:2], (7, 8)):
        assert n_hess == single[b][0] and keys.tobytes() == single[b][1].tobytes(), b
    assert res[2][0] == alone[0] and res[2][1].tobytes() == alone[1].tobytes()
