"""hesaff_describe_regions: the second half of the chain for caller-supplied keypoints - the batch form of calling the reference's
two public callback members of AffineHessianDetector oneself (hesaff.cpp:66-71 onHessianKeypointDetected, hesaff.cpp:73-105
onAffineShapeFound).  Round trips against hesaff_detect_regions and foreign keypoints against the CPU oracle, bit for bit: records
and keys are compared as bytes, float fields as uint32 bit patterns; no tolerance anywhere.

The CPU tests check the symbols, the constants and the argument checks; the GPU tests (marked) everything that computes."""
import ctypes as C
import glob
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from hesaff_amd.synth import band_noise_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
FILTER_SRC = os.path.join(ROOT, "tests", "native", "describe_filter.cpp")
SMALL_BANDS = ((1.5, 40.0), (3.0, 40.0), (6.0, 50.0))
GOLDEN_STAGES = sorted(os.path.basename(p)[:-len("_stages.npz")] for p in glob.glob(os.path.join(GOLD, "*_stages.npz")))
FROM_POINTS, FROM_SHAPES = 1, 2
REGION = _binding.REGION_DTYPE
KEY_FIELDS = ("x", "y", "s", "a11", "a12", "a21", "a22", "response")


# ------------------------------------------------------------------ CPU ------------------------------------------------------------------

def test_describe_symbols_constants_and_argument_errors():
    """T1: both symbols are exported and bound, the constants and the methods exist, a call without a context is HESAFF_ERR_ARG
    (not a crash), and the ABI version is still 8."""
    L = hesaff_amd.load_library()
    assert hasattr(L, "hesaff_describe_regions") and hasattr(L, "hesaff_describe_regions_f32")
    assert hesaff_amd.FROM_POINTS == _binding.FROM_POINTS == 1 and hesaff_amd.FROM_SHAPES == _binding.FROM_SHAPES == 2
    assert callable(hesaff_amd.HesaffContext.describe_regions) and callable(hesaff_amd.HesaffContext.describe_regions_f32)
    assert L.hesaff_abi_version() == _binding.ABI_VERSION == 8
    header = open(os.path.join(ROOT, "include", "hesaff_amd.h")).read()
    assert "#define HESAFF_FROM_POINTS 1" in header and "#define HESAFF_FROM_SHAPES 2" in header
    res = (_binding._RegionResult * 1)()
    one = (C.c_int * 1)(16)
    img = (C.c_void_p * 1)(None)
    recs = (C.c_void_p * 1)(None)
    for f in (L.hesaff_describe_regions, L.hesaff_describe_regions_f32):
        tail = (recs, one, FROM_POINTS, res)
        mid = (None, None) if f is L.hesaff_describe_regions else (None,)
        assert f(None, 0, None, None, None, *mid, None, None, FROM_POINTS, None) == -2
        assert f(None, 1, img, one, one, *mid, *tail) == -2


def test_describe_interface_compiles():
    """describe_filter.cpp (both callbacks subclassed, the kept records handed to the batch member) and the untouched
    callbacks_replay.cpp compile against hesaff.hpp with -Wall -Werror."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    for src in (FILTER_SRC, os.path.join(ROOT, "tests", "native", "callbacks_replay.cpp")):
        r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", src], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ helpers ------------------------------------------------------------------

def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _grey(name):
    return hesaff_amd.read_pnm(os.path.join(GOLD, name))


def _same_records(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.shape, want.shape)
    if got.tobytes() != want.tobytes():
        for name in got.dtype.names:
            ne = np.flatnonzero(got[name].view(np.uint32) != want[name].view(np.uint32)) if got[name].dtype.itemsize == 4 and got[name].ndim == 1 \
                else np.flatnonzero((got[name] != want[name]).reshape(len(got), -1).any(axis=1))
            if len(ne):
                raise AssertionError("%s: field %s differs in %d of %d records, first %d: %r vs %r" % (what, name, len(ne), len(got), ne[0],
                                                                                                   got[name][ne[0]], want[name][ne[0]]))
        raise AssertionError(what + ": records differ outside their fields")


def _renumbered(records):
    """the records with key counting the described ones in this order (what describing exactly these records yields)"""
    out = records.copy()
    d = out["outcome"] == 2
    out["key"] = -1
    out["key"][d] = np.arange(int(d.sum()), dtype=np.int32)
    return out


def _round_trip_images():
    imgs = [("probe_vga", _grey("probe_vga.pgm")), ("fhd", band_noise_image(1080, 1920, 77))]
    return imgs + [(n, _grey(n + ".pgm")) for n in GOLDEN_STAGES]


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

@pytest.mark.gpu
def test_round_trip_from_points(ctx):
    """T2: every record of detect_regions fed back through FROM_POINTS: regions and keys byte-identical to detection's."""
    names, imgs = zip(*_round_trip_images())
    det = ctx.detect_regions(list(imgs))
    back = ctx.describe_regions(list(imgs), [r for r, _ in det], FROM_POINTS)
    seen = set()
    for name, (r0, k0), (r1, k1) in zip(names, det, back):
        _same_records(r1, r0, name + ": regions")
        _same_records(k1, k0, name + ": keys")
        seen |= set(np.unique(r0["outcome"]).tolist())
    assert seen == {0, 1, 2}, seen
    assert sum(len(k) for _, k in det) > 3000


@pytest.mark.gpu
def test_round_trip_from_shapes(ctx):
    """T3: the converged records fed back through FROM_SHAPES: the same keys; the records come back as they went in with `key`
    renumbered; and neither a pyramid nor detection nor the affine iteration ran."""
    names, imgs = zip(*_round_trip_images())
    det = ctx.detect_regions(list(imgs))
    kept = [r[r["outcome"] >= 1] for r, _ in det]
    back = ctx.describe_regions(list(imgs), kept, FROM_SHAPES)
    # (the timings are those of the last device batch: the FHD image alone, so that the batch asked about is one with records)
    ctx.set_profiling(2)
    try:
        again = ctx.describe_regions([imgs[1]], [kept[1]], FROM_SHAPES)
        t = ctx.timings()
    finally:
        ctx.set_profiling(0)
    _same_records(again[0][1], det[1][1], "fhd alone, profiling on: keys")
    for name, (r0, k0), rin, (r1, k1) in zip(names, det, kept, back):
        _same_records(k1, k0, name + ": keys")
        _same_records(r1, _renumbered(rin), name + ": regions")
        assert np.isin(r1["outcome"], (1, 2)).all(), name
    assert sum(len(r) for r in kept) > 3000
    print("timings after FROM_SHAPES: pyramid %.3f detect %.3f affine %.3f patch %.3f sift %.3f total %.3f ms, blur_hess_launches %d"
          % (t.pyramid_ms, t.detect_ms, t.affine_ms, t.patch_ms, t.sift_ms, t.total_ms, t.blur_hess_launches))
    assert t.pyramid_ms == 0.0 and t.detect_ms == 0.0 and t.affine_ms == 0.0 and t.blur_hess_launches == 0
    assert t.patch_ms > 0.0 and t.sift_ms > 0.0 and t.total_ms > 0.0


def _check_selection(ctx, img, r0, k0, sel, from_, what):
    """records r0[sel] (any order, repeats allowed) described: each gets the key it had in the full run, in the caller's order"""
    rin = r0[sel]
    (r1, k1), = ctx.describe_regions([img], [rin], from_)
    _same_records(r1, _renumbered(rin), what + ": regions")
    want = k0[rin["key"][rin["outcome"] == 2]]
    _same_records(k1, want, what + ": keys")
    return k1


@pytest.mark.gpu
@pytest.mark.parametrize("from_", [FROM_POINTS, FROM_SHAPES])
def test_subset_order_and_repeats(ctx, from_):
    """T4: every third record, a seeded permutation, and a record supplied twice."""
    img = _grey("probe_vga.pgm")
    (r0, k0), = ctx.detect_regions([img])
    if from_ == FROM_SHAPES:
        r0 = r0[r0["outcome"] >= 1]
    n = len(r0)
    assert n > 300
    _check_selection(ctx, img, r0, k0, np.arange(0, n, 3), from_, "every third")
    perm = np.random.default_rng(4).permutation(n)
    assert (perm != np.arange(n)).any()
    _check_selection(ctx, img, r0, k0, perm, from_, "permutation")
    j = int(np.flatnonzero(r0["outcome"] == 2)[7])
    sel = np.concatenate([np.arange(0, n, 5), [j], np.arange(1, n, 7), [j]])
    k1 = _check_selection(ctx, img, r0, k0, sel, from_, "repeats")
    rows = np.flatnonzero((sel == j)[r0["outcome"][sel] == 2])
    assert len(rows) >= 2 and all(k1[rows[0]].tobytes() == k1[q].tobytes() for q in rows)


# ---- T5: foreign keypoints against the oracle ----

def patch_window(s, mr_size):
    """(P, smoothing branch) of normalizeAffine for scale s (affine.cpp:106-120): P0 = 2 * int(ceil(s * mrSize)) + 1, the window of the
    smoothing branch has P0 + 2 pixels a side; the direct branch (P = 0) when P0 / 41 <= 0.4"""
    p0 = 2 * int(np.ceil(np.float32(s) * np.float32(mr_size))) + 1
    smooth = float(np.float32(p0) / np.float32(41.0)) > 0.4
    return (p0 + 2 if smooth else 0), smooth


def patch_bin(P):
    return 0 if P <= 41 else 1 if P <= 64 else 2 if P <= 128 else 3 if P <= 512 else 4


def foreign_records(H, W, n_oct, pd0, seed, per_plane=28, shapes=False):
    """Seeded keypoints that no detector produced.  Every plane (octave, level 0..2) gets per_plane points with a scale near that
    level's own; a further set spans every window size from the direct branch (s < 1.4) to windows of more than 512 pixels, on the
    plane whose scale is nearest.  A fifth of the positions lie within a few pixels of the image border.  shapes: U = a rotation
    times diag(1, 1 / r), r from 1 (isotropic) to 6, times a factor that moves the determinant away from 1."""
    rng = np.random.default_rng(seed)
    sig = [1.6 * 2.0 ** (l / 3.0) for l in range(3)]
    rows = []
    for o in range(n_oct):
        for l in range(3):
            for _ in range(per_plane):
                rows.append((o, l, pd0 * 2 ** o * sig[l] * rng.uniform(0.6, 1.6)))
    for s in np.exp(rng.uniform(np.log(0.8), np.log(70.0), 10 * per_plane)):
        o = int(np.clip(np.floor(np.log2(max(s / (pd0 * 1.6), 1.0))), 0, n_oct - 1))
        l = int(np.clip(np.rint(3.0 * np.log2(max(s / (pd0 * 2 ** o * 1.6), 1.0))), 0, 2))
        rows.append((o, l, s))
    rec = np.zeros(len(rows), REGION)
    for k, (o, l, s) in enumerate(rows):
        if rng.uniform() < 0.2:    # near the border: 0 .. 6 pixels inside (or just outside) on one side
            x, y = rng.uniform(-2.0, W + 2.0), rng.uniform(-2.0, H + 2.0)
            side, d = rng.integers(4), rng.uniform(-1.0, 6.0)
            x, y = [(d, y), (W - 1 - d, y), (x, d), (x, H - 1 - d)][side]
        else:
            m = min(0.45 * min(H, W), 3.2 * s)   # mostly room for the window; large scales crowd the centre
            x, y = rng.uniform(m, W - m), rng.uniform(m, H - m)
        rec[k]["x"], rec[k]["y"], rec[k]["s"] = x, y, s
        rec[k]["octave"], rec[k]["level"] = o, l
        rec[k]["response"] = rng.normal(0.0, 40.0)
        rec[k]["type"] = rng.integers(3)
        rec[k]["pixelDistance"] = -7.0    # ignored on input
        rec[k]["key"] = 12345             # ignored on input
        if shapes:
            th, r, f = rng.uniform(0, 2 * np.pi), rng.uniform(1.0, 6.0), np.exp(rng.uniform(np.log(0.5), np.log(2.0)))
            R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
            R2 = np.array([[np.cos(1.7 * th), -np.sin(1.7 * th)], [np.sin(1.7 * th), np.cos(1.7 * th)]])
            U = f * (R @ np.diag([1.0, 1.0 / r]) @ R2)
            rec[k]["a11"], rec[k]["a12"], rec[k]["a21"], rec[k]["a22"] = U[0, 0], U[0, 1], U[1, 0], U[1, 1]
            rec[k]["iters"] = rng.integers(0, 16)
    return rec[rng.permutation(len(rec))]


def oracle_describe(oracle, plane, rec, from_, params=None):
    """What the reference computes for these records on the float grey plane, from the oracle library alone: the scale-space plane
    (octave, level) -> findAffineShape -> rectify -> normalizeAffine -> SIFT (hesaff.cpp:66-105).
    -> expected output records (REGION_DTYPE) and keys (KEYPOINT_DTYPE)"""
    handle = oracle.OracleHandle(params)
    pd0 = 0.5 if params is not None and params.upscaleInputImage else 1.0
    planes = {}
    if from_ == FROM_POINTS:
        run = oracle.OracleRun(plane, keep_planes=True, detect_only=True, params=params)
        for o, l in set(zip(rec["octave"].tolist(), rec["level"].tolist())):
            planes[(o, l)] = run.plane(o, 0, l)
    out = rec.copy()
    keys = []
    for k in range(len(rec)):
        r = rec[k]
        o, l = int(r["octave"]), int(r["level"])
        pd = np.float32(pd0 * 2 ** o)
        out[k]["pixelDistance"] = pd
        out[k]["reserved"] = 0
        out[k]["key"] = -1
        if from_ == FROM_POINTS:
            conv, U, it = handle.find_affine_shape(planes[(o, l)], r["x"], r["y"], r["s"], pd)
            out[k]["a11"], out[k]["a12"], out[k]["a21"], out[k]["a22"] = U if conv else (0, 0, 0, 0)
            out[k]["iters"] = it if conv else 0
            if not conv:
                out[k]["outcome"] = 0
                continue
        else:
            U = np.array([r["a11"], r["a12"], r["a21"], r["a22"]], np.float32)
        A = np.array(U, np.float32)
        oracle.lib().ho_rectify(A)
        rej, patch = handle.normalize_affine(plane, r["x"], r["y"], r["s"], A)
        if rej:
            out[k]["outcome"] = 1
            continue
        out[k]["outcome"] = 2
        out[k]["key"] = len(keys)
        key = np.zeros((), _binding.KEYPOINT_DTYPE)
        key["x"], key["y"], key["s"], key["response"], key["type"] = r["x"], r["y"], r["s"], r["response"], r["type"]
        key["a11"], key["a12"], key["a21"], key["a22"] = A
        key["desc"] = handle.sift(patch)   # cast to unsigned char as at hesaff.cpp:91
        keys.append(key)
    return out, (np.stack(keys) if keys else np.zeros(0, _binding.KEYPOINT_DTYPE))


def outcome_counts(want):
    return {"converged": int((want["outcome"] >= 1).sum()), "rejected": int((want["outcome"] == 1).sum()),
            "described": int((want["outcome"] == 2).sum())}


def coverage(want, mr_size):
    """window bins and normalizeAffine branches among the described records"""
    d = want[want["outcome"] == 2]
    win = [patch_window(s, mr_size) for s in d["s"]]
    return {patch_bin(P) for P, smooth in win if smooth}, {smooth for _, smooth in win}


def check_foreign(describe, oracle, plane, rec, from_, what, params=None):
    want_r, want_k = oracle_describe(oracle, plane, rec, from_, params)
    got_r, got_k = describe(rec)
    n = outcome_counts(want_r)
    print("%s: %d records, by the oracle %s" % (what, len(rec), n))
    # converged / iters / U, the rejection set, the rectified A, the descriptor bytes: every field of every record
    _same_records(got_r, want_r, what + ": regions")
    _same_records(got_k, want_k, what + ": keys")
    assert min(n.values()) >= 20, (what, n)
    return want_r


FOREIGN_SEED = 31
FOREIGN_H, FOREIGN_W, FOREIGN_OCTAVES = 1080, 1920, 7


def foreign_image():
    return band_noise_image(FOREIGN_H, FOREIGN_W, 77)


@pytest.mark.gpu
@pytest.mark.parametrize("from_", [FROM_POINTS, FROM_SHAPES])
def test_foreign_keypoints_against_oracle(ctx, oracle, from_):
    """T5: keypoints that are not the detector's, on every plane it can find keypoints on, near the border, through all five
    window-size bins and both branches of normalizeAffine: every field and every descriptor byte is the oracle's."""
    img = foreign_image()
    plane = oracle.gray_from_u8(img)
    rec = foreign_records(FOREIGN_H, FOREIGN_W, FOREIGN_OCTAVES, 1.0, FOREIGN_SEED, shapes=from_ == FROM_SHAPES)
    assert {(o, l) for o in range(FOREIGN_OCTAVES) for l in range(3)} == set(zip(rec["octave"].tolist(), rec["level"].tolist()))
    near = np.minimum(np.minimum(rec["x"], FOREIGN_W - 1 - rec["x"]), np.minimum(rec["y"], FOREIGN_H - 1 - rec["y"]))
    assert (near < 6).sum() >= 50
    want = check_foreign(lambda r: ctx.describe_regions([img], [r], from_)[0], oracle, plane, rec, from_, "foreign u8")
    bins, branches = coverage(want, ctx.params.mrSize)
    assert bins == {0, 1, 2, 3, 4} and branches == {False, True}, (bins, branches)
    if from_ == FROM_SHAPES:
        U = np.stack([rec[k] for k in ("a11", "a12", "a21", "a22")], 1).astype(np.float64)
        sv = np.linalg.svd(U.reshape(-1, 2, 2), compute_uv=False)
        ratio, det = sv[:, 0] / sv[:, 1], sv[:, 0] * sv[:, 1]
        assert ratio.min() < 1.2 and ratio.max() > 5.5 and det.min() < 0.5 and det.max() > 2.0


@pytest.mark.gpu
@pytest.mark.parametrize("from_", [FROM_POINTS, FROM_SHAPES])
def test_chunks_and_mixed_sizes(ctx, from_):
    """T6: 11 images of three sizes through max_batch = 4, record lists of different lengths with empty ones among them: each
    image's result equals that of the image alone."""
    sizes = [(120, 160), (97, 131), (150, 90)]
    imgs = [band_noise_image(*sizes[i % 3], 300 + i, SMALL_BANDS) for i in range(11)]
    lists = []
    for i, (r, _) in enumerate(ctx.detect_regions(imgs)):
        if from_ == FROM_SHAPES:
            r = r[r["outcome"] >= 1]
        lists.append(r[:0] if i in (0, 5, 10) else r[::1 + i % 3][:len(r) - 3 * i])
    assert len({len(r) for r in lists}) >= 4 and sum(len(r) for r in lists) > 300
    with hesaff_amd.HesaffContext(_params(max_batch=4), device=0) as c4:
        res = c4.describe_regions(imgs, lists, from_)
    for i, (img, rin, (r4, k4)) in enumerate(zip(imgs, lists, res)):
        (r1, k1), = ctx.describe_regions([img], [rin], from_)
        assert len(r4) == len(rin)
        _same_records(r4, r1, "image %d: regions" % i)
        _same_records(k4, k1, "image %d: keys" % i)
        _same_records(r4, _renumbered(rin), "image %d: regions against detection's" % i)


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(upscaleInputImage=1), dict(maxIterations=2), dict(mrSize=4.0), dict(fast=2),
                                dict(initialSigma=1.0), dict(initialSigma=2.0)],
                         ids=lambda kw: ",".join("%s=%g" % kv for kv in kw.items()))
def test_parameter_variants(oracle, kw):
    """T7: on a context with other parameters both modes round-trip to that context's own detect_regions (fast = 2 included: its
    FROM_SHAPES builds the pyramid its larger windows are sampled from; initialSigma 1.0 / 2.0: FROM_POINTS builds its blur planes with
    the LDS-tile / the two-pass kernels, the launch that only decimates included); the parity-mode variants also describe foreign
    keypoints as the oracle does with those parameters."""
    p = _params(**kw)
    imgs = [band_noise_image(300, 420, 91), band_noise_image(200, 260, 92, SMALL_BANDS)]
    with hesaff_amd.HesaffContext(p, device=0) as c2:
        det = c2.detect_regions(imgs)
        back_p = c2.describe_regions(imgs, [r for r, _ in det], FROM_POINTS)
        back_s = c2.describe_regions(imgs, [r[r["outcome"] >= 1] for r, _ in det], FROM_SHAPES)
        for (r0, k0), (rp, kp), (rs, ks) in zip(det, back_p, back_s):
            _same_records(rp, r0, str(kw) + ": FROM_POINTS regions")
            _same_records(kp, k0, str(kw) + ": FROM_POINTS keys")
            _same_records(rs, _renumbered(r0[r0["outcome"] >= 1]), str(kw) + ": FROM_SHAPES regions")
            _same_records(ks, k0, str(kw) + ": FROM_SHAPES keys")
        assert sum(len(k) for _, k in det) > (0 if "maxIterations" in kw else 100)
        if "upscaleInputImage" in kw:
            r = np.concatenate([r for r, _ in back_p])
            assert set(r["pixelDistance"][r["octave"] == 0].tolist()) == {0.5}
        if "fast" not in kw:
            img = imgs[0]
            up = 1 if "upscaleInputImage" in kw else 0
            n_oct = 0
            rr, cc = 300 << up, 420 << up
            while rr > 12 and cc > 12:
                n_oct += 1; rr //= 2; cc //= 2
            for from_ in (FROM_POINTS, FROM_SHAPES):
                rec = foreign_records(300, 420, n_oct, 0.5 if up else 1.0, 57, per_plane=16, shapes=from_ == FROM_SHAPES)
                want_r, want_k = oracle_describe(oracle, oracle.gray_from_u8(img), rec, from_, p)
                (got_r, got_k), = c2.describe_regions([img], [rec], from_)
                _same_records(got_r, want_r, "%s from %d: foreign regions" % (kw, from_))
                _same_records(got_k, want_k, "%s from %d: foreign keys" % (kw, from_))
                # (two iterations: findAffineShape converges for a handful of these keypoints, by the oracle 4 of 400, 1 described)
                assert len(want_k) >= (1 if "maxIterations" in kw and from_ == FROM_POINTS else 20)


@pytest.mark.gpu
@pytest.mark.parametrize("from_", [FROM_POINTS, FROM_SHAPES])
def test_float_planes(ctx, oracle, from_):
    """T8: describe_regions_f32 on the float plane of an 8-bit grey image equals the 8-bit call (a colour image against its numpy grey
    plane too); a plane scaled to [0, 1] goes against the oracle on that plane."""
    img = foreign_image()
    rec = foreign_records(FOREIGN_H, FOREIGN_W, FOREIGN_OCTAVES, 1.0, FOREIGN_SEED, shapes=from_ == FROM_SHAPES)
    rng = np.random.default_rng(9)
    colour = np.clip(band_noise_image(300, 420, 6)[:, :, None].astype(np.int16) + rng.integers(-40, 40, (300, 420, 3)), 0, 255).astype(np.uint8)
    c3 = colour.astype(np.float32)
    cplane = ((c3[:, :, 0] + c3[:, :, 1]) + c3[:, :, 2]) / np.float32(3.0)
    crec = foreign_records(300, 420, 5, 1.0, 58, per_plane=16, shapes=from_ == FROM_SHAPES)
    u8 = ctx.describe_regions([img, colour], [rec, crec], from_)
    padded = np.zeros((300, 431), np.float32); padded[:, :420] = cplane    # rows 4 * 431 bytes apart
    f32 = ctx.describe_regions_f32([img.astype(np.float32), padded[:, :420]], [rec, crec], from_)
    for (ru, ku), (rf, kf), what in zip(u8, f32, ("grey", "colour")):
        _same_records(rf, ru, what + ": f32 regions against u8")
        _same_records(kf, ku, what + ": f32 keys against u8")
        assert len(ku) >= 20
    unit = oracle.gray_from_u8(img) / np.float32(255.0)
    assert unit.max() <= 1.0 and (unit != np.round(unit)).any()
    check_foreign(lambda r: ctx.describe_regions_f32([unit], [r], from_)[0], oracle, unit, rec, from_, "foreign [0, 1] plane")


def _bad_records():
    """(name, from, field changes) - one per refusal rule of include/hesaff_amd.h"""
    inf, nan, big = np.float32(np.inf), np.float32(np.nan), np.float32(2.0 ** 20 * 1.001)
    both = [("type -1", dict(type=-1)), ("type 3", dict(type=3)), ("x nan", dict(x=nan)), ("y inf", dict(y=-inf)), ("s nan", dict(s=nan)),
            ("response inf", dict(response=inf)), ("x large", dict(x=-big)), ("y large", dict(y=big)), ("s zero", dict(s=0.0)),
            ("s negative", dict(s=-1.5)), ("s large", dict(s=big))]
    cases = [(n, f, ch) for n, ch in both for f in (FROM_POINTS, FROM_SHAPES)]
    cases += [(n, FROM_POINTS, ch) for n, ch in [("octave -1", dict(octave=-1)), ("octave past the pyramid", dict(octave=4)),
                                                 ("level -1", dict(level=-1)), ("level 3", dict(level=3))]]
    cases += [(n, FROM_SHAPES, ch) for n, ch in [("a12 nan", dict(a12=nan)), ("a21 inf", dict(a21=inf)), ("a22 large", dict(a22=big)),
                                                 ("zero U", dict(a11=0.0, a12=0.0, a21=0.0, a22=0.0)),
                                                 ("singular U", dict(a11=1.0, a12=2.0, a21=2.0, a22=4.0)),
                                                 ("zero first row", dict(a11=0.0, a12=0.0, a21=1.0, a22=1.0))]]
    return cases


@pytest.mark.gpu
def test_refusals(ctx):
    """T9: one bad record in the middle of a good batch per rule: HESAFF_ERR_ARG naming the image and the record, and the next call
    on the same context is right.  All of it is stopped on the host: nothing here reaches a keypoint kernel."""
    imgs = [band_noise_image(120, 160, 300 + i, SMALL_BANDS) for i in range(3)]    # 160 x 120: octaves 0..3
    det = ctx.detect_regions(imgs)
    good = {FROM_POINTS: [r for r, _ in det], FROM_SHAPES: [r[r["outcome"] >= 1] for r, _ in det]}
    assert all(len(r) > 12 for r in good[FROM_SHAPES])
    want = {f: ctx.describe_regions(imgs, good[f], f) for f in good}
    for name, from_, changes in _bad_records():
        lists = [r.copy() for r in good[from_]]
        for k, v in changes.items():
            lists[1][k][9] = v
        with pytest.raises(hesaff_amd.HesaffError) as e:
            ctx.describe_regions(imgs, lists, from_)
        assert e.value.code == -2 and "image 1" in str(e.value) and "record 9" in str(e.value), (name, from_, str(e.value))
        again = ctx.describe_regions(imgs, good[from_], from_)
        for (r0, k0), (r1, k1) in zip(want[from_], again):
            _same_records(r1, r0, name + ": regions of the call after the refusal")
            _same_records(k1, k0, name + ": keys of the call after the refusal")
    # the call's own arguments
    for from_ in (0, 3, -1):
        with pytest.raises(hesaff_amd.HesaffError) as e:
            ctx.describe_regions(imgs, good[FROM_POINTS], from_)
        assert e.value.code == -2
    L = ctx.L
    imgs_c, n, ptrs, ws, hs, st, chs = ctx._u8_list(imgs)
    recs, rptrs, counts = ctx._region_lists(good[FROM_POINTS], n)
    res = (_binding._RegionResult * n)()
    counts[2] = -1
    assert L.hesaff_describe_regions(ctx.h, n, ptrs, ws, hs, st, chs, rptrs, counts, FROM_POINTS, res) == -2
    assert "image 2" in L.hesaff_last_error(ctx.h).decode()
    counts[2] = len(recs[2]); rptrs[0] = None
    assert L.hesaff_describe_regions(ctx.h, n, ptrs, ws, hs, st, chs, rptrs, counts, FROM_POINTS, res) == -2
    assert "image 0" in L.hesaff_last_error(ctx.h).decode()
    # an empty list needs no pointer
    counts[0] = 0
    assert L.hesaff_describe_regions(ctx.h, n, ptrs, ws, hs, st, chs, rptrs, counts, FROM_POINTS, res) == 0
    assert res[0].count_hessian == 0 and res[0].count_desc == 0 and not res[0].regions
    assert res[1].count_hessian == len(recs[1])
    # more records than the context plans for
    with hesaff_amd.HesaffContext(_params(max_kpts_per_mpx=1000, max_batch=1), device=0) as small:
        many = np.tile(good[FROM_POINTS][0], 5000 // len(good[FROM_POINTS][0]) + 1)
        assert len(many) > 4096
        with pytest.raises(hesaff_amd.HesaffError) as e:
            small.describe_regions(imgs[:1], [many], FROM_POINTS)
        assert e.value.code == -3
        (r1, k1), = small.describe_regions(imgs[:1], good[FROM_POINTS][:1], FROM_POINTS)
        _same_records(r1, want[FROM_POINTS][0][0], "after the capacity refusal")
        _same_records(k1, want[FROM_POINTS][0][1], "after the capacity refusal")


@pytest.mark.gpu
def test_cpp_filter_then_describe(ctx, tmp_path):
    """T10: tests/native/describe_filter.cpp collects the records in both callbacks, keeps the affine shapes whose response lies above
    the median, and hands them to AffineHessianDetector::onAffineShapesFound: its keys are the matching rows of detection's."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "describe_filter")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, FILTER_SRC, "-L" + lib_dir, "-lhesaff_amd",
                           "-Wl,-rpath," + lib_dir])
    for name in ("probe_vga.pgm", "band_160x120.pgm"):
        path = os.path.join(GOLD, name)
        r = subprocess.run([exe, path], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        sel, keys, counts = [], b"", None
        for line in r.stdout.splitlines():
            if line.startswith("S "):
                sel.append(int(line[2:]))
            elif line.startswith("K "):
                keys += bytes.fromhex(line[2:])
            elif line.startswith("N "):
                counts = tuple(int(v) for v in line[2:].split())
            else:
                raise AssertionError("unexpected line from describe_filter: %r" % line)
        (r0, k0), = ctx.detect_regions([_grey(name)])
        conv = np.flatnonzero(r0["outcome"] >= 1)
        median = np.sort(r0["response"][conv])[len(conv) // 2]
        want_sel = conv[r0["response"][conv] > median]
        assert sel == want_sel.tolist() and len(sel) > 10, name
        want = k0[r0["key"][want_sel][r0["outcome"][want_sel] == 2]]
        assert keys == want.tobytes(), name
        # g_numberOfPoints = the records handed over; g_numberOfAffinePoints went on counting from the detection before
        assert counts == (len(sel), len(k0) + len(want), len(want)), (name, counts)
