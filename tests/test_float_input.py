"""Float grey-plane input: the reference's CV_32FC1 detector input (detectPyramidKeypoints(const Mat &), pyramid.h:73) through the
_f32 entry points of include/hesaff_amd.h, the float overload of hesaff.hpp and the HesaffContext *_f32 methods.

The CPU tests check the symbols, the argument checks and that the C++ interface compiles; the GPU tests (marked) compare the float
path bit for bit with the oracle (which takes a float plane itself) and with the 8-bit path, and check the value-domain refusals."""
import ctypes as C
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
REPLAY_SRC = os.path.join(ROOT, "tests", "native", "float_replay.cpp")
SMALL_BANDS = ((1.5, 40.0), (3.0, 40.0), (6.0, 50.0))
F32_SYMBOLS = ["hesaff_detect_batch_f32", "hesaff_detect_batch_cb_f32", "hesaff_detect_regions_f32", "hesaff_detect_batch_device_f32",
               "hesaff_stage_pyramid_f32"]
LIMIT = np.float32(2.0 ** 20)


# ------------------------------------------------------------------ CPU ------------------------------------------------------------------

def test_float_symbols_exported_and_abi_unchanged():
    L = hesaff_amd.load_library()
    for s in F32_SYMBOLS:
        assert hasattr(L, s), s
        assert s in _binding.ABI_SYMBOLS, s
    assert L.hesaff_abi_version() == _binding.ABI_VERSION == 8


def test_float_entry_points_argument_errors():
    """No context, bad counts, NULL images: HESAFF_ERR_ARG, not a crash (a context cannot be made without a GPU)."""
    L = hesaff_amd.load_library()
    res = (_binding._Result * 1)()
    rres = (_binding._RegionResult * 1)()
    one = (C.c_int * 1)(16)
    img = (C.c_void_p * 1)(None)
    sink = _binding.CHUNK_SINK(lambda *a: 0)
    ch = np.zeros(1, np.int32)
    no = C.c_int(); nf = C.c_size_t()
    assert L.hesaff_detect_batch_f32(None, 0, None, None, None, None, None) == -2
    assert L.hesaff_detect_batch_f32(None, 1, img, one, one, None, res) == -2
    assert L.hesaff_detect_batch_f32(None, -1, img, one, one, None, res) == -2
    assert L.hesaff_detect_regions_f32(None, 0, None, None, None, None, None) == -2
    assert L.hesaff_detect_regions_f32(None, 1, img, one, one, None, rres) == -2
    assert L.hesaff_detect_batch_cb_f32(None, 0, None, None, None, None, sink, None) == -2
    assert L.hesaff_detect_batch_cb_f32(None, 1, img, one, one, None, sink, None) == -2
    assert L.hesaff_detect_batch_device_f32(None, 1, None, 16, 16, 0, 0, ch, ch, None, None) == -2
    assert L.hesaff_detect_batch_device_f32(None, 0, None, 16, 16, 0, 0, ch, ch, None, None) == -2
    assert L.hesaff_stage_pyramid_f32(None, None, 16, 16, None, C.byref(no), C.byref(nf)) == -2
    assert L.hesaff_stage_pyramid_f32(None, None, 0, 16, None, C.byref(no), C.byref(nf)) == -2


def test_float_methods_take_float32_only():
    """The *_f32 methods never cast: any other dtype (or a 3-D array) is a TypeError, raised before anything reaches the library."""
    for bad in (np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.float64), np.zeros((8, 8, 3), np.float32), [[0.0]]):
        with pytest.raises(TypeError):
            hesaff_amd.HesaffContext._f32_list([np.zeros((8, 8), np.float32), bad])
    imgs, _, ws, hs, st = hesaff_amd.HesaffContext._f32_list([np.zeros((9, 40), np.float32)[:, 3:20]])
    assert (ws[0], hs[0], st[0]) == (17, 9, 160)   # a padded view travels as it is (row stride in bytes)


def test_float_interface_compiles():
    """A translation unit that calls the float detectPyramidKeypoints with both callbacks set compiles."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", REPLAY_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

def _u32(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _grey(path):
    return hesaff_amd.read_pnm(os.path.join(GOLD, path))


# float planes made from 8-bit images, all in numpy float32: an affine remap, a gamma-2.2 linearisation (kept on the 8-bit scale: the
# Hessian threshold is absolute, pyramid.h:37), the 16-bit range, negative offsets; all but x257 non-integer
TRANSFORMS = {
    "affine": lambda u: u.astype(np.float32) * np.float32(0.37) + np.float32(12.25),
    "gamma22": lambda u: (u.astype(np.float32) / np.float32(255.0)) ** np.float32(2.2) * np.float32(255.0),
    "x257": lambda u: u.astype(np.float32) * np.float32(257.0),
    "negative": lambda u: u.astype(np.float32) * np.float32(1.37) - np.float32(300.75),
}


def _images():
    return [_grey("tiny_20x15.pgm"), _grey("thin_12x40.pgm"), _grey("band_131x77.pgm"), _grey("probe_vga.pgm"),
            band_noise_image(1080, 1920, 77)]


def check_against_oracle(oracle, plane, n_hess, keys, what, params=None):
    o = oracle.OracleRun(plane, params=params)
    g, t, d = o.keys()
    assert n_hess == o.n_hessian and len(keys) == o.n_keys, (what, n_hess, o.n_hessian, len(keys), o.n_keys)
    assert np.array_equal(keys["type"], t), what + ": type"
    assert np.array_equal(keys["desc"], d), what + ": descriptor bytes"
    for j, name in enumerate(["x", "y", "s", "a11", "a12", "a21", "a22", "response"]):
        assert np.array_equal(_u32(keys[name]), _u32(g[:, j])), "%s: %s" % (what, name)
    return o


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(TRANSFORMS))
def test_oracle_float_planes(ctx, oracle, name):
    """detect_batch_f32 on non-integer planes (20x15, 12x40, 131x77, VGA, FHD in one call) is bit for bit the oracle's."""
    planes = [TRANSFORMS[name](u) for u in _images()]
    assert name == "x257" or all((p != np.round(p)).any() for p in planes)
    res = ctx.detect_batch_f32(planes)
    total = 0
    for p, (n_hess, keys) in zip(planes, res):
        check_against_oracle(oracle, p, n_hess, keys, "%s %dx%d" % (name, p.shape[1], p.shape[0]))
        total += len(keys)
    assert total > 100


@pytest.mark.gpu
def test_oracle_linearised_photo_mosaic(ctx, oracle):
    """An FHD photograph mosaic, grey-converted and gamma-2.2 linearised in numpy float32."""
    from hesaff_amd.synth import load_sample_photos, photo_mosaic
    photos = load_sample_photos()
    if not photos:
        pytest.skip("no sample photographs on this machine")
    m = photo_mosaic(1080, 1920, 0, photos)
    plane = TRANSFORMS["gamma22"](oracle.gray_from_u8(m))
    (n_hess, keys), = ctx.detect_batch_f32([plane])
    check_against_oracle(oracle, plane, n_hess, keys, "mosaic")
    assert len(keys) > 200


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [0, 2])
def test_float_of_u8_equals_u8_path(oracle, fast):
    """float32(u8) planes, and the colour plane ((float(c0) + c1) + c2) / 3.0f made in numpy, give the keys of the 8-bit path."""
    p = hesaff_amd.default_params(); p.fast = fast
    grey = [band_noise_image(240, 320, 5), _grey("probe_vga.pgm")]
    rng = np.random.default_rng(9)
    colour = np.clip(band_noise_image(300, 420, 6)[:, :, None].astype(np.int16) + rng.integers(-40, 40, (300, 420, 3)), 0, 255).astype(np.uint8)
    c3 = colour.astype(np.float32)
    cplane = ((c3[:, :, 0] + c3[:, :, 1]) + c3[:, :, 2]) / np.float32(3.0)
    assert np.array_equal(_u32(cplane), _u32(oracle.gray_from_u8(colour)))
    with hesaff_amd.HesaffContext(p, device=0) as c:
        want = c.detect_batch(grey + [colour])
        got = c.detect_batch_f32([g.astype(np.float32) for g in grey] + [cplane])
    for i, ((nh, k), (nh2, k2)) in enumerate(zip(got, want)):
        assert nh == nh2 and k.tobytes() == k2.tobytes(), "image %d (fast=%d)" % (i, fast)
        assert len(k) > 100


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(upscaleInputImage=1), dict(initialSigma=1.0), dict(initialSigma=0.4), dict(threshold=9.0),
                                dict(mrSize=1.0), dict(maxIterations=3)],
                         ids=lambda kw: ",".join("%s=%g" % kv for kv in kw.items()))
def test_non_default_parameters(oracle, kw):
    """The non-fused first level (up-sampling, K != 11, K = 0 direct copy) and three other parameter sets."""
    p = _params(**kw)
    planes = [TRANSFORMS["negative"](band_noise_image(300, 420, 91)), TRANSFORMS["gamma22"](band_noise_image(200, 260, 92, SMALL_BANDS))]
    with hesaff_amd.HesaffContext(p, device=0) as c:
        res = c.detect_batch_f32(planes)
    for plane, (n_hess, keys) in zip(planes, res):
        check_against_oracle(oracle, plane, n_hess, keys, str(kw), params=p)
    assert sum(len(k) for _, k in res) > 20


@pytest.mark.gpu
def test_batching_strides_and_sink(ctx):
    """11 planes of three sizes through max_batch = 4, handed over as padded views (row stride > 4 W): each equals the tightly
    packed plane alone; detect_batch_cb_f32 delivers the same records."""
    sizes = [(120, 160), (97, 131), (150, 90)]
    planes = [TRANSFORMS["negative"](band_noise_image(*sizes[i % 3], 300 + i, SMALL_BANDS)) for i in range(11)]
    padded = []
    for pl in planes:
        wide = np.full((pl.shape[0], pl.shape[1] + 13), np.float32(7.5))
        wide[:, 5:5 + pl.shape[1]] = pl
        padded.append(wide[:, 5:5 + pl.shape[1]])
        assert padded[-1].strides[0] > 4 * pl.shape[1]
    p = hesaff_amd.default_params(); p.max_batch = 4
    got = {}
    with hesaff_amd.HesaffContext(p, device=0) as c4:
        batch = c4.detect_batch_f32(padded)
        c4.detect_batch_cb_f32(planes, lambda idx, out: got.update(zip(idx, out)) and 0)
    total = 0
    for i, pl in enumerate(planes):
        (n1, k1), = ctx.detect_batch_f32([pl])
        assert batch[i][0] == n1 and batch[i][1].tobytes() == k1.tobytes(), "image %d" % i
        assert got[i][0] == n1 and got[i][1].tobytes() == k1.tobytes(), "image %d (sink)" % i
        total += len(k1)
    assert total > 500


@pytest.mark.gpu
def test_regions_against_oracle(ctx, oracle):
    """detect_regions_f32 at VGA and FHD: every record against the oracle's hessian() / affine() (all three outcomes occur); its keys
    are detect_batch_f32's."""
    from tests.test_regions import check_against_oracle as check_regions
    planes = [TRANSFORMS["gamma22"](_grey("probe_vga.pgm")), TRANSFORMS["x257"](band_noise_image(1080, 1920, 77))]
    res = ctx.detect_regions_f32(planes)
    keys_b = ctx.detect_batch_f32(planes)
    seen = set()
    for plane, (regions, keys), (n_hess, kb), what in zip(planes, res, keys_b, ("vga", "fhd")):
        check_regions(regions, oracle.OracleRun(plane), what)
        assert keys.tobytes() == kb.tobytes() and len(regions) == n_hess, what
        seen |= set(np.unique(regions["outcome"]).tolist())
    assert seen == {0, 1, 2}, seen


def _device_keys(dkeys, total):
    import torch
    buf = torch.empty(max(total, 1) * 164, dtype=torch.uint8, device="cuda")
    hip = C.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    if total:
        assert hip.hipMemcpy(C.c_void_p(buf.data_ptr()), C.c_void_p(dkeys), C.c_size_t(total * 164), 3) == 0
    return np.frombuffer(buf.cpu().numpy().tobytes()[: total * 164], dtype=hesaff_amd.KEYPOINT_DTYPE)


@pytest.mark.gpu
def test_device_tensor_input(ctx):
    """detect_batch_device_f32 on a torch tensor, contiguous and as a strided view of a wider tensor, equals detect_batch_f32."""
    import torch
    planes = [TRANSFORMS["negative"](band_noise_image(240, 320, 40 + i)) for i in range(3)]
    host = ctx.detect_batch_f32(planes)
    t = torch.from_numpy(np.stack(planes)).cuda()
    wide = torch.full((4, 240 + 3, 320 + 24), 3.0, dtype=torch.float32, device="cuda")
    wide[1:, 2:242, 9:329] = t
    view = wide[1:, 2:242, 9:329]
    assert not view.is_contiguous()
    for what, tt in (("contiguous", t), ("strided view", view)):
        ch, cd, dkeys, total = ctx.detect_batch_device_f32(tt)
        assert [int(v) for v in ch] == [h[0] for h in host], what
        assert [int(v) for v in cd] == [len(h[1]) for h in host], what
        assert _device_keys(dkeys, total).tobytes() == b"".join(h[1].tobytes() for h in host), what
    ch, cd, dkeys, total = ctx.detect_batch_device_f32(view[1])   # one [H, W] plane
    assert int(ch[0]) == host[1][0] and _device_keys(dkeys, total).tobytes() == host[1][1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("scale", [1.0, 2.0 ** -140], ids=["normal", "subnormal"])
def test_pyramid_planes(ctx, oracle, scale):
    """pyramid_f32 planes equal the oracle's plane(), also for an image scaled into the subnormal range."""
    plane = TRANSFORMS["affine"](band_noise_image(160, 250, 9, SMALL_BANDS)) * np.float32(scale)
    if scale < 1:
        assert (np.abs(plane) < np.finfo(np.float32).tiny).all() and (plane != 0).mean() > 0.99
    o = oracle.OracleRun(plane, keep_planes=True, detect_only=True)
    pyr = ctx.pyramid_f32(plane)
    assert len(pyr) == o.n_octaves()
    for oi, (Ls, Rs) in enumerate(pyr):
        for l in range(5):
            a, b = Ls[l], o.plane(oi, 0, l)
            assert np.array_equal(_u32(a), _u32(b)), "octave %d L%d" % (oi, l)
            a, b = Rs[l][1:-1, 1:-1], o.plane(oi, 1, l)[1:-1, 1:-1]
            ne = (_u32(a) != _u32(b)) & ~((a == 0) & (b == 0))
            assert not ne.any(), "octave %d R%d" % (oi, l)


@pytest.mark.gpu
def test_edge_of_the_range(ctx, oracle):
    """A +-2^20 high-contrast image is accepted, completes and matches the oracle."""
    u = band_noise_image(300, 420, 17)
    plane = np.where(u >= 128, LIMIT, -LIMIT).astype(np.float32)
    plane[::7, ::5] = np.float32(0.0)
    (n_hess, keys), = ctx.detect_batch_f32([plane])
    check_against_oracle(oracle, plane, n_hess, keys, "+-2^20")
    assert n_hess > 0


BAD_VALUES = [np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), np.float32(2.0 ** 20 + 1), np.float32(-(2.0 ** 20 + 1))]


@pytest.mark.gpu
def test_refusals_host(ctx):
    """NaN, +-Inf and |v| = 2^20 + 1 make every host entry point refuse the whole call, naming the image and the first pixel;
    the context then gives the right results for a valid batch."""
    good = [TRANSFORMS["affine"](band_noise_image(120, 160, 50 + i, SMALL_BANDS)) for i in range(3)]
    want = ctx.detect_batch_f32(good)
    for v in BAD_VALUES:
        bad = [g.copy() for g in good]
        bad[2][37, 11] = v
        bad[2][90, 3] = v
        for call in (lambda: ctx.detect_batch_f32(bad), lambda: ctx.detect_regions_f32(bad),
                     lambda: ctx.detect_batch_cb_f32(bad, lambda idx, out: 0), lambda: ctx.pyramid_f32(bad[2])):
            with pytest.raises(hesaff_amd.HesaffError) as e:
                call()
            assert e.value.code == -2
            msg = str(e.value)
            assert "row 37, column 11" in msg, msg
        assert "image 2" in str(pytest.raises(hesaff_amd.HesaffError, ctx.detect_batch_f32, bad).value)
    got = ctx.detect_batch_f32(good)
    for (n1, k1), (n2, k2) in zip(got, want):
        assert n1 == n2 and k1.tobytes() == k2.tobytes()
    edge = good[0].copy(); edge[0, 0] = LIMIT; edge[1, 1] = -LIMIT   # the bound itself is accepted
    ctx.detect_batch_f32([edge])


@pytest.mark.gpu
def test_refusals_device(ctx):
    """The device entry point's check kernel refuses the same values before any detection kernel runs."""
    import torch
    good = np.stack([TRANSFORMS["affine"](band_noise_image(120, 160, 60 + i, SMALL_BANDS)) for i in range(3)])
    want = ctx.detect_batch_f32(list(good))
    for v in BAD_VALUES:
        bad = good.copy()
        bad[1, 100, 150] = v
        with pytest.raises(hesaff_amd.HesaffError) as e:
            ctx.detect_batch_device_f32(torch.from_numpy(bad).cuda())
        assert e.value.code == -2 and "image 1" in str(e.value) and "row 100, column 150" in str(e.value), str(e.value)
    ch, cd, dkeys, total = ctx.detect_batch_device_f32(torch.from_numpy(good).cuda())
    assert [int(v) for v in ch] == [w[0] for w in want]
    assert _device_keys(dkeys, total).tobytes() == b"".join(w[1].tobytes() for w in want)


def _parse_replay(out):
    images = []
    for line in out.splitlines():
        if line.startswith("I "):
            images.append([[], b"", None])
        elif line[:2] in ("H ", "A "):
            images[-1][0].append(line)
        elif line.startswith("K "):
            images[-1][1] += bytes.fromhex(line[2:])
        elif line.startswith("N "):
            images[-1][2] = tuple(int(v) for v in line[2:].split())
        else:
            raise AssertionError("unexpected line from float_replay: %r" % line)
    return images


def _expected_stream(regions):
    """detect_regions_f32's records in the replay program's print format (hesaff.cpp:66-105 order)."""
    lines = []
    for g in regions:
        b = [int(np.float32(g[k]).view(np.uint32)) for k in ("x", "y", "s", "pixelDistance", "response", "a11", "a12", "a21", "a22")]
        lines.append("H %08x %08x %08x %08x %d %08x %d %d" % (b[0], b[1], b[2], b[3], g["type"], b[4], g["octave"], g["level"]))
        if g["outcome"] >= 1:
            lines.append("A %08x %08x %08x %08x %08x %08x %08x %08x %d %08x %d" % (b[0], b[1], b[2], b[3], b[5], b[6], b[7], b[8], g["type"],
                                                                                 b[4], g["iters"]))
    return lines


@pytest.mark.gpu
def test_cpp_float_replay(ctx, tmp_path):
    """tests/native/float_replay.cpp subclasses both callbacks through hesaff.hpp and calls the float detectPyramidKeypoints with
    padded rows: its callback stream and keys equal detect_regions_f32's."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "float_replay")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, REPLAY_SRC, "-L" + lib_dir, "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    planes = [TRANSFORMS["gamma22"](_grey("band_160x120.pgm")), TRANSFORMS["negative"](_grey("probe_vga.pgm"))]
    args = []
    for i, pl in enumerate(planes):
        path = str(tmp_path / ("plane%d.f32" % i))
        pl.astype("<f4").tofile(path)
        args += [path, str(pl.shape[1]), str(pl.shape[0])]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    plain = subprocess.run([exe, "--plain"] + args, capture_output=True, text=True, timeout=600)
    assert plain.returncode == 0, plain.stderr
    got, got_plain = _parse_replay(r.stdout), _parse_replay(plain.stdout)
    res = ctx.detect_regions_f32(planes)
    n_affine = 0
    for k, ((stream, keys, counts), (stream_p, keys_p, counts_p), (regions, want_keys)) in enumerate(zip(got, got_plain, res)):
        want = _expected_stream(regions)
        assert len(stream) == len(want), (k, len(stream), len(want))
        for j, (a, b) in enumerate(zip(stream, want)):
            assert a == b, "image %d: callback %d: %s vs %s" % (k, j, a, b)
        assert keys == keys_p == want_keys.tobytes(), k
        assert stream_p == []
        n_affine += len(want_keys)
        assert counts == counts_p == (len(regions), n_affine, len(want_keys)), (k, counts, counts_p)
    assert len(got) == 2 and n_affine > 100


@pytest.mark.gpu
def test_device_tensor_zero_strides(ctx):
    """A tensor that repeats an image (expand along n) or a row (expand along H) through a zero stride is read as the images it
    shows: the binding makes it contiguous (a stride of 0 means "tightly packed" to the C entry point)."""
    import torch
    plane = TRANSFORMS["negative"](band_noise_image(240, 320, 44))
    t = torch.from_numpy(plane).cuda()
    rep = t[None].expand(3, 240, 320)
    assert rep.stride(0) == 0
    (n1, k1), = ctx.detect_batch_f32([plane])
    ch, cd, dkeys, total = ctx.detect_batch_device_f32(rep)
    assert [int(v) for v in ch] == [n1] * 3 and [int(v) for v in cd] == [len(k1)] * 3
    assert _device_keys(dkeys, total).tobytes() == k1.tobytes() * 3
    assert len(k1) > 100
    rows = t[17][None].expand(240, 320)                 # every row the same: a stride of 0 along H
    assert rows.stride(0) == 0
    want = ctx.detect_batch_f32([np.broadcast_to(plane[17], (240, 320)).copy()])
    ch, cd, dkeys, total = ctx.detect_batch_device_f32(rows)
    assert int(ch[0]) == want[0][0] and _device_keys(dkeys, total).tobytes() == want[0][1].tobytes()


@pytest.mark.gpu
def test_device_tensor_on_another_device_refused(ctx):
    """The tensor must be on the context's device (and in device memory): ValueError before anything reaches the library."""
    import torch
    t = torch.zeros((2, 64, 64), dtype=torch.float32, device="cuda:%d" % ctx.device)
    with pytest.raises(ValueError):
        ctx.detect_batch_device_f32(t.cpu())
    saved = ctx.device
    try:
        ctx.device = saved + 1          # as if the context had been created on the next GPU
        with pytest.raises(ValueError, match="this context on cuda:%d" % (saved + 1)):
            ctx.detect_batch_device_f32(t)
    finally:
        ctx.device = saved
    with pytest.raises(TypeError):
        ctx.detect_batch_device_f32(t.double())


@pytest.mark.gpu
def test_refusal_in_a_later_chunk():
    """max_batch = 2, six planes, a NaN in image 4: the third chunk is refused while it is staged beside the kernels of the second.
    The call fails naming image 4; the sink form has delivered at most the chunks before it, with the right records; the context
    then gives the right results for a valid list."""
    planes = [TRANSFORMS["affine"](band_noise_image(120, 160, 70 + i, SMALL_BANDS)) for i in range(6)]
    bad = [p.copy() for p in planes]
    bad[4][60, 70] = np.float32(np.nan)
    p = hesaff_amd.default_params(); p.max_batch = 2
    with hesaff_amd.HesaffContext(p, device=0) as c2:
        singles = [c2.detect_batch_f32([pl])[0] for pl in planes]
        for call in (lambda: c2.detect_batch_f32(bad), lambda: c2.detect_regions_f32(bad)):
            with pytest.raises(hesaff_amd.HesaffError) as e:
                call()
            assert e.value.code == -2 and "image 4: pixel (row 60, column 70)" in str(e.value), str(e.value)
        got = {}
        with pytest.raises(hesaff_amd.HesaffError) as e:
            c2.detect_batch_cb_f32(bad, lambda idx, out: got.update(zip(idx, out)) and 0)
        assert "image 4" in str(e.value)
        assert set(got) <= {0, 1, 2, 3}, sorted(got)
        for i, (n, k) in got.items():
            assert n == singles[i][0] and k.tobytes() == singles[i][1].tobytes(), i
        after = c2.detect_batch_f32(planes)
        regions = c2.detect_regions_f32(planes)
    for i, ((n, k), (ns, ks), (r, kr)) in enumerate(zip(after, singles, regions)):
        assert n == ns and k.tobytes() == ks.tobytes() and kr.tobytes() == ks.tobytes() and len(r) == ns, i


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(initialSigma=1.0), dict(upscaleInputImage=1), dict(initialSigma=0.4)],
                         ids=lambda kw: ",".join("%s=%g" % kv for kv in kw.items()))
def test_device_input_non_fused_first_level(kw):
    """The first level without the fused float blur (K != 11, up-sampling, the K = 0 copy) from device planes: packed (one pitched
    copy of all images) and a strided view whose image stride is not rows x row stride (one pitched copy per image) equal the
    host entry point's results."""
    import torch
    planes = [TRANSFORMS["gamma22"](band_noise_image(120, 160, 80 + i, SMALL_BANDS)) for i in range(3)]
    wide = torch.full((3, 125, 171), -5.0, dtype=torch.float32, device="cuda")
    wide[:, 3:123, 7:167] = torch.from_numpy(np.stack(planes)).cuda()
    view = wide[:, 3:123, 7:167]
    assert view.stride(0) * 4 != view.stride(1) * 4 * 120
    with hesaff_amd.HesaffContext(_params(**kw), device=0) as c:
        host = c.detect_batch_f32(planes)
        want = b"".join(k.tobytes() for _, k in host)
        for what, t in (("packed", torch.from_numpy(np.stack(planes)).cuda()), ("strided view", view)):
            ch, cd, dkeys, total = c.detect_batch_device_f32(t)
            assert [int(v) for v in ch] == [h[0] for h in host], (kw, what)
            assert _device_keys(dkeys, total).tobytes() == want, (kw, what)
    assert len(want) > 0


@pytest.mark.gpu
def test_argument_errors_with_a_context(ctx):
    """With a real context: bad counts, NULL image lists and pointers, unaligned pointers and strides below 4 W or not a multiple
    of 4 are HESAFF_ERR_ARG for every _f32 entry point, and the context stays usable."""
    import torch
    L, h = ctx.L, ctx.h
    H, W = 64, 80
    buf = np.zeros(H * W + 4, np.float32)
    base = buf.ctypes.data
    res = (_binding._Result * 2)()
    rres = (_binding._RegionResult * 2)()
    sink = _binding.CHUNK_SINK(lambda *a: 0)
    ws = (C.c_int * 2)(W, W); hs = (C.c_int * 2)(H, H)

    def lists(ptr, stride):
        return (C.c_void_p * 2)(base, ptr), (None if stride is None else (C.c_int * 2)(4 * W, stride))
    cases = {"n < 0": (-1, base, None), "NULL image": (2, None, None), "unaligned": (2, base + 2, None),
             "stride < 4 W": (2, base, 4 * W - 4), "stride not a multiple of 4": (2, base, 4 * W + 2)}
    for what, (n, ptr, stride) in cases.items():
        imgs, st = lists(ptr, stride)
        assert L.hesaff_detect_batch_f32(h, n, imgs, ws, hs, st, res) == -2, what
        assert L.hesaff_detect_regions_f32(h, n, imgs, ws, hs, st, rres) == -2, what
        assert L.hesaff_detect_batch_cb_f32(h, n, imgs, ws, hs, st, sink, None) == -2, what
    assert L.hesaff_detect_batch_f32(h, 1, None, ws, hs, None, res) == -2
    assert L.hesaff_detect_regions_f32(h, 1, None, ws, hs, None, rres) == -2
    assert L.hesaff_detect_batch_cb_f32(h, 1, None, ws, hs, None, sink, None) == -2
    d = torch.zeros((2, H, W + 4), dtype=torch.float32, device="cuda")
    dp = d.data_ptr()
    ch = np.zeros(65, np.int32); cd = np.zeros(65, np.int32)
    dev_cases = {"n = 0": (0, dp, W, 0, 0), "n > max_batch": (65, dp, W, 0, 0), "NULL planes": (2, None, W, 0, 0),
                 "width 0": (2, dp, 0, 0, 0), "unaligned": (2, dp + 2, W, 0, 0), "row stride < 4 W": (2, dp, W, 4 * W - 4, 0),
                 "row stride not a multiple of 4": (2, dp, W, 4 * W + 2, 0), "images overlap": (2, dp, W, 4 * W, 4 * W * (H - 1)),
                 "image stride not a multiple of 4": (2, dp, W, 4 * (W + 4), 4 * (W + 4) * H + 2)}
    for what, (n, ptr, w, rs, ist) in dev_cases.items():
        assert L.hesaff_detect_batch_device_f32(h, n, None if ptr is None else C.c_void_p(ptr), w, H, rs, ist, ch, cd, None,
                                                None) == -2, what
    no = C.c_int(); nf = C.c_size_t()
    out = np.zeros(1 << 20, np.float32)
    assert L.hesaff_stage_pyramid_f32(h, None, H, W, out.ctypes.data, C.byref(no), C.byref(nf)) == -2
    assert L.hesaff_stage_pyramid_f32(h, base + 2, H, W, out.ctypes.data, C.byref(no), C.byref(nf)) == -2
    assert L.hesaff_stage_pyramid_f32(h, base, 0, W, None, C.byref(no), C.byref(nf)) == -2
    plane = TRANSFORMS["affine"](band_noise_image(120, 160, 90, SMALL_BANDS))
    (n1, k1), = ctx.detect_batch_f32([plane])
    o = hesaff_amd.HesaffContext(device=0)
    try:
        (n2, k2), = o.detect_batch_f32([plane])
    finally:
        o.close()
    assert n1 == n2 and k1.tobytes() == k2.tobytes() and len(k1) > 0
