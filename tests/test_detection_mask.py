"""hesaff_set_next_masks / hesaff_set_next_masks_device: per-image detection masks.  A Hessian keypoint of an image with a mask is
kept iff the mask is non-zero at (row, col) = (clamp((int)(y + 0.5f)), clamp((int)(x + 0.5f))); the rest is dropped on the device
before findAffineShape (include/hesaff_amd.h).  Everything a kept keypoint becomes - its hesaff_region record, its row of keys - is
what the unmasked run makes of it, bit for bit; only `key` is renumbered.  With a keypoint limit the mask acts first.

Expected values never come from the masked path: they come from the oracle's per-keypoint dumps (tests/golden/*_stages.npz,
tests._oracle.OracleRun), the one numpy rule `eligible` below and the reference selection of tests/test_keypoint_limit.py.  The CPU
tests check the symbols, the header, the CLI's refusals, the rule itself and what the fixtures can tell apart; the GPU tests (marked)
the masks through every entry point."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import _binding
from tests.test_keypoint_limit import GOLDEN, _golden_expect, _golden_image, _oracle_expect, _tiled_image, limited, select
from tests.test_regions import check_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
NATIVE_SRC = os.path.join(ROOT, "tests", "native", "detection_mask.cpp")
BANDS = GOLDEN[:3]   # band_96x96, band_131x77, band_160x120


def eligible(x, y, mask):
    """THE rule: which keypoints at (x, y) - the floats onHessianKeypointDetected receives - lie on a non-zero pixel of mask [H, W].
    The add is in binary32, the conversion truncates, the result is clamped into the mask."""
    mask = np.asarray(mask)
    H, W = mask.shape
    col = np.clip((np.asarray(x, np.float32) + np.float32(0.5)).astype(np.int32), 0, W - 1)
    row = np.clip((np.asarray(y, np.float32) + np.float32(0.5)).astype(np.int32), 0, H - 1)
    return mask[row, col] != 0


def eligible_truncating(x, y, mask):
    """what a rule that forgot the + 0.5 would keep"""
    mask = np.asarray(mask)
    H, W = mask.shape
    col = np.clip(np.asarray(x, np.float32).astype(np.int32), 0, W - 1)
    row = np.clip(np.asarray(y, np.float32).astype(np.int32), 0, H - 1)
    return mask[row, col] != 0


def checker(shape, value=255):
    r, c = np.indices(shape[:2])
    return (((r + c) & 1) * value).astype(np.uint8)


def left_half(shape):
    m = np.zeros(shape[:2], np.uint8)
    m[:, :shape[1] // 2] = 255
    return m


def kept_indices(e, mask, n_limit=0):
    """list indices of the keypoints of Expect e that mask (None: no mask) and then the limit (0: none) keep"""
    idx = np.arange(e.n) if mask is None else np.nonzero(eligible(e.hf[:, 0], e.hf[:, 1], mask))[0]
    if n_limit and len(idx):
        idx = idx[select(e.response[idx], n_limit)]
    return idx


def check_masked(e, regions, keys, mask, what, n_limit=0):
    """regions / keys of a masked run against the subset the rule (and then the reference selection) names"""
    idx = kept_indices(e, mask, n_limit)
    hf, hi, U, ai, src, want_keys = e.subset(idx)
    assert len(regions) == len(idx), (what, len(regions), len(idx))
    if len(idx):
        check_regions(regions, hf, hi, U, ai, src, what)
    assert len(keys) == len(want_keys), (what, len(keys), len(want_keys))
    assert keys.tobytes() == want_keys.tobytes(), what + ": key bytes differ from the unmasked keys of the kept keypoints"
    return idx


def subset_of_own(r0, k0, idx):
    """the records idx of a context's own unmasked output (r0, k0), `key` renumbered, and their keys"""
    want = r0[idx].copy()
    described = want["outcome"] == 2
    want_keys = k0[want["key"][described]]
    want["key"][described] = np.arange(int(described.sum()), dtype=np.int32)
    return want, want_keys


def _stages(name):
    return np.load(os.path.join(GOLD, name + "_stages.npz"))


def _write_pnm(path, arr):
    arr = np.ascontiguousarray(arr, np.uint8)
    with open(path, "wb") as f:
        f.write(b"%s\n%d %d\n255\n" % (b"P5" if arr.ndim == 2 else b"P6", arr.shape[1], arr.shape[0]))
        f.write(arr.tobytes())
    return str(path)


# ------------------------------------------------------------------ CPU ------------------------------------------------------------------

def test_symbols_and_argument_errors():
    L = hesaff_amd.load_library()
    assert "hesaff_set_next_masks" in _binding.ABI_SYMBOLS and "hesaff_set_next_masks_device" in _binding.ABI_SYMBOLS
    one = (C.c_void_p * 1)(None)
    assert L.hesaff_set_next_masks(None, 0, None, None) == -2
    assert L.hesaff_set_next_masks(None, 1, one, None) == -2
    assert L.hesaff_set_next_masks(None, -1, one, None) == -2
    assert L.hesaff_set_next_masks_device(None, 0, None, 0, 0) == -2
    assert L.hesaff_set_next_masks_device(None, -1, None, 0, 0) == -2
    assert L.hesaff_abi_version() == _binding.ABI_VERSION == 8


def test_set_mask_interface_compiles():
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", NATIVE_SRC], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    src = open(NATIVE_SRC).read()
    assert "setMask(" in src and "setHessianKeypointCallback" in src and "setAffineShapeCallback" in src


@pytest.mark.parametrize("case", ["no value", "unreadable", "three channels", "other size"])
def test_cli_refuses_a_bad_mask_before_any_device(tmp_path, case):
    img = os.path.join(GOLD, "band_96x96.pgm")
    if case == "no value":
        args, name = [img, "--mask"], "--mask"
    elif case == "unreadable":
        name = str(tmp_path / "no_such_mask.pgm")
        args = [img, "--mask", name]
    elif case == "three channels":
        name = _write_pnm(tmp_path / "colour_mask.ppm", np.full((96, 96, 3), 255, np.uint8))
        args = [img, "--mask", name]
    else:
        name = _write_pnm(tmp_path / "small_mask.pgm", np.full((96, 95), 255, np.uint8))
        args = [img, "--mask", name]
    r = subprocess.run([EXE] + args, capture_output=True, text=True)
    assert r.returncode == 1, (r.stdout, r.stderr)
    assert r.stdout == "" and r.stderr.startswith("hesaff: ") and name in r.stderr, r.stderr


def test_single_image_usage_is_unchanged():
    r = subprocess.run([EXE], capture_output=True, text=True)
    assert r.returncode == 0 and "mask" not in r.stdout


def test_eligible_rule_on_hand_made_values():
    W, H = 12, 5
    col_is = lambda x: int(np.argmax([eligible([x], [0.0], np.eye(1, W, c, dtype=np.uint8).repeat(H, 0))[0] for c in range(W)]))
    assert col_is(np.float32(9.5)) == 10
    assert col_is(np.nextafter(np.float32(9.5), np.float32(0))) == 9
    assert col_is(np.float32(W - 0.4)) == W - 1 and col_is(np.float32(W + 100)) == W - 1 and col_is(np.float32(-3.0)) == 0
    assert col_is(np.float32(0.49)) == 0 and col_is(np.float32(-0.6)) == 0
    # row and column are not swapped: a single pixel of a non-square mask
    m = np.zeros((H, W), np.uint8)
    m[3, 7] = 1
    assert eligible([7.2], [2.6], m)[0] and not eligible([2.6], [7.2], m)[0] and not eligible([3.0], [7.0], m)[0]
    assert eligible([7.2, 6.4, 7.49], [3.4, 3.0, 2.5], m).tolist() == [True, False, True]
    # rows clamp like columns
    m = np.zeros((H, W), np.uint8)
    m[H - 1, 0] = 200
    assert eligible([0.0], [H + 7.0], m)[0] and eligible([-2.0], [H - 0.6], m)[0] and not eligible([0.0], [H - 1.6], m)[0]


@pytest.mark.parametrize("max_batch", (1, 2, 64))
def test_mask_staging_arithmetic_under_sanitizers(tmp_path, max_batch):
    """tests/native/mask_block_sanitize.cpp, a stand-alone program under AddressSanitizer + UBSan: ArrayIO deals a mixed-size list's
    masks out with their images, fill_mask_block never reads a row's padding nor writes outside mask_block_bytes."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "mask_block_sanitize")
    src = [os.path.join(ROOT, "tests", "native", "mask_block_sanitize.cpp")]
    r = subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer",
                        "-o", exe] + src + ["-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe, str(max_batch)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="halt_on_error=1"))
    assert r.returncode == 0, (r.stdout, r.stderr[-4000:])
    assert r.stdout.strip().endswith(" ok") and "planes=13 " in r.stdout, r.stdout
    if max_batch == 1:
        assert "chunks=23 masked_chunks=13 " in r.stdout, r.stdout


def test_fixture_preconditions():
    """What the committed dumps can tell apart under the checkerboard and the left-half mask: a rule that truncates, or that swaps
    x and y, changes the eligibility of dozens of keypoints of every band image, and enough kept keypoints are described."""
    kept, total, trunc, swap, described = [], [], [], [], []
    for name in BANDS:
        st = _stages(name)
        img = _golden_image(name)
        x, y = st["hess_f"][:, 0], st["hess_f"][:, 1]
        ck, lh = checker(img.shape), left_half(img.shape)
        el = eligible(x, y, ck)
        kept.append(int(el.sum())); total.append(len(x))
        trunc.append(int((el != eligible_truncating(x, y, ck)).sum()))
        swap.append(int((eligible(x, y, lh) != eligible(y, x, lh)).sum()))
        described.append(int(np.isin(np.nonzero(el)[0], st["key_src"]).sum()))
    print("checkerboard keeps %s of %s; truncating changes %s; x/y swapped against the left half changes %s; kept and described %s"
          % (kept, total, trunc, swap, described))
    assert kept == [78, 89, 186] and total == [154, 165, 354]
    assert trunc == [80, 83, 187] and swap == [80, 84, 171]
    assert described == [39, 39, 109] and min(described) >= 30
    st = _stages("tiny_20x15")
    assert len(st["hess_f"]) == 1 and not eligible(st["hess_f"][:, 0], st["hess_f"][:, 1], checker(_golden_image("tiny_20x15").shape)).any()


# ------------------------------------------------------------------ GPU ------------------------------------------------------------------

def _golden_masks(imgs):
    return [checker(imgs[0].shape), None] + [checker(im.shape) for im in imgs[2:]]


@pytest.mark.gpu
def test_golden_fixtures_mixed_sizes_one_call(ctx):
    """The five golden fixtures in ONE call with masks [checker, None, checker, checker, checker]: every record and every key byte
    of every image, count_hessian == the eligible count, the unmasked image unchanged."""
    ex = _golden_expect(ctx)
    imgs = [_golden_image(n) for n in GOLDEN]
    masks = _golden_masks(imgs)
    res = ctx.detect_regions(imgs, masks=masks)
    batch = ctx.detect_batch(imgs, masks=masks)
    counts = []
    for name, e, m, (regions, keys), (n_hess, keys_b) in zip(GOLDEN, ex, masks, res, batch):
        idx = check_masked(e, regions, keys, m, name)
        assert n_hess == len(idx) and keys_b.tobytes() == keys.tobytes(), name
        counts.append(n_hess)
    assert counts == [78, 165, 186, 0, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("n_limit", (1, 7, 78, 79, 186, 10 ** 6))
def test_composition_with_the_keypoint_limit(ctx, n_limit):
    """Mask first, then the N strongest of what is left (78 and 79 straddle band_96x96's eligible count)."""
    ex = _golden_expect(ctx)
    imgs = [_golden_image(n) for n in GOLDEN]
    masks = _golden_masks(imgs)
    with limited(ctx, n_limit):
        res = ctx.detect_regions(imgs, masks=masks)
        batch = ctx.detect_batch(imgs, masks=masks)
    for name, e, m, (regions, keys), (n_hess, keys_b) in zip(GOLDEN, ex, masks, res, batch):
        what = "%s N=%d" % (name, n_limit)
        idx = check_masked(e, regions, keys, m, what, n_limit)
        assert n_hess == len(idx) == min(n_limit, len(kept_indices(e, m))) and keys_b.tobytes() == keys.tobytes(), what


@pytest.mark.gpu
def test_mask_values_and_layout(ctx):
    """band_131x77 (non-square): all-zero, all-255, value 1 against value 255, a bool mask, and padded rows whose padding is never read."""
    name = "band_131x77"
    e = _golden_expect(ctx)[1]
    img = _golden_image(name)
    H, W = img.shape
    assert H != W
    (r0, k0), = ctx.detect_regions([img])
    ck = checker(img.shape)
    pad_on = np.full((H, W + 13), 255, np.uint8); pad_on[:, :W] = 0
    pad_off = np.zeros((H, W + 13), np.uint8); pad_off[:, :W] = ck
    cases = [("all-zero", np.zeros((H, W), np.uint8), np.zeros((H, W), np.uint8)),
             ("all-255", np.full((H, W), 255, np.uint8), np.full((H, W), 255, np.uint8)),
             ("value 1", checker(img.shape, 1), ck), ("value 255", ck, ck), ("bool", ck != 0, ck),
             ("padding 255, mask zero", pad_on[:, :W], np.zeros((H, W), np.uint8)), ("padding 0, checkerboard", pad_off[:, :W], ck)]
    assert cases[5][1].strides[0] == W + 13
    # one call: the image seven times, each with its own mask
    res = ctx.detect_regions([img] * len(cases), masks=[c[1] for c in cases])
    for (what, _, as_mask), (regions, keys) in zip(cases, res):
        check_masked(e, regions, keys, as_mask, name + " " + what)
    assert len(res[0][0]) == 0 and len(res[0][1]) == 0 and len(res[5][0]) == 0
    assert res[1][0].tobytes() == r0.tobytes() and res[1][1].tobytes() == k0.tobytes()
    assert len(res[3][0]) == 89
    for i in (2, 4, 6):
        assert res[i][0].tobytes() == res[3][0].tobytes() and res[i][1].tobytes() == res[3][1].tobytes(), cases[i][0]


@pytest.mark.gpu
def test_single_pixels(ctx):
    """For one keypoint in each of octaves 0, 1 and 2 of band_96x96: a mask that is zero except that keypoint's pixel keeps exactly
    the keypoints the rule names (at least that one), the complement exactly the others."""
    e = _golden_expect(ctx)[0]
    img = _golden_image("band_96x96")
    H, W = img.shape
    masks, chosen = [], []
    for octave in (0, 1, 2):
        i = int(np.nonzero(e.hi[:, 1] == octave)[0][0])
        col = int(np.clip(np.int32(e.hf[i, 0] + np.float32(0.5)), 0, W - 1)); row = int(np.clip(np.int32(e.hf[i, 1] + np.float32(0.5)), 0, H - 1))
        m = np.zeros((H, W), np.uint8); m[row, col] = 255
        masks += [m, 255 - m]
        chosen.append(i)
    res = ctx.detect_regions([img] * 6, masks=masks)
    for k, i in enumerate(chosen):
        one = check_masked(e, res[2 * k][0], res[2 * k][1], masks[2 * k], "pixel of keypoint %d" % i)
        rest = check_masked(e, res[2 * k + 1][0], res[2 * k + 1][1], masks[2 * k + 1], "all but the pixel of keypoint %d" % i)
        assert i in one and len(one) >= 1 and len(one) + len(rest) == e.n and not np.isin(one, rest).any()


@pytest.fixture(scope="module")
def ctx_chunks():
    """a context of its own with max_batch = 2: lists split into chunks"""
    p = hesaff_amd.default_params(); p.max_batch = 2
    c = hesaff_amd.HesaffContext(p, device=0)
    yield c
    c.close()


@pytest.mark.gpu
def test_chunks_and_regrouping(ctx_chunks, oracle):
    """max_batch = 2 and a list of alternating sizes: the list is regrouped into chunks of one geometry, and every image still
    gets its own mask's subset - by detect_regions, detect_batch and detect_batch_cb.  probe_vga (4763 keypoints) takes several
    block-sized passes of the selection."""
    names = ("probe_vga", "band_160x120", "probe_vga", "tiny_20x15", "probe_vga")
    imgs = {n: _golden_image(n) for n in set(names)}
    ex = {n: _oracle_expect(oracle, n, imgs[n]) for n in imgs}
    assert ex["probe_vga"].n == 4763
    lst = [imgs[n] for n in names]
    shp = [im.shape for im in lst]
    masks = [left_half(shp[0]), checker(shp[1]), None, np.full(shp[3], 255, np.uint8), checker(shp[4])]
    c = ctx_chunks
    res = c.detect_regions(lst, masks=masks)
    batch = c.detect_batch(lst, masks=masks)
    streamed = {}
    c.detect_batch_cb(lst, lambda idx, out: streamed.update(zip(idx, out)) and None, masks=masks)
    assert sorted(streamed) == list(range(len(names)))
    kept = []
    for i, (name, m, (regions, keys), (n_hess, keys_b)) in enumerate(zip(names, masks, res, batch)):
        what = "image %d (%s)" % (i, name)
        kept.append(check_masked(ex[name], regions, keys, m, what))
        assert n_hess == len(regions) and keys_b.tobytes() == keys.tobytes(), what + ": detect_batch"
        assert streamed[i][0] == n_hess and streamed[i][1].tobytes() == keys.tobytes(), what + ": detect_batch_cb"
    print("kept per image: %s" % [len(k) for k in kept])
    assert len(kept[2]) == 4763 and len(kept[3]) == 1 and len(kept[1]) == 186
    assert 0 < len(kept[0]) < 4763 and 0 < len(kept[4]) < 4763 and kept[0].tolist() != kept[4].tolist()
    assert res[0][1].tobytes() != res[4][1].tobytes() and res[0][1].tobytes() != res[2][1].tobytes() and res[4][1].tobytes() != res[2][1].tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("padded", (False, True), ids=("tight", "padded"))
def test_device_entry_points(ctx, oracle, padded):
    """Two copies of probe_vga in one device-resident call with device masks left-half and checker, tightly packed and with padded
    rows and planes (the padding 255): counts and device key bytes are the expected subsets, from the 8-bit and the float entry."""
    import torch
    from tests.test_gpu_parity import _device_keys
    vga = _golden_image("probe_vga")
    e = _oracle_expect(oracle, "probe_vga", vga)
    H, W = vga.shape
    masks = [left_half(vga.shape), checker(vga.shape)]
    row = W + 64 if padded else W
    img_stride = row * H + 192 if padded else W * H
    buf = np.full(2 * img_stride, 255, np.uint8)
    for b, m in enumerate(masks):
        plane = buf[b * img_stride:b * img_stride + row * H].reshape(H, row)
        plane[:, :W] = m
    d_masks = torch.from_numpy(buf).cuda()
    want = [e.subset(kept_indices(e, m))[5] for m in masks]
    want_counts = [len(kept_indices(e, m)) for m in masks]
    want_bytes = want[0].tobytes() + want[1].tobytes()
    t8 = torch.from_numpy(np.stack([vga, vga])).cuda()
    tf = torch.from_numpy(np.stack([oracle.gray_from_u8(vga)] * 2)).cuda()
    torch.cuda.synchronize()
    strides = dict(mask_row_stride=row, mask_img_stride=img_stride) if padded else {}
    ch, cd, dkeys, total = ctx.detect_batch_device(t8.data_ptr(), 2, W, H, masks_ptr=d_masks.data_ptr(), **strides)
    assert ch.tolist() == want_counts and cd.tolist() == [len(w) for w in want] and total == len(want[0]) + len(want[1])
    assert _device_keys(dkeys, total).tobytes() == want_bytes, "detect_batch_device"
    ch, cd, dkeys, total = ctx.detect_batch_device_f32(tf, masks_ptr=d_masks.data_ptr(), **strides)
    assert ch.tolist() == want_counts and total == len(want[0]) + len(want[1])
    assert _device_keys(dkeys, total).tobytes() == want_bytes, "detect_batch_device_f32"
    # one-shot: the next device call is unmasked
    ch, cd, dkeys, total = ctx.detect_batch_device(t8.data_ptr(), 2, W, H)
    assert ch.tolist() == [4763, 4763] and total == 2 * len(e.keys)


@pytest.mark.gpu
def test_float_twins(ctx, oracle):
    """detect_regions_f32 / detect_batch_f32 / detect_batch_cb_f32 with masks on the grey plane of the tiled image: the 8-bit call's
    bytes, and both the expected subset."""
    img = _tiled_image()
    e = _oracle_expect(oracle, "tiled", img)
    m = checker(img.shape)
    gray = oracle.gray_from_u8(img)
    (r8, k8), = ctx.detect_regions([img], masks=[m])
    (rf, kf), = ctx.detect_regions_f32([gray], masks=[m])
    (nf, kbf), = ctx.detect_batch_f32([gray], masks=[m])
    streamed = {}
    ctx.detect_batch_cb_f32([gray], lambda idx, out: streamed.update(zip(idx, out)) and None, masks=[m])
    idx = check_masked(e, r8, k8, m, "tiled 8-bit")
    check_masked(e, rf, kf, m, "tiled f32")
    assert 0 < len(idx) < e.n
    assert rf.tobytes() == r8.tobytes() and kf.tobytes() == k8.tobytes() == kbf.tobytes() == streamed[0][1].tobytes()
    assert nf == len(rf) == streamed[0][0]


@pytest.mark.gpu
def test_one_shot_and_refusals(ctx):
    """The masks serve one call; calls that take none refuse them and clear them; the stage operators leave them alone."""
    imgs = [_golden_image(n) for n in GOLDEN]
    masks = _golden_masks(imgs)
    with hesaff_amd.HesaffContext(device=0) as fresh:
        want = fresh.detect_regions(imgs)
    with hesaff_amd.HesaffContext(device=0) as c:
        L, h = c.L, c.h
        first = c.detect_regions(imgs, masks=masks)
        got = c.detect_regions(imgs)
        assert [len(r) for r, _ in first] == [78, 165, 186, 0, 0]
        for (r, k), (rw, kw) in zip(got, want):
            assert r.tobytes() == rw.tobytes() and k.tobytes() == kw.tobytes()
        img = imgs[2]
        ck = checker(img.shape)
        ptr = (C.c_void_p * 1)(ck.ctypes.data)
        two = (C.c_void_p * 2)(ck.ctypes.data, ck.ctypes.data)
        r0, k0 = want[2]
        assert L.hesaff_set_next_masks(h, -1, ptr, None) == -2 and L.hesaff_set_next_masks(h, 1, None, None) == -2
        assert L.hesaff_set_next_masks_device(h, 1, None, 0, 0) == -2 and L.hesaff_set_next_masks_device(h, 1, ptr, -1, 0) == -2
        # armed n != the call's n
        assert L.hesaff_set_next_masks(h, 2, two, None) == 0
        with pytest.raises(hesaff_amd.HesaffError) as err:
            c.detect_regions([img])
        assert err.value.code == -2 and "2 masks" in str(err.value) and "1 image" in str(err.value), str(err.value)
        (r, k), = c.detect_regions([img])
        assert r.tobytes() == r0.tobytes() and k.tobytes() == k0.tobytes()
        # a stride below the width
        assert L.hesaff_set_next_masks(h, 1, ptr, (C.c_int * 1)(img.shape[1] - 1)) == 0
        with pytest.raises(hesaff_amd.HesaffError) as err:
            c.detect_regions([img])
        assert err.value.code == -2 and "image 0" in str(err.value), str(err.value)
        assert len(c.detect_regions([img])[0][0]) == 354
        # describe_regions takes no masks
        assert L.hesaff_set_next_masks(h, 1, ptr, None) == 0
        with pytest.raises(hesaff_amd.HesaffError) as err:
            c.describe_regions([img], [r0], hesaff_amd.FROM_POINTS)
        assert err.value.code == -2
        (rd, kd), = c.describe_regions([img], [r0], hesaff_amd.FROM_POINTS)
        assert rd.tobytes() == r0.tobytes() and kd.tobytes() == k0.tobytes()
        assert len(c.detect_regions([img])[0][0]) == 354
        # process_files takes no masks
        assert L.hesaff_set_next_masks(h, 1, ptr, None) == 0
        with pytest.raises(hesaff_amd.HesaffError) as err:
            c.process_files([])
        assert err.value.code == -2
        assert len(c.detect_regions([img])[0][0]) == 354
        # the stage operators neither read nor clear them
        assert L.hesaff_set_next_masks(h, 1, ptr, None) == 0
        f, i, count = c.hessian_keypoints(img)
        assert count == 354
        assert len(c.detect_regions([img])[0][0]) == 186 and len(c.detect_regions([img])[0][0]) == 354
        # disarming
        assert L.hesaff_set_next_masks(h, 1, ptr, None) == 0 and L.hesaff_set_next_masks(h, 0, None, None) == 0
        assert len(c.detect_regions([img])[0][0]) == 354
        # host masks meet a device call, and the reverse
        import torch
        t = torch.from_numpy(img[None]).cuda()
        d_mask = torch.from_numpy(ck).cuda()
        torch.cuda.synchronize()
        assert L.hesaff_set_next_masks(h, 1, ptr, None) == 0
        with pytest.raises(hesaff_amd.HesaffError) as err:
            c.detect_batch_device(t.data_ptr(), 1, img.shape[1], img.shape[0])
        assert err.value.code == -2
        ch, _, _, _ = c.detect_batch_device(t.data_ptr(), 1, img.shape[1], img.shape[0])
        assert ch.tolist() == [354]
        c.set_next_masks_device(d_mask.data_ptr(), 1)
        with pytest.raises(hesaff_amd.HesaffError) as err:
            c.detect_regions([img])
        assert err.value.code == -2
        ch, _, _, _ = c.detect_batch_device(t.data_ptr(), 1, img.shape[1], img.shape[0], masks_ptr=d_mask.data_ptr())
        assert ch.tolist() == [186]
        (r, k), = c.detect_regions([img])
        assert r.tobytes() == r0.tobytes() and k.tobytes() == k0.tobytes()


@pytest.mark.gpu
@pytest.mark.parametrize("kw", [dict(fast=2), dict(upscaleInputImage=1)], ids=lambda kw: ",".join("%s=%d" % kv for kv in kw.items()))
def test_other_parameter_sets(kw):
    """fast = 2 and upscaleInputImage = 1 (the mask stays at the caller's size): the checkerboard's result is the eligible subset
    of that context's own unmasked detect_regions output (which the existing tests pin)."""
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    img = _golden_image("band_160x120")
    m = checker(img.shape)
    with hesaff_amd.HesaffContext(p, device=0) as c:
        (r0, k0), = c.detect_regions([img])
        (r, k), = c.detect_regions([img], masks=[m])
    assert len(r0) > 100
    idx = np.nonzero(eligible(r0["x"], r0["y"], m))[0]
    want, want_keys = subset_of_own(r0, k0, idx)
    assert 30 < len(idx) < len(r0) - 30
    assert r.tobytes() == want.tobytes(), kw
    assert k.tobytes() == want_keys.tobytes() and len(k) > 0, kw
    if kw.get("upscaleInputImage"):
        assert (r["pixelDistance"] == 0.5).any()


@pytest.mark.gpu
def test_cpp_detector_and_cli(ctx, tmp_path):
    """tests/native/detection_mask.cpp: setMask(checker) on band_96x96 with both callbacks - 78 Hessian callbacks with the expected
    responses in order, the affine callbacks and keys the dumps name, and 154 callbacks from a second run without setMask.
    `hesaff band_96x96.pgm --mask checker.pgm`: the file is hesaff_format_sift of the expected keys."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    e = _golden_expect(ctx)[0]
    img = _golden_image("band_96x96")
    idx = kept_indices(e, checker(img.shape))
    want_keys = e.subset(idx)[5]
    n_affine = int(e.ai[idx, 0].sum())
    assert len(idx) == 78 and 0 < len(want_keys) <= n_affine < 78
    image = str(tmp_path / "band_96x96.pgm")
    shutil.copy(os.path.join(GOLD, "band_96x96.pgm"), image)
    mask = _write_pnm(tmp_path / "checker.pgm", checker(img.shape))
    exe = str(tmp_path / "detection_mask")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, NATIVE_SRC, "-L" + lib_dir, "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, image, mask], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert [ln for ln in lines if ln.startswith("R ")] == ["R %08x" % v for v in e.response[idx].view(np.uint32)]
    assert lines[-3] == "C 78 %d" % n_affine and lines[-2] == "N 78 %d" % len(want_keys) and lines[-1] == "U 154 154", lines[-3:]
    r = subprocess.run([EXE, image, "--mask", mask], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    assert r.stdout.startswith("Detected 78 keypoints and %d affine shapes in " % len(want_keys)), r.stdout
    assert open(image + ".hesaff.sift", "rb").read() == hesaff_amd.format_sift(want_keys, ctx.params.mrSize)
