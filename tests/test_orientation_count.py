"""GPU suite of the orientation count (hesaff_set_orientation_count, include/hesaff_amd.h: secondary orientation peaks, up to four keys
per region).  The reference is the chain of tests/orientation_count_ref.py: tests/orientation_ref.py's oracle chain with the peak rule
stated in numpy float32, every rank turning the same up-is-up frame.  Every comparison is bit for bit."""
import collections
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from hesaff_amd import DESC_ROOTSIFT, FROM_POINTS, FROM_SHAPES, ORI_DOMINANT, ORI_UP, _binding
from tests import orientation_count_ref as P
from tests import orientation_ref as R
from tests import rootsift_ref
from tests.test_orientation import E2E_IMAGES, _same_records, _u32, oracle_patches

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
REGION = _binding.REGION_DTYPE
KEY = _binding.KEYPOINT_DTYPE
f32 = np.float32


def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def pctx():
    """a context of its own in ORI_DOMINANT with orientation count 4 (the session's context stays as it was made)"""
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_orientation(ORI_DOMINANT)
        assert c.orientation_count == 1
        c.set_orientation_count(4)
        assert c.orientation_count == 4
        yield c


_images = {}
_chains = {}


def image(oracle, name):
    if name not in _images:
        img = hesaff_amd.read_pnm(os.path.join(GOLD, name + ".pgm"))
        _images[name] = (img, oracle.gray_from_u8(img))
    return _images[name]


def chain(oracle, name, K=4):
    """the reference chain's (regions, keys, n_hessian, ranks) of a golden image with orientation count K: computed once, never written"""
    if (name, K) not in _chains:
        _chains[(name, K)] = P.peaks_run(oracle, image(oracle, name)[1], K)
    return _chains[(name, K)]


def key_ranks(ranks):
    """the rank of every key, in key order"""
    return np.array([j for r in ranks if r for j in r], np.int64)


# ---------------------------------------------------------------- the stage operator

def check_stage(ctx, oracle, patches, K, what, counts=()):
    """counts: the operator on the first n patches alone as well, for every n of it, against the same reference"""
    want = [P.peaks_of(oracle, p, K) for p in patches]
    for n in tuple(counts) + (len(patches),):
        n_ori, bins, theta = ctx.orientation_peaks_of(patches[:n], K)
        for k, (wn, wb, wt) in enumerate(want[:n]):
            assert n_ori[k] == wn, "%s, K = %d, first %d: n_ori of patch %d: %d, reference %d" % (what, K, n, k, n_ori[k], wn)
            assert bins[k].tolist() == wb.tolist(), "%s, K = %d, first %d: bins of patch %d: %s, reference %s" % (what, K, n, k, bins[k], wb)
            assert np.array_equal(_u32(theta[k]), _u32(wt)), "%s, K = %d, first %d: thetas of patch %d: %s, reference %s" % (what, K, n, k, theta[k], wt)
    return np.array([w[0] for w in want]), np.stack([w[1] for w in want]), theta


@pytest.mark.gpu
def test_stage_on_oracle_patches(ctx, oracle):
    """hesaff_stage_orientation_peaks on 100 patches normalizeAffine made on band_160x120: n_ori, the bins and the angles of every
    rank are the numpy rule's, for K = 4 and K = 2 - at K = 4 of the first 1, 3 and 65 patches alone too, sizes at which the operator's
    arrays are multiples of nothing; rank 0's angle is hesaff_stage_orientation's.  The reference shows every n_ori."""
    patches = oracle_patches(oracle, "band_160x120", 100)
    assert len(patches) == 100
    n_ori, bins, theta = check_stage(ctx, oracle, patches, 4, "oracle patches", counts=(1, 3, 65))
    census = collections.Counter(n_ori.tolist())
    print("n_ori over 100 oracle patches: %s" % sorted(census.items()))
    assert set(census) == {1, 2, 3, 4}, census
    check_stage(ctx, oracle, patches, 2, "oracle patches")
    assert np.array_equal(_u32(theta[:, 0]), _u32(ctx.orientation_of(patches)))
    assert ctx.orientation == ORI_UP and ctx.orientation_count == 1   # the operator neither needs nor changes the context's state
    for bad in (0, 5):
        with pytest.raises(hesaff_amd.HesaffError):
            ctx.orientation_peaks_of(patches[:1], bad)


def constructed_patches():
    c = np.tile(np.arange(41, dtype=np.float64) - 20.0, (41, 1))
    r = c.T.copy()

    def ramp(deg):
        return c * np.cos(np.deg2rad(deg)) + r * np.sin(np.deg2rad(deg))

    return {
        "flat": np.full((41, 41), 93.0, f32),
        "ramp": (3.0 * ramp(15.0)).astype(f32),
        # a ramp towards 15 degrees in the left half, towards 105 degrees in the right half: two comparable peaks nine bins apart
        "two_ramps": np.where(c < 0, 3.0 * ramp(15.0), 3.0 * ramp(105.0)).astype(f32),
        # the upper envelope of six ramps 60 degrees apart - a hexagonal pyramid: six comparable peaks six bins apart
        "star": (3.0 * np.max(np.stack([ramp(15.0 + 60.0 * k) for k in range(6)]), axis=0)).astype(f32),
    }


@pytest.mark.gpu
def test_stage_on_constructed_patches(ctx, oracle):
    """A flat patch (n_ori 1, bin 0, angle 0), one ramp (one peak), two ramps at right angles (two), a six-fold star, which has more
    than four peaks (the four highest, in height order): the numpy rule's bits, for every K."""
    cases = constructed_patches()
    names = list(cases)
    patches = np.stack([cases[n] for n in names])
    at = {n: i for i, n in enumerate(names)}
    for K in (1, 2, 3, 4):
        n_ori, bins, theta = check_stage(ctx, oracle, patches, K, "constructed")
        assert n_ori[at["flat"]] == 1 and bins[at["flat"]].tolist() == [0, -1, -1, -1] and not _u32(theta[at["flat"]]).any()
        assert n_ori[at["ramp"]] == 1
        assert n_ori[at["two_ramps"]] == min(K, 2)
        assert n_ori[at["star"]] == K
    # what the reference says of the constructions themselves
    h = R.histogram(oracle, cases["two_ramps"])
    two, _ = P.peak_bins(h)
    assert len(two) == 2 and (two[1] - two[0]) % 36 in (9, 27), two
    every, _ = P.peak_bins(R.histogram(oracle, cases["star"]))
    assert len(every) == 6 and sorted((b - every[0]) % 6 for b in every) == [0] * 6, every


# ---------------------------------------------------------------- end to end

@pytest.mark.gpu
@pytest.mark.parametrize("name", E2E_IMAGES)
def test_end_to_end_equals_the_reference_chain(pctx, oracle, name):
    """detect_regions and detect_batch with K = 4: counts, every field of every region - outcome, key and reserved included - and
    every byte of every key are the reference chain's.  On band_160x120 the reference holds regions with 0, 1, 2, 3 and 4 keys and
    regions whose rank 0 is rejected while a later rank is described, so nothing here can pass empty."""
    img = image(oracle, name)[0]
    want_r, want_k, n_hess, ranks = chain(oracle, name)
    (got_r, got_k), = pctx.detect_regions([img])
    (nh, keys_b), = pctx.detect_batch([img])
    accepted = [r for r in ranks if r is not None]
    census = collections.Counter(len(r) for r in accepted)
    late = sum(1 for r in accepted if r and r[0] != 0)
    print("%s: %d Hessian keypoints, %d accepted by pass one, %d keys, keys per region %s, rank 0 rejected and a later rank described: %d"
          % (name, n_hess, len(accepted), len(want_k), sorted(census.items()), late))
    if name == "band_160x120":
        assert set(census) == {0, 1, 2, 3, 4}, census
        assert late >= 1
        assert len(want_k) > len(accepted)
    assert nh == n_hess == len(got_r)
    _same_records(got_r, want_r, name + ": regions")
    _same_records(got_k, want_k, name + ": keys")
    assert keys_b.tobytes() == got_k.tobytes()
    # the layout the records promise: a region's keys are rows key .. key + reserved, regions in order, nothing between them
    has = got_r["reserved"] > 0
    assert ((got_r["outcome"] == 2) == has).all() and (got_r["key"][~has] == -1).all()
    assert got_r["key"][has].tolist() == (np.cumsum(got_r["reserved"][has]) - got_r["reserved"][has]).tolist()
    assert int(got_r["reserved"].sum()) == len(got_k)


# ---------------------------------------------------------------- invariants

@pytest.mark.gpu
def test_count_1_and_upright_are_untouched(ctx, oracle):
    """K = 1 in ORI_DOMINANT gives a fresh ORI_DOMINANT context's bytes (reserved = 0 included), also after K = 4 ran on the context;
    ORI_UP with K = 4 gives a default context's bytes; refused counts change nothing."""
    imgs = [image(oracle, "band_160x120")[0], image(oracle, "band_96x96")[0]]
    with hesaff_amd.HesaffContext(device=0) as fresh:
        fresh.set_orientation(ORI_DOMINANT)
        dominant = fresh.detect_regions(imgs)
    upright = ctx.detect_regions(imgs)
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_orientation_count(4)
        assert c.orientation == ORI_UP
        up4 = c.detect_regions(imgs)
        c.set_orientation(ORI_DOMINANT)
        four = c.detect_regions(imgs)
        for bad in (0, 5, -1):
            with pytest.raises(hesaff_amd.HesaffError) as e:
                c.set_orientation_count(bad)
            assert e.value.code == -2 and c.orientation_count == 4
        c.orientation_count = 1
        one = c.detect_regions(imgs)
    for (ur, uk), (gr, gk), (dr, dk), (orr, ok), (fr, fk) in zip(upright, up4, dominant, one, four):
        assert gr.tobytes() == ur.tobytes() and gk.tobytes() == uk.tobytes()
        assert orr.tobytes() == dr.tobytes() and ok.tobytes() == dk.tobytes()
        assert not orr["reserved"].any() and len(fk) > len(dk)


@pytest.mark.gpu
def test_ranks_nest(pctx, oracle):
    """K = 2's keys are exactly the rank-below-2 keys of K = 4's, and the rank-0 key of every region that K = 1 describes has K = 1's
    bytes.  (The ranks are the reference chain's, which the end-to-end test holds the K = 4 run to.)"""
    name = "band_160x120"
    img = image(oracle, name)[0]
    _, _, _, ranks = chain(oracle, name)
    kr = key_ranks(ranks)
    (r4, k4), = pctx.detect_regions([img])
    assert len(kr) == len(k4)
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_orientation(ORI_DOMINANT)
        (r1, k1), = c.detect_regions([img])
        c.set_orientation_count(2)
        (r2, k2), = c.detect_regions([img])
    assert 0 < len(k1) < len(k2) < len(k4)
    assert k2.tobytes() == k4[kr < 2].tobytes()
    assert r2["reserved"].tolist() == [sum(1 for j in (r or []) if j < 2) for r in ranks]
    described = np.nonzero(r1["outcome"] == 2)[0]
    first_is_rank0 = np.array([bool(ranks[i]) and ranks[i][0] == 0 for i in described])
    assert first_is_rank0.all()   # K = 1 describes a region iff its rank 0 is accepted
    assert k4[r4["key"][described]].tobytes() == k1[r1["key"][described]].tobytes()
    assert k1.tobytes() == k4[kr == 0].tobytes()


# ---------------------------------------------------------------- composition

def _identity(recs):
    return [tuple(_u32(np.array([k[f] for f in ("x", "y", "s", "response")], f32)).tolist()) for k in recs]


@pytest.mark.gpu
def test_composes_with_limit_and_mask(pctx, oracle):
    """set_keypoint_limit(40) and a half-image mask with K = 4: every kept region has the keys - all of them, in rank order - of the
    same region in the unlimited, unmasked run."""
    name = "band_160x120"
    img = image(oracle, name)[0]
    want_r, want_k, n_hess, _ = chain(oracle, name)
    mask = np.zeros(img.shape, np.uint8)
    mask[:, : img.shape[1] // 2] = 1
    pctx.set_keypoint_limit(40)
    try:
        (got_r, got_k), = pctx.detect_regions([img], masks=[mask])
    finally:
        pctx.set_keypoint_limit(0)
    full = {}
    for ident, r in zip(_identity(want_r), want_r):
        full[ident] = want_k[r["key"]: r["key"] + r["reserved"]].tobytes() if r["reserved"] else b""
    assert len(full) == n_hess
    assert len(got_r) == 40 < n_hess and (got_r["x"] < img.shape[1] // 2 + 1).all()
    assert (got_r["reserved"] > 1).sum() > 3 and int(got_r["reserved"].sum()) == len(got_k)
    for ident, r in zip(_identity(got_r), got_r):
        mine = got_k[r["key"]: r["key"] + r["reserved"]].tobytes() if r["reserved"] else b""
        assert full[ident] == mine, ident


@pytest.mark.gpu
def test_composes_with_rootsift(oracle):
    """DESC_ROOTSIFT with K = 4: the regions and every key field but desc are the SIFT chain's, and desc is the RootSIFT bytes of
    each rank's own patch."""
    name = "band_96x96"
    img, gray = image(oracle, name)
    want_r, want_k, n_hess, _ = chain(oracle, name)
    root_r, root_k, _, _ = P.peaks_run(oracle, gray, 4, lambda handle: (lambda p: rootsift_ref.describe(handle, p, f32(0.2), rootsift_ref.ROOTSIFT)))
    assert root_r.tobytes() == want_r.tobytes() and len(root_k) == len(want_k) > 80
    assert (root_k["desc"] != want_k["desc"]).any()
    with hesaff_amd.HesaffContext(device=0) as c:
        c.set_orientation(ORI_DOMINANT)
        c.set_orientation_count(4)
        c.set_descriptor(DESC_ROOTSIFT)
        (got_r, got_k), = c.detect_regions([img])
    _same_records(got_r, root_r, "RootSIFT: regions")
    _same_records(got_k, root_k, "RootSIFT: keys")


def _four_key_record(oracle, name):
    want_r, want_k, _, ranks = chain(oracle, name)
    i = next(i for i, r in enumerate(ranks) if r == [0, 1, 2, 3])
    return want_r[i:i + 1].copy(), want_k[want_r[i]["key"]: want_r[i]["key"] + 4]


@pytest.mark.gpu
def test_describe_from_shapes_with_a_four_key_record_given_twice(pctx, oracle):
    """describe_regions(FROM_SHAPES) over [a four-key region, a one-key region, the four-key region again, a region without a key]:
    the reference chain's records and keys - each copy of the record owns four adjacent rows."""
    name = "band_160x120"
    img, gray = image(oracle, name)
    want_r, _, _, ranks = chain(oracle, name)
    four, four_keys = _four_key_record(oracle, name)
    one = want_r[[next(i for i, r in enumerate(ranks) if r == [0])]]
    none = want_r[[next(i for i, r in enumerate(ranks) if r == [])]]
    rec = np.concatenate([four, one, four, none])
    exp_r, exp_k, exp_ranks = P.peaks_from_shapes(oracle, gray, rec, 4)
    assert exp_ranks == [[0, 1, 2, 3], [0], [0, 1, 2, 3], []] and exp_r["key"].tolist() == [0, 4, 5, -1] and exp_r["reserved"].tolist() == [4, 1, 4, 0]
    assert exp_k[0:4].tobytes() == four_keys.tobytes() == exp_k[5:9].tobytes()
    (got_r, got_k), = pctx.describe_regions([img], [rec], FROM_SHAPES)
    _same_records(got_r, exp_r, "FROM_SHAPES: regions")
    _same_records(got_k, exp_k, "FROM_SHAPES: keys")


@pytest.mark.gpu
def test_describe_from_points_equals_the_detecting_run(pctx, oracle):
    imgs = [image(oracle, "band_160x120")[0], image(oracle, "band_96x96")[0]]
    detected = pctx.detect_regions(imgs)
    described = pctx.describe_regions(imgs, [r for r, _ in detected], FROM_POINTS)
    for (dr, dk), (pr, pk) in zip(detected, described):
        assert len(dk) > (dr["outcome"] == 2).sum() > 20
        _same_records(pr, dr, "FROM_POINTS: regions")
        _same_records(pk, dk, "FROM_POINTS: keys")


@pytest.mark.gpu
def test_process_files_text_is_the_keys(pctx, oracle, tmp_path):
    name = "band_160x120"
    _, want_k, n_hess, _ = chain(oracle, name)
    path = str(tmp_path / "band.pgm")
    shutil.copyfile(os.path.join(GOLD, name + ".pgm"), path)
    st = pctx.process_files([path])
    assert st[0][0] == 0 and st[0][2] == n_hess and st[0][3] == len(want_k), st
    text = open(path + ".hesaff.sift", "rb").read()
    assert text == hesaff_amd.format_sift(want_k, pctx.params.mrSize)


@pytest.mark.gpu
def test_cpp_detector_with_orientation_count(oracle, tmp_path):
    """tests/native/orientation_count_keys.cpp: AffineHessianDetector::setOrientationCount(4) holds the reference chain's keys, all of
    them, and replays each callback once per region."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    want_r, want_k, n_hess, _ = chain(oracle, "band_96x96")
    exe = str(tmp_path / "orientation_count_keys")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "orientation_count_keys.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    r = subprocess.run([exe, "4", os.path.join(GOLD, "band_96x96.pgm")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert len(want_k) > (want_r["outcome"] == 2).sum()
    assert lines[0] == "N %d %d %d %d %d" % (n_hess, len(want_k), len(want_k), n_hess, int((want_r["outcome"] >= 1).sum())), lines[0]
    assert [ln[2:] for ln in lines[1:]] == [k.tobytes().hex() for k in want_k]


@pytest.mark.gpu
def test_cli_orientations(oracle, tmp_path):
    """hesaff <image> --orientation dominant --orientations 4 and the --batch form: the text file holds the reference chain's keys;
    without --orientation dominant the count is inert."""
    exe = os.path.join(os.path.dirname(hesaff_amd.lib_path()), "bin", "hesaff")
    name = "band_96x96"
    _, want_k, _, _ = chain(oracle, name)
    want = hesaff_amd.format_sift(want_k, hesaff_amd.default_params().mrSize)
    for form in ("single", "batch", "upright"):
        path = str(tmp_path / (form + ".pgm"))
        shutil.copyfile(os.path.join(GOLD, name + ".pgm"), path)
        if form == "batch":
            lst = str(tmp_path / "list.txt")
            open(lst, "w").write(path + "\n")
            cmd = [exe, "--batch", lst, "--orientation", "dominant", "--orientations", "4"]
        else:
            cmd = [exe, path] + (["--orientation", "dominant"] if form == "single" else []) + ["--orientations", "4"]
        r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, (form, r.stderr)
        text = open(path + ".hesaff.sift", "rb").read()
        if form == "upright":
            assert text == open(os.path.join(GOLD, name + ".hesaff.sift"), "rb").read()
        else:
            assert text == want, form
    r = subprocess.run([exe, path, "--orientations", "5"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "--orientations" in r.stderr


# ---------------------------------------------------------------- the group pipeline

@pytest.mark.gpu
def test_slots_wrap_over_groups_and_ranks():
    """One batch of 12 dense UHD images (tests/test_descriptor_chain.py's) with K = 4: at least four image groups of four ranks each, so
    the patch slots wrap over (group, rank) many times.  Per-image counts and every record byte equal the same images run one per call."""
    import torch
    from hesaff_amd.synth import band_noise_batch_torch
    from tests.test_descriptor_chain import N_UHD, UHD_H, UHD_W, _device_records
    imgs = band_noise_batch_torch(N_UHD, UHD_H, UHD_W, seed=777, device="cuda")
    torch.cuda.synchronize()
    p = hesaff_amd.default_params(); p.max_batch = N_UHD
    with hesaff_amd.HesaffContext(p, device=0) as c:
        c.set_orientation(ORI_DOMINANT)
        c.set_orientation_count(4)
        single = []
        for b in range(N_UHD):
            ch, cd, dk, total = c.detect_batch_device(imgs[b].data_ptr(), 1, UHD_W, UHD_H)
            assert total == int(cd[0])
            single.append((int(ch[0]), _device_records(dk, total).copy()))
        counts = [s[0] for s in single]
        assert min(counts) > 75000 and max(counts) < 150000, counts   # 300 000 per group: four groups at least
        assert all(len(s[1]) > s[0] for s in single)                  # more keys than Hessian keypoints
        ch, cd, dk, total = c.detect_batch_device(imgs.data_ptr(), N_UHD, UHD_W, UHD_H)
        keys = _device_records(dk, total)
    assert ch.tolist() == counts
    assert cd.tolist() == [len(s[1]) for s in single]
    starts = np.concatenate([[0], np.cumsum(cd)])
    for b in range(N_UHD):
        assert keys[starts[b]:starts[b + 1]].tobytes() == single[b][1].tobytes(), "records of image %d" % b
    del imgs
    torch.cuda.empty_cache()


# ---------------------------------------------------------------- capacity

@pytest.mark.gpu
def test_keys_beyond_the_capacity_are_refused(oracle):
    """describe_regions(FROM_SHAPES) with a four-key record repeated 1100 times on a context whose keypoint capacity is 4096: the
    records fit, their 4400 keys do not.  The pack kernel writes no row at or beyond the capacity, the call returns
    HESAFF_ERR_CAPACITY, and the next call on the context succeeds."""
    name = "band_160x120"
    img, gray = image(oracle, name)
    four, four_keys = _four_key_record(oracle, name)
    with hesaff_amd.HesaffContext(_params(max_kpts_per_mpx=1000, max_batch=1), device=0) as small:
        small.set_orientation(ORI_DOMINANT)
        small.set_orientation_count(4)
        many = np.tile(four, 1100)
        assert len(many) < 4096 < 4 * len(many)
        with pytest.raises(hesaff_amd.HesaffError) as e:
            small.describe_regions([img], [many], FROM_SHAPES)
        assert e.value.code == -3
        fits = np.tile(four, 1000)
        (got_r, got_k), = small.describe_regions([img], [fits], FROM_SHAPES)
        assert len(got_k) == 4000 and got_r["key"].tolist() == list(range(0, 4000, 4)) and (got_r["reserved"] == 4).all()
        assert got_k.tobytes() == np.tile(four_keys, 1000).tobytes()
