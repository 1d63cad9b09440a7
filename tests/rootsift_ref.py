"""The reference of the descriptor modes (hesaff_set_descriptor, include/hesaff_amd.h), from the CPU oracle and numpy alone: the
un-normalised 128-bin histogram of OracleHandle.sift_parts -> normalize, clip at maxBinValue, normalize again if a bin was clipped
(siftdesc.cpp:83-106), restated in numpy float32 -> the bytes of either mode.  In SIFT mode the restatement reproduces the oracle's
own bytes (tests/test_rootsift_host.py), which is what entitles it to define the RootSIFT ones.
Helper of tests/test_rootsift.py and tests/test_rootsift_host.py; nothing here touches the product library."""
import numpy as np

from hesaff_amd import _binding

f32 = np.float32
SIFT, ROOTSIFT = 0, 1


def seq_sum(x):
    """((x[0] + x[1]) + ...) + x[n-1] in float32 (np.sum adds pairwise: another order)"""
    return np.cumsum(np.ascontiguousarray(x, f32), dtype=f32)[-1]


def _normalize(v):
    """SIFTDescriptor::normalize, siftdesc.cpp:83-96"""
    fac = f32(1.0) / np.sqrt(seq_sum(v * v))
    return v * fac


def normalized(hist, max_bin):
    """`vec` as it stands after siftdesc.cpp:102-106 -> (v[128] float32, clipped).  A zero histogram gives NaN throughout (0 * inf)."""
    max_bin = f32(max_bin)
    with np.errstate(all="ignore"):
        v = _normalize(np.ascontiguousarray(hist, f32).reshape(128))
        over = v > max_bin
        if over.any():
            v = _normalize(np.where(over, max_bin, v).astype(f32))
    return v, bool(over.any())


def quantise(v):
    """byte = min((int)(512 v), 255), 0 where 512 v is NaN (the oracle's (int)NaN ends as byte 0 too)"""
    with np.errstate(all="ignore"):
        q = f32(512.0) * v
        nan = np.isnan(q)
        return np.where(nan, 0, np.minimum(np.where(nan, 0, q).astype(np.int64), 255)).astype(np.uint8)


def unit_vector(hist, max_bin, mode):
    """the float vector that is quantised: v (SIFT) or u = sqrtf(v / s), s the sequential sum of v (RootSIFT)"""
    v, _ = normalized(hist, max_bin)
    if mode == SIFT:
        return v
    assert mode == ROOTSIFT
    with np.errstate(all="ignore"):
        return np.sqrt(v / seq_sum(v))


def to_bytes(hist, max_bin, mode):
    """hist[128] (un-normalised, OracleHandle.sift_parts) -> desc[128] u8 in descriptor mode `mode`"""
    return quantise(unit_vector(hist, max_bin, mode))


def describe(handle, patch, max_bin, mode):
    """one 41 x 41 patch -> desc[128] u8 (the oracle's histogram, this module's epilogue)"""
    return to_bytes(handle.sift_parts(patch)[1], max_bin, mode)


def describe_many(handle, patches, max_bin, mode):
    """-> (desc [n, 128] u8, hist [n, 128] float32, clipped [n] bool)"""
    parts = [handle.sift_parts(p)[1] for p in patches]
    desc = np.stack([to_bytes(h, max_bin, mode) for h in parts])
    return desc, np.stack(parts), np.array([normalized(h, max_bin)[1] for h in parts])


def chain(oracle, gray, mode, params=None):
    """The whole upright chain on one float grey image: the oracle's Hessian keypoints and affine shapes, then ho_rectify ->
    normalizeAffine -> the descriptor of `mode` for every converged one.
    -> (regions REGION_DTYPE in the reference's order, keys KEYPOINT_DTYPE, n_hessian)."""
    run = oracle.OracleRun(gray, params=params)
    hf, hi = run.hessian()
    U, ai = run.affine()
    n = run.n_hessian
    max_bin = f32(0.2) if params is None else f32(params.maxBinValue)
    rec = np.zeros(n, _binding.REGION_DTYPE)
    handle = oracle.OracleHandle(params)
    keys = []
    for k in range(n):
        rec[k]["x"], rec[k]["y"], rec[k]["s"], rec[k]["pixelDistance"], rec[k]["response"] = hf[k, 0], hf[k, 1], hf[k, 2], hf[k, 3], hf[k, 4]
        rec[k]["type"], rec[k]["octave"], rec[k]["level"] = hi[k, 0], hi[k, 1], hi[k, 2]
        rec[k]["key"] = -1
        if not ai[k, 0]:
            continue
        rec[k]["a11"], rec[k]["a12"], rec[k]["a21"], rec[k]["a22"] = U[k]
        rec[k]["iters"] = ai[k, 1]
        A = U[k].copy()
        oracle.lib().ho_rectify(A)
        rej, patch = handle.normalize_affine(gray, hf[k, 0], hf[k, 1], hf[k, 2], A)
        rec[k]["outcome"] = 1 if rej else 2
        if rej:
            continue
        rec[k]["key"] = len(keys)
        key = np.zeros((), _binding.KEYPOINT_DTYPE)
        key["x"], key["y"], key["s"], key["response"], key["type"] = hf[k, 0], hf[k, 1], hf[k, 2], hf[k, 4], hi[k, 0]
        key["a11"], key["a12"], key["a21"], key["a22"] = A
        key["desc"] = describe(handle, patch, max_bin, mode)
        keys.append(key)
    return rec, (np.stack(keys) if keys else np.zeros(0, _binding.KEYPOINT_DTYPE)), n
