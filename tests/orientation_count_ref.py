"""The reference of the orientation count (hesaff_set_orientation_count, include/hesaff_amd.h): tests/orientation_ref.py's chain with the
peak rule stated in numpy float32 - every bin that is a strict circular local maximum and at least float32(0.8) * h[m] high is a
candidate, ordered by height descending and bin ascending; each rank turns the same up-is-up A and has a run of normalizeAffine and
a descriptor of its own.  Helper of tests/test_orientation_count.py; nothing here touches the product library."""
import numpy as np

from hesaff_amd import _binding
from tests import orientation_ref as R

f32 = np.float32


def peak_bins(h, K=36):
    """-> (bins of ranks 0 .. n_ori - 1, flat).  K = 36: every candidate."""
    h = np.asarray(h, f32)
    m = int(np.argmax(h))   # the lowest index of the maximum
    if h[m] == 0:
        return [m], True
    least = f32(0.8) * h[m]
    cand = [b for b in range(36) if b != m and h[b] > h[(b - 1) % 36] and h[b] > h[(b + 1) % 36] and h[b] >= least]
    cand.sort(key=lambda b: (-float(h[b]), b))   # (float64 of a float32 orders as the float32 does)
    return ([m] + cand)[:K], False


def theta_at(h, b):
    """step 5's formula around bin b"""
    l, q, r = h[(b - 1) % 36], h[b], h[(b + 1) % 36]
    den = (l + r) - (q + q)
    off = f32(0.0) if den == 0 else (f32(0.5) * (l - r)) / den
    return ((f32(b) + f32(0.5)) + off) * R.BIN_WIDTH - R.PI


def peaks_of(oracle, patch, K):
    """the stage operator's outputs for one patch: n_ori, bins [4] (-1 beyond n_ori), theta [4] (0 beyond it)"""
    h = R.histogram(oracle, patch)
    bins, flat = peak_bins(h, K)
    out_b = np.full(4, -1, np.int32)
    out_t = np.zeros(4, f32)
    for j, b in enumerate(bins):
        out_b[j] = b
        out_t[j] = f32(0.0) if flat else theta_at(h, b)
    return len(bins), out_b, out_t


def describe_ranks(oracle, handle, plane, x, y, s, A_up, K, sift=None):
    """One keypoint whose up-is-up matrix is A_up -> None when pass one rejects it, else [(rank, A'_rank, desc[128])] of the ranks
    whose own run of normalizeAffine accepted, in ascending rank.  sift: patch -> desc[128] (default: the oracle's SIFT bytes)."""
    sift = sift or handle.sift
    rej, patch = handle.normalize_affine(plane, x, y, s, A_up)
    if rej:
        return None
    h = R.histogram(oracle, patch)
    bins, flat = peak_bins(h, K)
    out = []
    for j, b in enumerate(bins):
        A2 = R.rotate(A_up, f32(0.0) if flat else theta_at(h, b), flat)   # every rank from the same A
        rej, p2 = handle.normalize_affine(plane, x, y, s, A2)
        if not rej:
            out.append((j, A2, sift(p2)))
    return out


def _key(x, y, s, response, type_, A2, desc):
    key = np.zeros((), _binding.KEYPOINT_DTYPE)
    key["x"], key["y"], key["s"], key["response"], key["type"] = x, y, s, response, type_
    key["a11"], key["a12"], key["a21"], key["a22"] = A2
    key["desc"] = desc
    return key


def peaks_from_shapes(oracle, plane, rec, K, params=None):
    """hesaff_describe_regions(HESAFF_FROM_SHAPES) in HESAFF_ORI_DOMINANT with orientation count K, for REGION_DTYPE records on a
    float grey plane -> expected output records, keys, and the ranks of every record's keys."""
    handle = oracle.OracleHandle(params)
    pd0 = 0.5 if params is not None and params.upscaleInputImage else 1.0
    out = rec.copy()
    keys, ranks = [], []
    for k in range(len(rec)):
        r = rec[k]
        out[k]["pixelDistance"] = f32(pd0 * 2 ** int(r["octave"]))
        A = np.array([r["a11"], r["a12"], r["a21"], r["a22"]], f32)
        oracle.lib().ho_rectify(A)
        got = describe_ranks(oracle, handle, plane, r["x"], r["y"], r["s"], A, K) or []
        out[k]["outcome"] = 2 if got else 1
        out[k]["key"] = len(keys) if got else -1
        out[k]["reserved"] = len(got) if K > 1 else 0   # (K = 1 is the mode as it stands: reserved stays 0)
        ranks.append([j for j, _, _ in got])
        for _, A2, desc in got:
            keys.append(_key(r["x"], r["y"], r["s"], r["response"], r["type"], A2, desc))
    return out, (np.stack(keys) if keys else np.zeros(0, _binding.KEYPOINT_DTYPE)), ranks


def peaks_run(oracle, gray, K, sift_of=None):
    """The whole chain on one float grey image: the oracle's Hessian keypoints and affine shapes, then up to K keys of every converged
    one.  -> (regions REGION_DTYPE in the reference's order, keys KEYPOINT_DTYPE, n_hessian, ranks: per region the ranks of its keys,
    None where findAffineShape did not converge or pass one rejected).  sift_of: OracleHandle -> (patch -> desc[128]), for another
    descriptor mode than the oracle's SIFT bytes."""
    run = oracle.OracleRun(gray)
    hf, hi = run.hessian()
    U, ai = run.affine()
    n = run.n_hessian
    rec = np.zeros(n, _binding.REGION_DTYPE)
    handle = oracle.OracleHandle()
    sift = sift_of(handle) if sift_of else None
    keys, ranks = [], []
    for k in range(n):
        rec[k]["x"], rec[k]["y"], rec[k]["s"], rec[k]["pixelDistance"], rec[k]["response"] = hf[k, 0], hf[k, 1], hf[k, 2], hf[k, 3], hf[k, 4]
        rec[k]["type"], rec[k]["octave"], rec[k]["level"] = hi[k, 0], hi[k, 1], hi[k, 2]
        rec[k]["key"] = -1
        ranks.append(None)
        if not ai[k, 0]:
            continue
        rec[k]["a11"], rec[k]["a12"], rec[k]["a21"], rec[k]["a22"] = U[k]
        rec[k]["iters"] = ai[k, 1]
        A = U[k].copy()
        oracle.lib().ho_rectify(A)
        got = describe_ranks(oracle, handle, gray, hf[k, 0], hf[k, 1], hf[k, 2], A, K, sift)
        rec[k]["outcome"] = 2 if got else 1
        if got is None:
            continue
        ranks[k] = [j for j, _, _ in got]
        if not got:
            continue
        rec[k]["key"] = len(keys)
        rec[k]["reserved"] = len(got) if K > 1 else 0   # (K = 1 is the mode as it stands: reserved stays 0)
        for _, A2, desc in got:
            keys.append(_key(hf[k, 0], hf[k, 1], hf[k, 2], hf[k, 4], hi[k, 0], A2, desc))
    return rec, (np.stack(keys) if keys else np.zeros(0, _binding.KEYPOINT_DTYPE)), n, ranks
