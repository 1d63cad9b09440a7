"""The reference of the dominant-orientation mode (hesaff_set_orientation, include/hesaff_amd.h), from the CPU oracle and numpy alone:
ho_rectify -> normalizeAffine -> the orientation estimator, stated in numpy float32 with the oracle's atan2f and circular mask ->
A' = A R(theta) in numpy float32 with c, s = float32(cos / sin(float64(theta))) -> normalizeAffine -> SIFT.
Helper of tests/test_orientation.py; nothing here touches the product library."""
import numpy as np

from hesaff_amd import _binding

f32 = np.float32
PI = f32(np.pi)
TO_BIN = f32(36.0) / (f32(2.0) * PI)
BIN_WIDTH = (f32(2.0) * PI) / f32(36.0)

_mask = None


def mask(oracle):
    global _mask
    if _mask is None:
        m = np.zeros((41, 41), f32)
        oracle.lib().ho_circ_gauss_mask(41, m.reshape(-1))
        _mask = m
    return _mask


def at2(oracle, gy, gx):
    """the oracle's ho_atan2f (this image's libm), element-wise"""
    fn = oracle.lib().ho_atan2f
    out = np.empty(gy.shape, f32)
    o, a, b = out.reshape(-1), gy.reshape(-1), gx.reshape(-1)
    for i in range(len(o)):
        o[i] = fn(float(a[i]), float(b[i]))
    return out


def bins_of(oracle, p):
    """steps 1: -> w [39, 39], b [39, 39] (after the wrap), and the bins before the wrap"""
    p = np.ascontiguousarray(p, f32).reshape(41, 41)
    with np.errstate(all="ignore"):
        gx = p[1:40, 2:41] - p[1:40, 0:39]
        gy = p[2:41, 1:40] - p[0:39, 1:40]
        w = mask(oracle)[1:40, 1:40] * np.sqrt(gx * gx + gy * gy)
        t = (at2(oracle, gy, gx) + PI) * TO_BIN
    raw = t.astype(np.int32)
    b = raw.copy()
    b[b >= 36] -= 36
    return w, b, raw


def histogram(oracle, p):
    """steps 1-4 -> h [36] float32 after the six smoothing passes"""
    w, b, _ = bins_of(oracle, p)
    rows = np.zeros((39, 36), f32)
    for c in range(39):
        rows[np.arange(39), b[:, c]] += w[:, c]
    h = np.zeros(36, f32)
    for r in range(39):
        h = h + rows[r]
    for _ in range(6):
        h = ((np.roll(h, 1) + h) + np.roll(h, -1)) / f32(3)
    return h


def peak(h):
    """step 5 -> (theta float32, flat): flat when the maximum is 0 (theta = 0, the frame stays)"""
    m = int(np.argmax(h))   # the lowest index of the maximum
    if h[m] == 0:
        return f32(0.0), True
    l, q, r = h[(m - 1) % 36], h[m], h[(m + 1) % 36]
    den = (l + r) - (q + q)
    off = f32(0.0) if den == 0 else (f32(0.5) * (l - r)) / den
    return ((f32(m) + f32(0.5)) + off) * BIN_WIDTH - PI, False


def cos_sin(theta):
    return f32(np.cos(np.float64(theta))), f32(np.sin(np.float64(theta)))


def estimate(oracle, p):
    """-> theta, hist [36], (c, s), flat"""
    h = histogram(oracle, p)
    theta, flat = peak(h)
    return theta, h, cos_sin(theta), flat


def rotate(A, theta, flat=False):
    """step 6: A' = A R(theta) in float32, left to right; the frame stays bit for bit when the histogram was flat"""
    A = np.asarray(A, f32)
    if flat:
        return A.copy()
    c, s = cos_sin(theta)
    a11, a12, a21, a22 = A
    return np.array([a11 * c + a12 * s, a12 * c - a11 * s, a21 * c + a22 * s, a22 * c - a21 * s], f32)


def describe_one(oracle, handle, plane, x, y, s, A_up):
    """One keypoint whose up-is-up matrix is A_up -> (described, A', desc[128] or None, theta or None).  Described iff
    normalizeAffine accepts it in both passes."""
    rej, patch = handle.normalize_affine(plane, x, y, s, A_up)
    if rej:
        return False, None, None, None
    theta, _, _, flat = estimate(oracle, patch)
    A2 = rotate(A_up, theta, flat)
    rej, patch = handle.normalize_affine(plane, x, y, s, A2)
    if rej:
        return False, A2, None, theta
    return True, A2, handle.sift(patch), theta


def oriented_from_shapes(oracle, plane, rec, params=None):
    """hesaff_describe_regions(HESAFF_FROM_SHAPES) with orientation on, for REGION_DTYPE records on a float grey plane:
    -> expected output records and keys (as tests/test_describe_regions.py's oracle_describe lays them out)."""
    handle = oracle.OracleHandle(params)
    pd0 = 0.5 if params is not None and params.upscaleInputImage else 1.0
    out = rec.copy()
    keys = []
    for k in range(len(rec)):
        r = rec[k]
        out[k]["pixelDistance"] = f32(pd0 * 2 ** int(r["octave"]))
        out[k]["reserved"] = 0
        out[k]["key"] = -1
        A = np.array([r["a11"], r["a12"], r["a21"], r["a22"]], f32)
        oracle.lib().ho_rectify(A)
        ok, A2, desc, _ = describe_one(oracle, handle, plane, r["x"], r["y"], r["s"], A)
        out[k]["outcome"] = 2 if ok else 1
        if not ok:
            continue
        out[k]["key"] = len(keys)
        key = np.zeros((), _binding.KEYPOINT_DTYPE)
        key["x"], key["y"], key["s"], key["response"], key["type"] = r["x"], r["y"], r["s"], r["response"], r["type"]
        key["a11"], key["a12"], key["a21"], key["a22"] = A2
        key["desc"] = desc
        keys.append(key)
    return out, (np.stack(keys) if keys else np.zeros(0, _binding.KEYPOINT_DTYPE))


def oriented_run(oracle, gray):
    """The whole chain on one float grey image: the oracle's Hessian keypoints and affine shapes, then the oriented description of
    every converged one.  -> (regions REGION_DTYPE in the reference's order, keys KEYPOINT_DTYPE, n_hessian)."""
    run = oracle.OracleRun(gray)
    hf, hi = run.hessian()
    U, ai = run.affine()
    n = run.n_hessian
    rec = np.zeros(n, _binding.REGION_DTYPE)
    handle = oracle.OracleHandle()
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
        ok, A2, desc, _ = describe_one(oracle, handle, gray, hf[k, 0], hf[k, 1], hf[k, 2], A)
        rec[k]["outcome"] = 2 if ok else 1
        if not ok:
            continue
        rec[k]["key"] = len(keys)
        key = np.zeros((), _binding.KEYPOINT_DTYPE)
        key["x"], key["y"], key["s"], key["response"], key["type"] = hf[k, 0], hf[k, 1], hf[k, 2], hf[k, 4], hi[k, 0]
        key["a11"], key["a12"], key["a21"], key["a22"] = A2
        key["desc"] = desc
        keys.append(key)
    return rec, (np.stack(keys) if keys else np.zeros(0, _binding.KEYPOINT_DTYPE)), n
