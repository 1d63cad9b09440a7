"""ctypes binding of the CPU oracle (oracle/libhesaff_oracle.so).

Test infrastructure only: imported by tests/, __graft_entry__.smoke() and bench.py's
cpu_baseline leg.  Nothing under hesaff_amd/ imports this module.
"""
import ctypes as C
import os
import subprocess

import numpy as np

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SO = os.path.join(_ROOT, "oracle", "libhesaff_oracle.so")

f32p = np.ctypeslib.ndpointer(dtype=np.float32, flags="C_CONTIGUOUS")
i32p = np.ctypeslib.ndpointer(dtype=np.int32, flags="C_CONTIGUOUS")
u32p = np.ctypeslib.ndpointer(dtype=np.uint32, flags="C_CONTIGUOUS")
u8p = np.ctypeslib.ndpointer(dtype=np.uint8, flags="C_CONTIGUOUS")


def build():
    src = os.path.join(_ROOT, "oracle", "hesaff_oracle.cpp")
    if (not os.path.exists(_SO)) or os.path.getmtime(_SO) < os.path.getmtime(src):
        subprocess.check_call(["make", "-C", os.path.join(_ROOT, "oracle")], stdout=subprocess.DEVNULL)
    return _SO


_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    L = C.CDLL(build())
    L.ho_gauss_ksize.argtypes = [C.c_float]; L.ho_gauss_ksize.restype = C.c_int
    L.ho_gauss_kernel.argtypes = [C.c_int, C.c_float, f32p]
    L.ho_gaussian_blur.argtypes = [f32p, C.c_int, C.c_int, C.c_float, f32p]
    L.ho_hessian_response.argtypes = [f32p, C.c_int, C.c_int, C.c_float, f32p]
    L.ho_half_image.argtypes = [f32p, C.c_int, C.c_int, f32p]
    L.ho_double_image.argtypes = [f32p, C.c_int, C.c_int, f32p]
    L.ho_gray_from_u8.argtypes = [u8p, C.c_int, C.c_int, f32p]
    L.ho_interpolate.argtypes = [f32p, C.c_int, C.c_int] + [C.c_float] * 6 + [f32p, C.c_int, C.c_int]
    L.ho_interpolate.restype = C.c_int
    L.ho_solve_linear3x3.argtypes = [f32p, f32p]
    L.ho_inv_sqrt.argtypes = [f32p, f32p]
    L.ho_get_eigenvalues.argtypes = [C.c_float] * 4 + [f32p]; L.ho_get_eigenvalues.restype = C.c_int
    L.ho_rectify.argtypes = [f32p]
    L.ho_gauss_mask.argtypes = [C.c_int, f32p]
    L.ho_circ_gauss_mask.argtypes = [C.c_int, f32p]
    L.ho_sift_tables.argtypes = [i32p, i32p, f32p, f32p]
    L.ho_atan2f.argtypes = [C.c_float, C.c_float]; L.ho_atan2f.restype = C.c_float
    L.ho_pow2f.argtypes = [C.c_float]; L.ho_pow2f.restype = C.c_float
    L.ho_find_affine_shape.argtypes = [f32p, C.c_int, C.c_int] + [C.c_float] * 4 + [f32p, i32p]
    L.ho_find_affine_shape.restype = C.c_int
    L.ho_normalize_affine.argtypes = [f32p, C.c_int, C.c_int] + [C.c_float] * 3 + [f32p, f32p]
    L.ho_normalize_affine.restype = C.c_int
    L.ho_sift.argtypes = [f32p, f32p]
    L.ho_create.restype = C.c_void_p
    L.ho_destroy.argtypes = [C.c_void_p]
    L.ho_set_keep_planes.argtypes = [C.c_void_p, C.c_int]
    L.ho_set_detect_only.argtypes = [C.c_void_p, C.c_int]
    L.ho_detect.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int]
    L.ho_set_params.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int, C.c_float, C.c_float, C.c_float]
    L.ho_set_upscale.argtypes = [C.c_void_p, C.c_int]
    L.ho_h_find_affine_shape.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int] + [C.c_float] * 4 + [f32p, i32p]
    L.ho_h_find_affine_shape.restype = C.c_int
    L.ho_h_normalize_affine.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int] + [C.c_float] * 3 + [f32p, f32p]
    L.ho_h_normalize_affine.restype = C.c_int
    L.ho_h_sift.argtypes = [C.c_void_p, f32p, f32p]
    L.ho_h_sift_parts.argtypes = [C.c_void_p, f32p, f32p, f32p, f32p]
    for n in ("ho_num_hessian", "ho_num_keys", "ho_num_octaves"):
        getattr(L, n).argtypes = [C.c_void_p]; getattr(L, n).restype = C.c_int
    L.ho_num_candidates.argtypes = [C.c_void_p]; L.ho_num_candidates.restype = C.c_long
    L.ho_get_hessian.argtypes = [C.c_void_p, C.c_int, f32p, i32p]
    L.ho_get_affine.argtypes = [C.c_void_p, C.c_int, f32p, i32p]
    L.ho_get_key.argtypes = [C.c_void_p, C.c_int, f32p, i32p, u8p]
    L.ho_get_keys.argtypes = [C.c_void_p, f32p, i32p, u8p]
    L.ho_plane_dims.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.ho_get_plane.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, f32p]
    L.ho_export.argtypes = [C.c_void_p, C.c_char_p, C.c_long]; L.ho_export.restype = C.c_long
    L.ho_ellipse.argtypes = [f32p, C.c_float, f32p]
    L.ho_h_detect_planes.argtypes = [C.c_void_p, f32p, f32p, C.c_int, C.c_int]
    L.ho_set_trace.argtypes = [C.c_void_p, C.c_int]
    L.ho_num_trace.argtypes = [C.c_void_p]; L.ho_num_trace.restype = C.c_int
    L.ho_get_trace.argtypes = [C.c_void_p, i32p, u32p]
    L.ho_get_thresholds.argtypes = [C.c_void_p, f32p]
    L.ho_h_affine_trace.argtypes = [C.c_void_p, f32p, C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_int, u32p, i32p, f32p]
    L.ho_h_affine_trace.restype = C.c_int
    L.ho_affine_tail.argtypes = [C.c_int, f32p, f32p, f32p, C.c_float, f32p, i32p]
    _lib = L
    return L


def gray_from_u8(img):
    """hesaff.cpp:138-148 grey conversion; img is HxW (grey) or HxWx3 (BGR) uint8."""
    img = np.ascontiguousarray(img, dtype=np.uint8)
    ch = 1 if img.ndim == 2 else 3
    out = np.empty(img.shape[:2], dtype=np.float32)
    lib().ho_gray_from_u8(img.reshape(-1), out.size, ch, out.reshape(-1))
    return out


def set_params(h, params):
    """Copy the reference-side fields of a hesaff_params-like object (hesaff_amd.Params) into an oracle handle."""
    lib().ho_set_params(h, params.threshold, params.edgeEigenValueRatio, params.initialSigma, int(params.maxIterations),
                        params.convergenceThreshold, params.mrSize, params.maxBinValue)
    lib().ho_set_upscale(h, int(getattr(params, "upscaleInputImage", 0)))


class OracleHandle:
    """An oracle object with (optionally non-default) parameters, for the stage-level functions."""

    def __init__(self, params=None):
        self.h = lib().ho_create()
        if params is not None:
            set_params(self.h, params)

    def __del__(self):
        if getattr(self, "h", None):
            lib().ho_destroy(self.h)
            self.h = None

    def normalize_affine(self, gray, x, y, s, A):
        patch = np.zeros(41 * 41, np.float32)
        rej = lib().ho_h_normalize_affine(self.h, gray, gray.shape[0], gray.shape[1], float(x), float(y), float(s),
                                          np.ascontiguousarray(A, np.float32), patch)
        return rej, patch.reshape(41, 41)

    def find_affine_shape(self, blur, x, y, s, pd):
        A = np.zeros(4, np.float32); it = np.zeros(1, np.int32)
        conv = lib().ho_h_find_affine_shape(self.h, blur, blur.shape[0], blur.shape[1], float(x), float(y), float(s), float(pd), A, it)
        return conv, A, int(it[0])

    def affine_trace(self, blur, x, y, s, pd, cap=64):
        """findAffineShape with a record per iteration entered -> AffineTrace"""
        blur = np.ascontiguousarray(blur, np.float32)
        rec = np.zeros((cap, AFT_WORDS), np.uint32); n = np.zeros(1, np.int32); U = np.zeros(4, np.float32)
        kind = lib().ho_h_affine_trace(self.h, blur, blur.shape[0], blur.shape[1], float(x), float(y), float(s), float(pd), cap,
                                       rec.reshape(-1), n, U)
        return AffineTrace(kind, int(n[0]), U, rec[:min(int(n[0]), cap)].copy())

    def sift(self, patch):
        p = np.ascontiguousarray(patch, np.float32).reshape(-1).copy()
        vec = np.zeros(128, np.float32)
        lib().ho_h_sift(self.h, p, vec)
        return vec.astype(np.uint8)

    def sift_parts(self, patch):
        """-> meanvar[2] (mean and `var` of photometricallyNormalize), hist[128] (before normalizeVec), desc[128] u8."""
        p = np.ascontiguousarray(patch, np.float32).reshape(-1).copy()
        mv = np.zeros(2, np.float32); hist = np.zeros(128, np.float32); vec = np.zeros(128, np.float32)
        lib().ho_h_sift_parts(self.h, p, mv, hist, vec)
        return mv, hist, vec.astype(np.uint8)


# exits of findAffineShape (AffExit), the states of one pass of its tail (AffTailState) and an iteration's record (AFT_WORDS)
AX_CONVERGED, AX_NO_REAL_EIGEN, AX_ANISOTROPY, AX_MAX_ITER = range(4)
AX_NAMES = ["converged", "no-real-eigen", "anisotropy", "max-iter"]
AT_CONTINUE, AT_NO_REAL_EIGEN, AT_ANISOTROPY, AT_CONVERGED = range(4)
AFT_WORDS = 18


class AffineTrace:
    """kind (AX_*), n_iter (iterations entered), U (the matrix at the exit), and per iteration entered: abc_in[3], abc[3], l[2] (invSqrt's),
    ratio (eigen_ratio_act), Us[4] (U after the update), ev[2] (getEigenvalues' l1, l2), max_coord (largest finite |tap coordinate|) as
    float32 arrays over the bits the oracle had; outside (taps that fell outside) and state (AT_*) as integers."""

    def __init__(self, kind, n_iter, U, rec):
        f = rec.view(np.float32)
        self.kind = kind; self.n_iter = n_iter; self.U = U
        self.abc_in = f[:, 0:3]; self.abc = f[:, 3:6]; self.l = f[:, 6:8]; self.ratio = f[:, 8]; self.Us = f[:, 9:13]
        self.ev = f[:, 13:15]; self.max_coord = f[:, 15]
        self.outside = rec[:, 16].astype(np.int64); self.state = rec[:, 17].astype(np.int64)

    def result(self):
        """what findAffineShape returns for this trace: (converged, U, iters), zeros where it reports no shape"""
        if self.kind == AX_CONVERGED:
            return 1, self.U.copy(), self.n_iter - 1
        return 0, np.zeros(4, np.float32), 0


def affine_tail(abc, U, ratio_bef, thr):
    """one pass of affine.cpp:72-97 per row -> abc'[n,3], U'[n,4], ratio[n], l[n,4], state[n] (AT_*)"""
    abc = np.ascontiguousarray(abc, np.float32).reshape(-1, 3).copy(); U = np.ascontiguousarray(U, np.float32).reshape(-1, 4).copy()
    ratio = np.ascontiguousarray(ratio_bef, np.float32).reshape(-1).copy()
    n = len(abc)
    assert len(U) == n and len(ratio) == n
    l = np.zeros((n, 4), np.float32); state = np.zeros(n, np.int32)
    lib().ho_affine_tail(n, abc.reshape(-1), U.reshape(-1), ratio, float(np.float32(thr)), l.reshape(-1), state)
    return abc, U, ratio, l, state


# exits of localizeKeypoint in a trace record (TraceExit, oracle/hesaff_oracle.cpp)
TX_KEPT, TX_EDGE_HIGH, TX_EDGE_NEG, TX_NAN, TX_OUT_RIGHT, TX_OUT_DOWN, TX_OUT_LEFT, TX_OUT_UP, TX_SHIFT, TX_WEAK, TX_TAKEN = range(11)
TX_NAMES = ["kept", "edge>=threshold", "edge<0", "nan", "out-right", "out-down", "out-left", "out-up", "|b|>1.5", "<finalThreshold", "taken"]


def thresholds(params=None):
    """-> (positiveThreshold, finalThreshold, edgeScoreThreshold) as float32, of the oracle with these parameters"""
    o = OracleHandle(params)
    t = np.zeros(3, np.float32)
    lib().ho_get_thresholds(o.h, t)
    return t[0], t[1], t[2]


class PlanesRun:
    """The extrema scans and localizeKeypoint on caller-supplied planes of one octave (L, R: [5, rows, cols] float32), with the trace."""

    def __init__(self, L, R, params=None):
        lb = lib()
        L = np.ascontiguousarray(L, np.float32); R = np.ascontiguousarray(R, np.float32)
        assert L.shape == R.shape and L.ndim == 3 and L.shape[0] == 5
        o = OracleHandle(params)
        lb.ho_set_trace(o.h, 1)
        lb.ho_h_detect_planes(o.h, L.reshape(-1), R.reshape(-1), L.shape[1], L.shape[2])
        n = lb.ho_num_hessian(o.h)
        self.f = np.zeros((n, 6), np.float32); self.i = np.zeros((n, 5), np.int32)
        for k in range(n):
            lb.ho_get_hessian(o.h, k, self.f[k], self.i[k])
        nt = lb.ho_num_trace(o.h)
        self.trace_i = np.zeros((nt, 17), np.int32); self.trace_u = np.zeros((nt, 5), np.uint32)
        if nt:
            lb.ho_get_trace(o.h, self.trace_i.reshape(-1), self.trace_u.reshape(-1))
        self.n_candidates = lb.ho_num_candidates(o.h)

    def trace_at(self, level, r0, c0):
        """the trace record of candidate (level, r0, c0) as (ints[17], bits[5]), or None when it was no candidate.
        ints = level, r0, c0, iterations, final r, final c, exit (TX_*), then (r, c) of each iteration's centre (-1: not entered)"""
        t = self.trace_i
        m = np.flatnonzero((t[:, 0] == level) & (t[:, 1] == r0) & (t[:, 2] == c0))
        assert len(m) <= 1
        return (self.trace_i[m[0]], self.trace_u[m[0]]) if len(m) else None


class OracleRun:
    """Full reference-order pipeline on one float32 grey image."""

    def __init__(self, gray, keep_planes=False, detect_only=False, params=None):
        L = lib()
        gray = np.ascontiguousarray(gray, dtype=np.float32)
        self.h = L.ho_create()
        if params is not None:
            set_params(self.h, params)
        L.ho_set_keep_planes(self.h, int(keep_planes))
        L.ho_set_detect_only(self.h, int(detect_only))
        L.ho_detect(self.h, gray, gray.shape[0], gray.shape[1])
        self.n_hessian = L.ho_num_hessian(self.h)
        self.n_keys = L.ho_num_keys(self.h)
        self.n_candidates = L.ho_num_candidates(self.h)

    def __del__(self):
        if getattr(self, "h", None):
            lib().ho_destroy(self.h)
            self.h = None

    def hessian(self):
        """-> (f[n,6] = x,y,s,pd,response,0 ; i[n,5] = type,octave,level,r0,c0)"""
        f = np.zeros((self.n_hessian, 6), np.float32)
        i = np.zeros((self.n_hessian, 5), np.int32)
        for k in range(self.n_hessian):
            lib().ho_get_hessian(self.h, k, f[k], i[k])
        return f, i

    def affine(self):
        """-> (U[n,4] un-rectified, i[n,2] = converged, iters)"""
        f = np.zeros((self.n_hessian, 4), np.float32)
        i = np.zeros((self.n_hessian, 2), np.int32)
        for k in range(self.n_hessian):
            lib().ho_get_affine(self.h, k, f[k], i[k])
        return f, i

    def keys(self):
        """-> geom[n,8] = x,y,s,a11,a12,a21,a22,response ; type[n] ; desc[n,128] u8"""
        n = self.n_keys
        g = np.zeros((n, 8), np.float32)
        t = np.zeros((n,), np.int32)
        d = np.zeros((n, 128), np.uint8)
        if n:
            lib().ho_get_keys(self.h, g, t, d)
        return g, t, d

    def key_sources(self):
        n = self.n_keys
        src = np.zeros(n, np.int32)
        f = np.zeros(8, np.float32); i = np.zeros(2, np.int32); d = np.zeros(128, np.uint8)
        for k in range(n):
            lib().ho_get_key(self.h, k, f, i, d)
            src[k] = i[1]
        return src

    def n_octaves(self):
        return lib().ho_num_octaves(self.h)

    def plane(self, octave, which, level):
        r = C.c_int(); c = C.c_int()
        lib().ho_plane_dims(self.h, octave, C.byref(r), C.byref(c))
        out = np.empty((r.value, c.value), np.float32)
        lib().ho_get_plane(self.h, octave, which, level, out)
        return out

    def export_text(self):
        n = lib().ho_export(self.h, None, 0)
        buf = C.create_string_buffer(n)
        lib().ho_export(self.h, buf, n)
        return buf.raw[:n]
