"""Constructed inputs for the affine shape iteration at the edges of its domain (tests/test_affine_edges.py).

Plain numpy, seeded, no files, no GPU.  A CASE is one keypoint (x, y, s, pixelDistance) on one float32 plane of at most 64 x 64.
Every case carries a CLAIM under the default parameters - how findAffineShape (affine.cpp:35-100) leaves its loop and after how
many iterations, for some cases the taps that fall outside the plane in every iteration, or the exact U - which the CPU half of
the tests proves with the oracle's trace (Oracle::affineTrace), so the inputs cannot rot; the GPU half runs the same cases
through k_affine_stage and compares every row, converged or not, with the trace's U at the exit.

Families:

  scaled       one smooth converging plane times 2^k.  Bits identical to k = 0 while no product is denormal or infinite, thirteen
               different results where gxx * gxx * v is denormal, and both ends where the sums are 0 or infinite (NaN flow).
  threshold    blob(p): a Gaussian blob whose axis ratio is the float32 p.  Pairs of ADJACENT float32 values of p, found by bisection
               on p's bit pattern against the oracle and written down here, at which (a) eigen_ratio_act crosses
               convergenceThreshold: converged or one more iteration, (b) l1 / l2 of getEigenvalues crosses 6: rejected or going
               on, (c) the keypoint converges in the last iteration maxIterations allows, or not at all.
  flat         a constant plane, a zero plane, a ramp in x only (c == 0 exactly: z = 1 / sqrt(0)), content no tap reaches: a, b, c
               make NaN of invSqrt, every later tap has NaN coordinates and falls outside, the loop runs to maxIterations.
  exact        integer-valued planes, integer centres, s = 1.6 * pd: ratio == 1, the first iteration's taps fall on pixels.
               The paraboloid (x - 32)^2 + (y - 32)^2 converges at l = 0 (its b is the rounding left of 361 cancelling terms); a single
               non-zero pixel gives b == 0 exactly (invSqrt's other branch), with a == c at the centre and a != c beside it; a seeded
               integer plane carries the 19 x 19 window with its last column on cols - 1 (19 taps outside), one pixel further in
               (none), its first column on column 0 (none: floor(w) >= 0) and one pixel further out (19), the same for rows,
               and the four corners.
  limits       positions at +-2^20 on every side (every tap zero), s = 2^20 (only the centre tap inside: b == 0, converged with
               U = identity at l = 0), the smallest s that still converges and its float32 neighbour below, s = 0,
               pixelDistance 0.5 and 8, planes of 2 x 2 and 13 x 13, x = y = -0.0.
  nonfinite    NaN and infinite x, y, s.  The reference's x86 build and the library treat such a tap as outside; the claims are
               the exit and the NaN-ness of U only.
  anisotropic  ridges: rejected by l1 / l2 > 6 in iteration 0, 1 and later.
  no_real_eigen  getEigenvalues' delta1 < 0: blobs found by a scan of blob(p) (no_real_eigen_scan: 1800 keypoints - three angles,
               three widths, forty axis ratios, five keypoints - meet the exit nine times, always after iteration 10).
  mixed        orders of the above (mixed_lists): see there.

PSETS are the parameter sets of the GPU half, one context each; the claims written here are for "default", the other sets are
checked against the trace under their own parameters and against what they were chosen to change.
"""
import functools

import numpy as np

F = np.float32
N = 64
CONVERGED, NO_REAL_EIGEN, ANISOTROPY, MAX_ITER = range(4)   # the oracle's AffExit
KIND_NAMES = ("converged", "no-real-eigen", "anisotropy", "max-iter")
THR = F(0.05)        # affine.h:41
MAX_ITERATIONS = 16  # affine.h:39
SLOTS = 16           # keypoint slots of a wavefront of k_affine_stage
STAGE_BLOCKS = 1536  # the stage launch's grid limit

PSETS = {
    "default": {},
    "maxit1": dict(maxIterations=1),
    "maxit2": dict(maxIterations=2),
    "maxit40": dict(maxIterations=40),
    "thr0": dict(convergenceThreshold=0.0),     # nothing converges
    "thr1": dict(convergenceThreshold=1.0),     # everything finite converges at l = 0
}


def bits(v):
    return int(np.array([v], F).view(np.uint32)[0])


def from_bits(u):
    return np.array([u], np.uint32).view(F)[0]


class Case:
    """name, family, plane (a key of planes()), kp = (x, y, s, pd); the claim: kind, n_iter (iterations entered), and where given
    outside (taps outside per iteration), U (the exact matrix at the exit), nan_U (every element of U at the exit is NaN)."""

    def __init__(self, name, family, plane, kp, kind, n_iter, outside=None, U=None, nan_U=False):
        self.name = name; self.family = family; self.plane = plane
        self.kp = tuple(F(v) for v in kp)
        self.kind = kind; self.n_iter = n_iter; self.outside = outside; self.U = U; self.nan_U = nan_U

    def __repr__(self):
        return "Case(%s on %s at %s)" % (self.name, self.plane, tuple(float(v) for v in self.kp))


# ----------------------------------------------------------------------------------------------------------------------
# planes
# ----------------------------------------------------------------------------------------------------------------------
def two_blobs():
    """the smooth converging plane of the scaled family: two overlapping Gaussian blobs, peak about 200"""
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    g1 = np.exp(-(((xx - 30.0) / 7.0) ** 2 + ((yy - 33.0) / 4.5) ** 2) / 2)
    g2 = np.exp(-(((xx - 40.0) / 5.0) ** 2 + ((yy - 24.0) / 6.0) ** 2) / 2)
    return (200.0 * g1 + 120.0 * g2).astype(F)


def blob(p, theta=0.4, sx=3.0):
    """a Gaussian blob at (32, 32), peak 200, with axis sigmas sx and sx * p (p: a float32), turned by theta"""
    p = float(F(p))
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    c, s = np.cos(theta), np.sin(theta)
    u = (xx - 32.0) * c + (yy - 32.0) * s
    v = -(xx - 32.0) * s + (yy - 32.0) * c
    return (200.0 * np.exp(-((u / sx) ** 2 + (v / (sx * p)) ** 2) / 2)).astype(F)


def ridge(theta, width, wobble=0.0):
    """a straight ridge through (32, 32) along the direction theta, Gaussian profile of sigma `width`, peak 200; wobble > 0 lets the
    peak fall off along the ridge with sigma width / wobble"""
    yy, xx = np.mgrid[0:N, 0:N].astype(np.float64)
    c, s = np.cos(theta), np.sin(theta)
    u = (xx - 32.0) * c + (yy - 32.0) * s
    v = -(xx - 32.0) * s + (yy - 32.0) * c
    return (200.0 * np.exp(-(v / width) ** 2 / 2 - (u * wobble / width) ** 2 / 2)).astype(F)


def paraboloid():
    yy, xx = np.mgrid[0:N, 0:N].astype(np.int64)
    return ((xx - 32) ** 2 + (yy - 32) ** 2).astype(F)


def integer_plane(rows=N, cols=N, seed=5):
    """seeded integers 0..255 on a coarse grid, linearly interpolated and rounded: integer-valued with gradients everywhere"""
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, size=(rows // 4 + 2, cols // 4 + 2)).astype(np.float64)
    yy, xx = np.mgrid[0:rows, 0:cols].astype(np.float64) / 4.0
    y0 = yy.astype(np.int64); x0 = xx.astype(np.int64); fy = yy - y0; fx = xx - x0
    v = (1 - fy) * ((1 - fx) * g[y0, x0] + fx * g[y0, x0 + 1]) + fy * ((1 - fx) * g[y0 + 1, x0] + fx * g[y0 + 1, x0 + 1])
    return np.rint(v).astype(F)


def scaled(plane, k):
    """plane * 2^k, rounded once to float32 (exact while nothing is denormal)"""
    return (plane.astype(np.float64) * 2.0 ** k).astype(F)


# k of the scaled family, with what the oracle makes of two_blobs() * 2^k at SCALED_KP.  k = 0 converges after four iterations.
SCALED_KP = (32.3, 31.2, 4.0, 1.0)
SCALED_SAME = (0, -1, -20, -40, -62, -65, 1, 20, 40, 55)            # bits identical to k = 0
SCALED_DENORMAL = (-66, -67, -68, -69, -70, -71, -72, -73, -74, -75, -76, -77, -78)   # every one different from k = 0 and from the others
SCALED_GONE = (-79, -80, -100, -126, 56, 60, 100, 120)               # NaN flow: the sums are 0, or infinite
SCALED_CLAIMS = {-77: (MAX_ITER, 16), -78: (CONVERGED, 3)}           # (all other k of SAME and DENORMAL: converged, 4 iterations)

# threshold pairs: (theta, sx, keypoint, bits of p below, bits of p above = below + 1), and the claims of the two
_KP = (32.3, 31.2, 4.0, 1.0)
_KP2 = (30.2, 33.9, 5.0, 1.0)
THRESHOLD = {
    # (a) eigen_ratio_act of iteration 0 is 0.04999995 | >= 0.05: converged at l = 0, or two iterations later
    "a/l=0": (0.4, 3.0, _KP, 1065841071, ((CONVERGED, 1), (CONVERGED, 3))),
    # (a) eigen_ratio_act of iteration 2 is 0.04999995 | >= 0.05: converged at l = 3 or at l = 4
    "a/l=3": (0.4, 3.0, _KP, 1074788215, ((CONVERGED, 4), (CONVERGED, 5))),
    # (b) l1 / l2 of iteration 0 is <= 6 | 6.000002: going on (to an ANISOTROPY exit ten iterations later), or rejected at once
    "b/l=0": (0.4, 3.0, _KP, 1082924183, ((ANISOTROPY, 11), (ANISOTROPY, 1))),
    # (b) l1 / l2 of iteration 10 is 5.9999566 | 6.000003: going on (to a NO_REAL_EIGEN exit in the next iteration), or rejected
    "b/late": (0.4, 3.0, _KP, 1082750565, ((NO_REAL_EIGEN, 12), (ANISOTROPY, 11))),
    # (c) eigen_ratio_act of iteration 14 is 0.04999989 | 0.05000132: converged in iteration 15, the last one allowed, or never
    "c": (0.4, 3.0, _KP2, 1079228852, ((CONVERGED, 16), (MAX_ITER, 16))),
}
# the iteration (counted from 0) whose decision differs within a pair, and what differs: "ratio" (eigen_ratio_act against
# convergenceThreshold) or "ev" (l1 / l2 of getEigenvalues against 6)
THRESHOLD_AT = {"a/l=0": (0, "ratio"), "a/l=3": (2, "ratio"), "b/l=0": (0, "ev"), "b/late": (10, "ev"), "c": (14, "ratio")}

# the blobs that leave by getEigenvalues: (theta, sx, p, keypoint, claim)
NO_REAL_EIGEN_BLOBS = (
    (0.4, 2.0, 4.2, (32.0, 32.0, 2.5, 1.0), (NO_REAL_EIGEN, 12)),
    (0.4, 4.0, 3.1, (32.0, 32.0, 2.5, 1.0), (NO_REAL_EIGEN, 13)),
    (0.4, 4.0, 3.7, _KP, (NO_REAL_EIGEN, 14)),
    (0.4, 3.0, 3.3, (32.0, 32.0, 2.5, 1.0), (NO_REAL_EIGEN, 16)),
)

# ridges: (theta, width, wobble, keypoint, claim)
ANISOTROPIC = (
    (0.0, 1.0, 0.0, (33.0, 33.5, 2.5, 1.0), (ANISOTROPY, 1)),
    (0.0, 1.0, 0.1, _KP, (ANISOTROPY, 2)),
    (0.0, 1.0, 0.1, (31.0, 32.5, 6.0, 1.0), (ANISOTROPY, 3)),
    (0.3, 1.0, 0.1, (31.0, 32.5, 6.0, 1.0), (ANISOTROPY, 4)),
    (0.3, 4.0, 0.4, (32.0, 32.0, 1.6, 1.0), (ANISOTROPY, 16)),      # in the last iteration allowed
    (1.2, 4.0, 0.3, (33.0, 33.5, 2.5, 1.0), (NO_REAL_EIGEN, 11)),   # a ridge that leaves by getEigenvalues
    (0.0, 1.0, 0.0, (32.0, 32.0, 1.6, 1.0), (MAX_ITER, 16)),        # the centre of an endless ridge along x: a == b == 0 exactly
)


def no_real_eigen_scan():
    """the seeded scan that found NO_REAL_EIGEN_BLOBS: 1800 keypoints (theta, sx, p, keypoint) on blob(p, theta, sx), of which nine
    leave by getEigenvalues (tests/test_affine_edges.py counts them)"""
    for theta in (0.0, 0.4, 0.8):
        for sx in (2.0, 3.0, 4.0):
            for p in np.arange(1.0, 5.0, 0.1):
                for kp in (_KP, (33.5, 30.5, 3.0, 1.0), (32.0, 32.0, 2.5, 1.0), _KP2, (34.0, 34.0, 3.0, 1.0)):
                    yield theta, sx, F(p), kp


@functools.lru_cache(maxsize=None)
def planes():
    """name -> float32 plane (read-only)"""
    P = {}
    base = two_blobs()
    for k in SCALED_SAME + SCALED_DENORMAL + SCALED_GONE:
        P["blobs*2^%d" % k] = scaled(base, k)
    for key, (theta, sx, kp, lo, claims) in THRESHOLD.items():
        for j in (0, 1):
            P["blob/%s/%d" % (key, j)] = blob(from_bits(lo + j), theta, sx)
    for j, (theta, sx, p, kp, claim) in enumerate(NO_REAL_EIGEN_BLOBS):
        P["blob/nre/%d" % j] = blob(p, theta, sx)
    for j, (theta, width, wobble, kp, claim) in enumerate(ANISOTROPIC):
        P["ridge/%d" % j] = ridge(theta, width, wobble)
    P["const"] = np.full((N, N), 77.0, F)
    P["zero"] = np.zeros((N, N), F)
    yy, xx = np.mgrid[0:N, 0:N]
    P["ramp_x"] = (3 * xx).astype(F)
    far = np.zeros((N, N), F)
    far[0:6, 0:6] = integer_plane(6, 6, 9)   # content no tap of a window around (45, 45) reaches
    P["unreached"] = far
    P["paraboloid"] = paraboloid()
    spike = np.zeros((N, N), F)
    spike[32, 32] = 64.0
    P["spike"] = spike
    P["integers"] = integer_plane()
    P["2x2"] = np.array([[1.0, 7.0], [4.0, 2.0]], F)
    P["13x13"] = np.ascontiguousarray(base[27:40, 26:39])
    for a in P.values():
        a.setflags(write=False)
    return P


# ----------------------------------------------------------------------------------------------------------------------
# cases
# ----------------------------------------------------------------------------------------------------------------------
T20 = 2.0 ** 20


def _scaled_cases():
    out = []
    for k in SCALED_SAME + SCALED_DENORMAL:
        kind, n = SCALED_CLAIMS.get(k, (CONVERGED, 4))
        out.append(Case("scaled/%d" % k, "scaled", "blobs*2^%d" % k, SCALED_KP, kind, n))
    for k in SCALED_GONE:
        out.append(Case("scaled/%d" % k, "scaled", "blobs*2^%d" % k, SCALED_KP, MAX_ITER, MAX_ITERATIONS, nan_U=True))
    return out


def _threshold_cases():
    out = []
    for key, (theta, sx, kp, lo, claims) in THRESHOLD.items():
        for j in (0, 1):
            out.append(Case("threshold/%s/%d" % (key, j), "threshold", "blob/%s/%d" % (key, j), kp, claims[j][0], claims[j][1]))
    return out


EXACT_S = 1.6   # s = 1.6 * pd: ratio == 1 (1.6f / (1.6f * 1))

# the 19 x 19 window of iteration 0 against the border of the 64 x 64 integer plane: (name, x, y, taps outside in every iteration)
BORDER_EXACT = (
    ("right_on", 54, 32, (19, 0, 0)), ("right_in", 53, 32, (0, 0, 0)), ("left_on", 9, 32, (0, 38, 38)), ("left_out", 8, 32, (19, 57, 57, 57)),
    ("down_on", 32, 54, (19, 19, 27, 30)), ("down_in", 32, 53, (0, 0, 0, 18)), ("up_on", 32, 9, (0, 19, 19)), ("up_out", 32, 8, (19, 38, 38)),
    ("corner_dr", 54, 54, (37,)), ("corner_ul", 8, 8, (37, 52, 53)), ("corner_ur", 54, 8, (37, 39, 48, 39, 45)), ("corner_dl", 8, 54, (37, 37, 37, 38)),
    ("corner_in_dr", 53, 53, (0, 0, 0)), ("corner_in_ul", 9, 9, (0, 26, 25)),
)

# claims the oracle's trace gave for the cases that name none themselves: name -> (kind, iterations entered).  (Every case of
# BORDER_EXACT converges, after as many iterations as its tuple is long.)
CLAIMS = {
    'exact/spike/off': (CONVERGED, 1),
    'limits/s_min/1': (CONVERGED, 16),
    'limits/s=2^-2': (ANISOTROPY, 1),
    'limits/s=2^-18': (ANISOTROPY, 2),
    'limits/s=2^-21': (CONVERGED, 13),
    'limits/pd=0.5': (CONVERGED, 4),
    'limits/pd=8': (CONVERGED, 4),
    'limits/pd=8/s_large': (CONVERGED, 4),
    'limits/2x2/wide': (CONVERGED, 1),
    'limits/13x13': (CONVERGED, 8),
    'limits/-0': (CONVERGED, 5),
    'limits/-0/blobs': (ANISOTROPY, 8),
    'ordinary/0': (CONVERGED, 4),
    'ordinary/1': (CONVERGED, 5),
    'ordinary/2': (CONVERGED, 4),
    'ordinary/3': (CONVERGED, 4),
    'ordinary/4': (CONVERGED, 5),
    'ordinary/5': (CONVERGED, 4),
}


def _claim(name, default=None):
    return CLAIMS.get(name, default if default is not None else (MAX_ITER, MAX_ITERATIONS))


def _flat_cases():
    nan = dict(nan_U=True)
    out = []
    for pl, kp in (("const", (32.3, 31.2, 4.0, 1.0)), ("zero", (32.3, 31.2, 4.0, 1.0)), ("ramp_x", (32.0, 32.0, EXACT_S, 1.0)),
                   ("ramp_x", (20.0, 40.0, 2 * EXACT_S, 1.0)), ("unreached", (45.0, 45.0, EXACT_S, 1.0)), ("unreached", (44.6, 45.3, 2.0, 1.0))):
        out.append(Case("flat/%s/%d" % (pl, len(out)), "flat", pl, kp, MAX_ITER, MAX_ITERATIONS, **nan))
    return out


def _exact_cases():
    out = [Case("exact/paraboloid", "exact", "paraboloid", (32.0, 32.0, EXACT_S, 1.0), CONVERGED, 1)]
    for name, x, y, outside in BORDER_EXACT:
        out.append(Case("exact/" + name, "exact", "integers", (float(x), float(y), EXACT_S, 1.0), CONVERGED, len(outside), outside=outside))
    # one pixel of 64 in a plane of zeros: gxx is non-zero left and right of it, gyy above and below, never both: b == 0 exactly.
    # At the window's centre a == c as well (U = identity at l = 0); one pixel off the centre a != c.
    out.append(Case("exact/spike", "exact", "spike", (32.0, 32.0, EXACT_S, 1.0), CONVERGED, 1, outside=(0,), U=(1.0, 0.0, 0.0, 1.0)))
    kind, n = _claim("exact/spike/off")
    out.append(Case("exact/spike/off", "exact", "spike", (31.0, 32.0, EXACT_S, 1.0), kind, n))
    return out


def _limit_cases():
    out = []
    for name, x, y in (("x+", T20, 32.0), ("x-", -T20, 32.0), ("y+", 32.0, T20), ("y-", 32.0, -T20), ("x+y-", T20, -T20), ("x-y+", -T20, T20),
                       ("x+y+", T20, T20), ("x-y-", -T20, -T20)):
        c = Case("limits/pos/" + name, "limits", "blobs*2^0", (x, y, 4.0, 1.0), MAX_ITER, MAX_ITERATIONS, outside=(361,) * MAX_ITERATIONS, nan_U=True)
        out.append(c)
    # s = 2^20: the taps are 655360 pixels apart, the centre tap alone is inside, every gradient of the 19 x 19 tile is zero but the
    # four around the centre: a == c, b == 0
    out.append(Case("limits/s=2^20", "limits", "blobs*2^0", (32.3, 31.2, T20, 1.0), CONVERGED, 1, outside=(360,), U=(1.0, 0.0, 0.0, 1.0)))
    out.append(Case("limits/s=2^20/integers", "limits", "integers", (17.0, 40.0, T20, 1.0), CONVERGED, 1, outside=(360,), U=(1.0, 0.0, 0.0, 1.0)))
    for j in (0, 1):
        kind, n = _claim("limits/s_min/%d" % j)
        out.append(Case("limits/s_min/%d" % j, "limits", "blobs*2^0", (32.3, 31.2, from_bits(S_MIN_BITS + j), 1.0), kind, n))
    out.append(Case("limits/s=0", "limits", "blobs*2^0", (32.3, 31.2, 0.0, 1.0), MAX_ITER, MAX_ITERATIONS, nan_U=True))
    for e in (-2, -18, -21, -40, -149):
        kind, n = _claim("limits/s=2^%d" % e)
        out.append(Case("limits/s=2^%d" % e, "limits", "blobs*2^0", (32.3, 31.2, 2.0 ** e, 1.0), kind, n, nan_U=e <= -40))
    for name, pl, kp in (("pd=0.5", "blobs*2^0", (16.15, 15.6, 2.0, 0.5)), ("pd=8", "blobs*2^0", (258.4, 249.6, 32.0, 8.0)),
                         ("pd=8/s_large", "blobs*2^0", (258.4, 249.6, 60.0, 8.0)), ("2x2", "2x2", (0.5, 0.5, 0.1, 1.0)),
                         ("2x2/wide", "2x2", (0.5, 0.5, 1.6, 1.0)), ("13x13", "13x13", (6.3, 6.2, 0.4, 1.0)), ("13x13/wide", "13x13", (6.0, 6.0, 1.6, 1.0)),
                         ("-0", "integers", (-0.0, -0.0, EXACT_S, 1.0)), ("-0/blobs", "blobs*2^0", (-0.0, -0.0, 4.0, 1.0))):
        kind, n = _claim("limits/" + name)
        out.append(Case("limits/" + name, "limits", pl, kp, kind, n))
    return out


# From s = 4 downwards the keypoint (32.3, 31.2) of two_blobs() converges ever later; S_MIN_BITS are the bits of the largest s (about
# 0.674) at which it no longer does, + 1 those of the smallest at which it still does, in the sixteenth iteration.  (Far below, where
# the window shrinks into the rounding of 32.3 + i * a11, the outcome is noise: two such s are cases of their own.)
S_MIN_BITS = 1059881670


def _nonfinite_cases():
    nan, inf = float("nan"), float("inf")
    out = []
    for name, kp in (("x=nan", (nan, 31.2, 4.0, 1.0)), ("y=nan", (32.3, nan, 4.0, 1.0)), ("s=nan", (32.3, 31.2, nan, 1.0)), ("x=+inf", (inf, 31.2, 4.0, 1.0)),
                     ("y=-inf", (32.3, -inf, 4.0, 1.0)), ("s=+inf", (32.3, 31.2, inf, 1.0)), ("pd=nan", (32.3, 31.2, 4.0, nan)), ("pd=0", (32.3, 31.2, 4.0, 0.0))):
        out.append(Case("nonfinite/" + name, "nonfinite", "blobs*2^0", kp, MAX_ITER, MAX_ITERATIONS, nan_U=True))
    return out


def _anisotropic_cases():
    return [Case("anisotropic/%d" % j, "anisotropic", "ridge/%d" % j, kp, claim[0], claim[1], nan_U=claim[0] == MAX_ITER)
            for j, (th, w, wb, kp, claim) in enumerate(ANISOTROPIC)]


def _nre_cases():
    return [Case("no_real_eigen/%d" % j, "no_real_eigen", "blob/nre/%d" % j, kp, claim[0], claim[1]) for j, (th, sx, p, kp, claim) in enumerate(NO_REAL_EIGEN_BLOBS)]


# ordinary keypoints on two_blobs(): each converges (the claims say after how many iterations)
ORDINARY = ((32.3, 31.2, 4.0, 1.0), (30.5, 33.0, 3.0, 1.0), (40.2, 24.4, 3.5, 1.0), (35.0, 28.0, 5.0, 1.0), (28.7, 34.1, 2.5, 1.0), (38.0, 26.5, 4.5, 1.0))


def _ordinary_cases():
    out = []
    for j, kp in enumerate(ORDINARY):
        kind, n = _claim("ordinary/%d" % j)
        out.append(Case("ordinary/%d" % j, "ordinary", "blobs*2^0", kp, kind, n))
    return out


@functools.lru_cache(maxsize=None)
def cases():
    """every case, in a fixed order"""
    out = (_scaled_cases() + _threshold_cases() + _flat_cases() + _exact_cases() + _limit_cases() + _nonfinite_cases() + _anisotropic_cases()
           + _nre_cases() + _ordinary_cases())
    names = [c.name for c in out]
    assert len(set(names)) == len(names)
    return tuple(out)


def case(name):
    return next(c for c in cases() if c.name == name)


# ----------------------------------------------------------------------------------------------------------------------
# mixed orders, all on two_blobs(): rows of keypoints and, per row, the name of the case it repeats
# ----------------------------------------------------------------------------------------------------------------------
ODD = ("limits/pos/x+", "nonfinite/x=nan", "limits/pos/x-y+", "nonfinite/s=+inf", "nonfinite/y=-inf", "limits/s=0", "limits/pos/y-", "nonfinite/pd=nan")
BIG_ROWS = 2 * SLOTS * STAGE_BLOCKS   # every slot of every block of the stage launch takes a second keypoint


def big_position(r):
    """the position in its block's walk of row r of a list of BIG_ROWS rows (hs_affine_groups: 1536 blocks, a multiple of 8, so each
    XCD takes a contiguous eighth of the list and its 192 blocks stride inside it)"""
    return (r % (BIG_ROWS // 8)) // (STAGE_BLOCKS // 8)


@functools.lru_cache(maxsize=None)
def mixed_lists():
    """name -> tuple of case names, every case on the plane "blobs*2^0".
    batch/j (j = 0..3): sixteen rows = one block, slot = row; every batch of four slots (rows 4q .. 4q+3) holds one NaN-flow or
        far-outside keypoint at position j beside three ordinary ones: the batch's one ballot gives the three the tested taps.
    batch/j/short: the same list without its last two rows (a batch with idle slots).
    refill: BIG_ROWS rows.  Positions 0..15 of every block's walk, the keypoints its slots start on, are ordinary ones, which
        converge; position 16, the first refill of the block, therefore enters a slot whose previous keypoint converged, and is a
        NaN-flow or far-outside keypoint; of the positions behind it one in four is."""
    ordinary = ["ordinary/%d" % j for j in range(len(ORDINARY))]
    L = {}
    for j in range(4):
        rows = []
        for q in range(4):
            o = [ordinary[(3 * q + t) % len(ordinary)] for t in range(3)]
            o.insert(j, ODD[(q + 4 * (j & 1)) % len(ODD)])
            rows += o
        L["batch/%d" % j] = tuple(rows)
        L["batch/%d/short" % j] = tuple(rows[:-2])
    rows = []
    for r in range(BIG_ROWS):
        p = big_position(r)
        if p >= SLOTS and (p - SLOTS) % 4 == 0:
            rows.append(ODD[(r // 7) % len(ODD)])
        else:
            rows.append(ordinary[(r + r // len(ordinary)) % len(ordinary)])
    L["refill"] = tuple(rows)
    return L
