"""Constructed inputs for the descriptor and patch kernels at the edges of their domains (tests/test_stage_edges.py).

Plain numpy, seeded, no GPU.  The CPU tests prove with the oracle alone that every input hits what it claims (which body
of k_sift_grad, which operands of atan2f, which window kernel); the GPU tests run the same inputs through the kernels.

Patch families (each function returns float32 [k][41][41]; the `*_names` functions give one label per patch):

  flat         var < 1e-4 (helpers.cpp:270): the patch keeps its raw pixels and k_sift_grad takes the general forms
  threshold    one pattern at the scales where the oracle's float32 `var` crosses 1e-4
  saturating   var >= 1e-4 with exact orientations, zero gradients, clamped pixels
  ordinary     128 + c * pattern_k: the photometrically normalised body as the pipeline meets it

A patch whose non-zero pixels all lie outside the circular mask has mean = var = 0 over the masked pixels and is
therefore FLAT, whatever its content: the border-only patches and the spikes at radius 20 and 21 are part of `flat`
(group "outside"), not of `saturating`.
"""
import functools

import numpy as np

F = np.float32
PS = 41
HALF = 20
MR_SIZE = F(3.0 * np.sqrt(3.0))   # affine.h:44, the default hesaff_params.mrSize

FLAT_EXPONENTS = (-14, -20, -40, -60, -62, -63, -64, -66, -70, -73, -74, -75, -76, -100, -126, -140, -149)
FLAT_OFFSETS = (1.0, 100.0, 255.0)
FLAT_CONSTANTS = (0.0, -0.0, 77.0, 255.0, 2.0 ** 20)


def circular_mask():
    """True where computeCircularGaussMask (helpers.cpp:131) is positive: squared distance from the centre below 20^2."""
    yy, xx = np.mgrid[0:PS, 0:PS]
    return (yy - HALF) ** 2 + (xx - HALF) ** 2 < HALF * HALF


def stencil_reach():
    """True for every pixel some masked pixel's gradient stencil reads."""
    m = circular_mask()
    r = np.zeros_like(m)
    r[:, 1:] |= m[:, :-1]; r[:, :-1] |= m[:, 1:]; r[1:, :] |= m[:-1, :]; r[:-1, :] |= m[1:, :]
    return r


def gradients(patches):
    """(gy, gx) of every pixel in float32, the reference's stencil (siftdesc.cpp:123-134): central differences without the
    1/2, one-sided at the frame."""
    p = np.ascontiguousarray(patches, F).reshape(-1, PS, PS)
    gx = np.empty_like(p); gy = np.empty_like(p)
    gx[:, :, 1:-1] = p[:, :, 2:] - p[:, :, :-2]
    gx[:, :, 0] = p[:, :, 1] - p[:, :, 0]; gx[:, :, -1] = p[:, :, -1] - p[:, :, -2]
    gy[:, 1:-1, :] = p[:, 2:, :] - p[:, :-2, :]
    gy[:, 0, :] = p[:, 1, :] - p[:, 0, :]; gy[:, -1, :] = p[:, -1, :] - p[:, -2, :]
    return gy, gx


def masked_gradients(patches):
    """(gy, gx) of the masked pixels only, flattened."""
    gy, gx = gradients(patches)
    m = circular_mask()
    return gy[:, m].reshape(-1), gx[:, m].reshape(-1)


@functools.lru_cache(maxsize=None)
def patterns():
    """Two seeded patterns with values in about [-1.6, 1.6] (float64; the families scale and round them)."""
    yy, xx = np.mgrid[0:PS, 0:PS].astype(np.float64)
    rng = np.random.default_rng(20240)
    a = np.sin(xx / 3.0) * np.cos(yy / 5.0) + 0.3 * rng.standard_normal((PS, PS))
    b = np.cos(xx / 4.0 + yy / 7.0) * np.sin(yy / 3.0 + 0.5) + 0.3 * rng.standard_normal((PS, PS))
    return a, b


GAP_SPIKE = (14, 23)   # inside the mask, away from its edge


@functools.lru_cache(maxsize=None)
def _flat_items():
    pa = patterns()
    items = []
    for e in FLAT_EXPONENTS:
        for k, p in enumerate(pa):
            items.append(("scale:%d:%d" % (e, k), (p.astype(F).astype(np.float64) * 2.0 ** e).astype(F)))   # one rounding, in the subnormals only
    for off in FLAT_OFFSETS:
        for e in (e for e in FLAT_EXPONENTS if e >= -20):
            for k, p in enumerate(pa):
                items.append(("offset:%g:%d:%d" % (off, e, k), (F(off) + (p * 2.0 ** e).astype(F)).astype(F)))
    for c in FLAT_CONSTANTS:
        items.append(("const:%r" % c, np.full((PS, PS), c, F)))
    # exponent gaps: one pixel at +-2^-9 on a 2^-100 / 2^-140 texture.  With the spike at (r, c): pixel (r, c - 1) has
    # (gy, gx) = (tiny, 2^-9), pixel (r - 1, c) has (2^-9, tiny) and, its two horizontal neighbours made equal, pixel
    # (r + 1, c) has (-2^-9, 0)
    r, c = GAP_SPIKE
    for e in (-100, -140):
        for sgn in (1.0, -1.0):
            t = (pa[0] * 2.0 ** e).astype(F)
            t[r + 1, c + 1] = t[r + 1, c - 1]
            t[r, c] = F(sgn * 2.0 ** -9)
            items.append(("gap:%d:%+d" % (e, int(sgn)), t))
    # non-zero only where no masked pixel's stencil reaches, in row 0 / row 40 / column 0 / column 40: nothing may come out
    reach = stencil_reach()
    rng = np.random.default_rng(20241)
    for name, sl in (("row0", np.s_[0, :]), ("row40", np.s_[PS - 1, :]), ("col0", np.s_[:, 0]), ("col40", np.s_[:, PS - 1])):
        t = np.zeros((PS, PS), F)
        t[sl] = rng.integers(1, 256, PS).astype(F)
        t[reach | circular_mask()] = 0
        assert t.any()
        items.append(("outside:silent:" + name, t))
    # the whole frame at 255 and spikes outside the mask: still flat (the masked pixels are all zero), but the masked pixels
    # next to them see gradients of 255 -- the general body on ordinary operands
    t = np.zeros((PS, PS), F); t[0, :] = 255; t[-1, :] = 255; t[:, 0] = 255; t[:, -1] = 255
    items.append(("outside:frame", t))
    # radius 20 on the axes (a masked neighbour sees it) and radius 21.02 at (9, 19) off them (no masked pixel's stencil reaches it)
    for name, (dy, dx) in (("20:x", (0, 20)), ("20:y", (-20, 0)), ("21:a", (9, 19)), ("21:b", (-19, 9))):
        assert not circular_mask()[HALF + dy, HALF + dx]
        t = np.zeros((PS, PS), F); t[HALF + dy, HALF + dx] = 255
        items.append(("outside:spike:" + name, t))
    return tuple(items)


def flat():
    return np.stack([p for _, p in _flat_items()])


def flat_names():
    return [n for n, _ in _flat_items()]


@functools.lru_cache(maxsize=None)
def _saturating_items():
    yy, xx = np.mgrid[0:PS, 0:PS].astype(np.float64)
    items = []
    # 0/255 step edges, normal at 0, 45, ..., 315 degrees, through the centre and 6 pixels off it.  Integer normals: the
    # diagonal edges are exact staircases (|gy| == |gx|), the axis-parallel ones have gy == +0 or gx == +0 along the edge
    normals = ((1, 0), (1, 1), (0, 1), (-1, 1), (-1, 0), (-1, -1), (0, -1), (1, -1))
    for k, (nx, ny) in enumerate(normals):
        for off in (0, 6):
            d = (xx - HALF) * nx + (yy - HALF) * ny - off
            items.append(("edge:%d:%d" % (45 * k, off), np.where(d > 0, 255.0, 0.0).astype(F)))
    for period in (1, 2):
        items.append(("checker:%d" % period, (255.0 * (((yy // period) + (xx // period)) % 2)).astype(F)))
    for name, r in (("x", xx), ("y", yy), ("d1", xx + yy), ("d2", xx - yy)):
        items.append(("ramp:" + name, (3.0 * r + 10.0).astype(F)))
    # one-pixel spikes inside the mask: at the centre and at radius 19, the last masked pixel of the axis (radius 20 and 21
    # lie outside the mask, which makes the patch flat: stage_inputs.flat, group "outside")
    for name, (py, px) in (("centre", (HALF, HALF)), ("r19:x", (HALF, HALF + 19)), ("r19:y", (HALF - 19, HALF))):
        t = np.zeros((PS, PS), F); t[py, px] = 255
        items.append(("spike:" + name, t))
    rng = np.random.default_rng(20242)
    for k in range(2):
        items.append(("twolevel:%d" % k, np.where(rng.random((PS, PS)) < 0.5, F(2.0 ** 20), F(-2.0 ** 20)).astype(F)))
    return tuple(items)


def saturating():
    return np.stack([p for _, p in _saturating_items()])


def saturating_names():
    return [n for n, _ in _saturating_items()]


@functools.lru_cache(maxsize=None)
def ordinary():
    rng = np.random.default_rng(20243)
    yy, xx = np.mgrid[0:PS, 0:PS].astype(np.float64)
    out = np.empty((200, PS, PS), F)
    for k in range(200):
        a, b = rng.uniform(2.0, 7.0, 2)
        ph = rng.uniform(0.0, 2 * np.pi, 2)
        pat = np.sin(xx / a + ph[0]) * np.cos(yy / b + ph[1]) + 0.3 * rng.standard_normal((PS, PS))
        out[k] = (128.0 + rng.uniform(5.0, 80.0) * pat).astype(F)
    out.setflags(write=False)
    return out


THRESHOLD_VAR = F(1e-4)   # the largest float32 below the double 0.0001 that helpers.cpp:270 compares with: itself still flat


def is_flat_var(var):
    """helpers.cpp:270 `if (var < 0.0001)`: the float32 var against the double constant."""
    return float(var) < 0.0001


@functools.lru_cache(maxsize=None)
def _threshold_items():
    """Bisect the float32 scale c of c * pattern_0 (over its bit pattern) down to two neighbouring floats with the oracle's
    `var` on either side of 1e-4, then keep, of the 64 scales on each side, the two whose var is nearest the constant."""
    from tests import _oracle
    oh = _oracle.OracleHandle()
    pat = patterns()[0].astype(F)

    def at(bits):
        c = np.uint32(bits).view(F) if isinstance(bits, np.uint32) else np.array(bits, np.uint32).view(F)
        p = (c * pat).astype(F)
        return p, F(oh.sift_parts(p)[0][1])
    lo, hi = int(F(1e-6).view(np.uint32)), int(F(1e-2).view(np.uint32))
    assert is_flat_var(at(lo)[1]) and not is_flat_var(at(hi)[1])
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if is_flat_var(at(mid)[1]):
            lo = mid
        else:
            hi = mid
    tb = int(THRESHOLD_VAR.view(np.uint32))
    below, above = [], []
    for bits in range(lo - 63, hi + 64):
        p, var = at(bits)
        d = abs(int(var.view(np.uint32)) - tb)
        (below if is_flat_var(var) else above).append((d, bits, p, var))
    items = []
    for side, lst in (("below", below), ("above", above)):
        for d, bits, p, var in sorted(lst, key=lambda t: (t[0], t[1]))[:2]:
            items.append(("threshold:%s:%08x" % (side, bits), p, var))
    return tuple(items)


def threshold():
    return np.stack([p for _, p, _ in _threshold_items()])


def threshold_names():
    return [n for n, _, _ in _threshold_items()]


def threshold_vars():
    return np.array([v for _, _, v in _threshold_items()], F)


@functools.lru_cache(maxsize=None)
def interleaved(n):
    """The first n patches of a fixed interleaving of all families: flat scales and gaps, ordinary, constants / outside /
    threshold, saturating, and round again; each list is walked cyclically.  Neighbours always differ in family."""
    fl, names = flat(), flat_names()
    varying = np.array([i for i, nm in enumerate(names) if nm.startswith(("scale", "offset", "gap"))])
    still = np.array([i for i, nm in enumerate(names) if nm.startswith(("const", "outside"))])
    groups = (fl[varying], ordinary(), np.concatenate([fl[still], threshold()]), saturating())
    out = np.empty((n, PS, PS), F)
    for j in range(n):
        g = groups[j % 4]
        out[j] = g[(j // 4) % len(g)]
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# Window list for normalizeAffine (affine.cpp:102-144).  m = ceil(s * mrSize); the reference samples a window of
# P0 = 2 m + 1 pixels a side directly when P0 / 41 <= 0.4 and otherwise warps and smooths one of P = P0 + 2 = 2 m + 3.
# The kernels are cut by P: k_patch_extract_small<0> up to 41, <1> up to 63, k_patch_mid<128> 65..127, k_patch_mid<512>
# 129..511, k_patch_large_rows three-row form 513..1279, one-row form (second launch) from 1281.
# ---------------------------------------------------------------------------------------------------------------------------
WINDOW_IMAGE_SIDE = 1536
WINDOW_P_RANGES = ((19, 169), (495, 549), (1245, 1315))
WINDOW_DIRECT_P0 = (13, 15, 17)   # 13 and 15: P0 / 41 <= 0.4, direct; 17: the first smoothing window (P = 19)
WINDOW_SHAPE = (1.08, 0.0, 0.15, 1.0 / 1.08)   # rectified (a12 = 0), determinant 1, anisotropy 1.17 : 1, sheared


def window_side(s, mr_size=MR_SIZE):
    """(P0, P) as normalizeAffine computes them in float32."""
    m = int(np.ceil(F(s) * F(mr_size)))
    return 2 * m + 1, 2 * m + 3


def scale_for_p0(p0, mr_size=MR_SIZE):
    """The middle of the interval of s that gives this P0."""
    m = (p0 - 1) // 2
    s = F((m - 0.5) / float(mr_size))
    assert window_side(s, mr_size)[0] == p0 and window_side(np.nextafter(s, F(0)), mr_size)[0] == p0
    return s


@functools.lru_cache(maxsize=None)
def window_image():
    """One seeded 8-bit noise image: every window content differs in every pixel, nothing is smooth."""
    img = np.random.default_rng(20244).integers(0, 256, (WINDOW_IMAGE_SIDE, WINDOW_IMAGE_SIDE), dtype=np.uint8)
    img.setflags(write=False)
    return img


@functools.lru_cache(maxsize=None)
def windows():
    """-> kp [n][3] = x, y, s ; A [n][4] ; P0 [n] ; P [n] (P = P0 for the two direct windows).  Every P0 of
    WINDOW_DIRECT_P0 and every odd P of WINDOW_P_RANGES once with A = identity at a sub-pixel position, every fourth P of
    the ranges again with WINDOW_SHAPE."""
    rng = np.random.default_rng(20245)
    c = WINDOW_IMAGE_SIDE / 2.0
    kp, A, P0s, Ps = [], [], [], []

    def add(p0, shape):
        s = scale_for_p0(p0)
        kp.append((c + rng.uniform(-3.0, 3.0), c + rng.uniform(-3.0, 3.0), s)); A.append(shape)
        P0s.append(p0); Ps.append(p0 if p0 / 41.0 <= 0.4 else p0 + 2)
    for p0 in WINDOW_DIRECT_P0:
        add(p0, (1.0, 0.0, 0.0, 1.0))
    for lo, hi in WINDOW_P_RANGES:
        for j, P in enumerate(range(lo, hi + 1, 2)):
            if P - 2 in WINDOW_DIRECT_P0:
                continue   # P = 19 is already there
            add(P - 2, (1.0, 0.0, 0.0, 1.0))
        for j, P in enumerate(range(lo, hi + 1, 2)):
            if j % 4 == 0:
                add(P - 2, WINDOW_SHAPE)
    kp = np.array(kp, F); A = np.array(A, F)
    kp.setflags(write=False); A.setflags(write=False)
    return kp, A, np.array(P0s), np.array(Ps)
