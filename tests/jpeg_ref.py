"""A plain numpy statement of the device half of the JPEG reader (hesaff_amd/csrc/kernels_jpeg.h: k_jpeg_idct, k_jpeg_pixels), from
(hesaff_jpeg_layout, coefficient blob) to pixels [H][W][channels].  Test infrastructure: tests/test_jpeg_constructed_host.py pins it
to hesaff_read_jpeg (and, where Pillow imports, to libjpeg-turbo) on the CPU; tests/test_jpeg_constructed.py then holds the kernels to it.

Three parts, each written in another shape than the kernel's so that two statements of one definition are compared:
  * jidctint.c's islow transform on whole arrays of blocks, every add, subtract and multiply reduced modulo 2^32 (two's complement) -
    the project's definition for coefficients whose transform leaves 32 bits (jpeg_decode.cpp, W32) - and libjpeg's 10-bit
    range-limit window; `_idct_islow_numpy` is the same transform in plain int64, equal to it wherever nothing wraps;
  * jdsample.c's choice of up-sampling method and its five methods, row-wise over whole planes (the kernel works per output pixel);
  * jdcolor.c's table-driven YCbCr -> RGB conversion (the kernel evaluates the products per pixel), or the plain copy for Adobe RGB."""
import numpy as np

BLOB_HEADER = 1024   # HESAFF_JPEG_BLOB_HEADER

_F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
          f2562=20995, f3072=25172)


def _w32(x):
    """int64 -> the int64 value of its low 32 bits read as two's complement"""
    return ((x + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)


def _pass_wrapping(d, shift):
    """one 1-D pass of jpeg_idct_islow along the last axis; every operation reduced to 32 bits (operands are then below 2^31 in
    magnitude and the constants below 2^15, so int64 holds every product exactly before it is reduced)"""
    w = _w32
    F = _F
    z2, z3 = d[..., 2], d[..., 6]
    z1 = w(w(z2 + z3) * F["f0541"])
    tmp2 = w(z1 + w(z3 * -F["f1847"]))
    tmp3 = w(z1 + w(z2 * F["f0765"]))
    tmp0 = w(w(d[..., 0] + d[..., 4]) * (1 << 13))
    tmp1 = w(w(d[..., 0] - d[..., 4]) * (1 << 13))
    tmp10, tmp13, tmp11, tmp12 = w(tmp0 + tmp3), w(tmp0 - tmp3), w(tmp1 + tmp2), w(tmp1 - tmp2)
    t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
    z1, z2, z3, z4 = w(t0 + t3), w(t1 + t2), w(t0 + t2), w(t1 + t3)
    z5 = w(w(z3 + z4) * F["f1175"])
    t0, t1, t2, t3 = w(t0 * F["f0298"]), w(t1 * F["f2053"]), w(t2 * F["f3072"]), w(t3 * F["f1501"])
    z1, z2 = w(z1 * -F["f0899"]), w(z2 * -F["f2562"])
    z3, z4 = w(w(z3 * -F["f1961"]) + z5), w(w(z4 * -F["f0390"]) + z5)
    t0, t1, t2, t3 = w(w(t0 + z1) + z3), w(w(t1 + z2) + z4), w(w(t2 + z2) + z3), w(w(t3 + z1) + z4)
    out = np.stack([w(tmp10 + t3), w(tmp11 + t2), w(tmp12 + t1), w(tmp13 + t0), w(tmp13 - t0), w(tmp12 - t1), w(tmp11 - t2), w(tmp10 - t3)], -1)
    return w(out + (1 << (shift - 1))) >> shift   # descale: the rounding add wraps too, the shift is arithmetic


def range_limit(x):
    """libjpeg's range_limit[x & RANGE_MASK] behind the level shift: the low 10 bits, read as signed, plus 128, clamped to 0..255"""
    v = x & 1023
    v = np.where(v >= 512, v - 1024, v) + 128
    return np.clip(v, 0, 255).astype(np.uint8)


def idct_islow_wrapping(coef, quant):
    """blocks [n, 8, 8] int16, quantisation table(s) [8, 8] or [n, 8, 8] uint16 -> (samples uint8 [n, 8, 8], the values before the
    range limit int64 [n, 8, 8])"""
    q = np.asarray(quant).astype(np.int64)
    d = _w32(np.asarray(coef).astype(np.int64) * (q if q.ndim == 3 else q[None]))
    ws = np.swapaxes(_pass_wrapping(np.swapaxes(d, 1, 2), 13 - 2), 1, 2)   # columns
    pre = _pass_wrapping(ws, 13 + 2 + 3)                                   # rows
    return range_limit(pre), pre


def _idct_islow_numpy(coef, quant):
    """jidctint.c (JDCT_ISLOW) on an array of blocks [n, 8, 8] int16 with one quantisation table [8, 8]: int64 arithmetic (a legal
    stream never leaves 32 bits), the same constants, shifts and range limit as idct_islow / k_jpeg_idct -> uint8 [n, 8, 8]."""
    F = dict(f0298=2446, f0390=3196, f0541=4433, f0765=6270, f0899=7373, f1175=9633, f1501=12299, f1847=15137, f1961=16069, f2053=16819,
             f2562=20995, f3072=25172)

    def pass1d(d, shift):   # d: [..., 8] along the transformed axis (last)
        z2, z3 = d[..., 2], d[..., 6]
        z1 = (z2 + z3) * F["f0541"]
        tmp2 = z1 + z3 * -F["f1847"]
        tmp3 = z1 + z2 * F["f0765"]
        tmp0 = (d[..., 0] + d[..., 4]) << 13
        tmp1 = (d[..., 0] - d[..., 4]) << 13
        tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
        t0, t1, t2, t3 = d[..., 7], d[..., 5], d[..., 3], d[..., 1]
        z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
        z5 = (z3 + z4) * F["f1175"]
        t0, t1, t2, t3 = t0 * F["f0298"], t1 * F["f2053"], t2 * F["f3072"], t3 * F["f1501"]
        z1, z2, z3, z4 = z1 * -F["f0899"], z2 * -F["f2562"], z3 * -F["f1961"] + z5, z4 * -F["f0390"] + z5
        t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
        out = np.stack([tmp10 + t3, tmp11 + t2, tmp12 + t1, tmp13 + t0, tmp13 - t0, tmp12 - t1, tmp11 - t2, tmp10 - t3], -1)
        return (out + (1 << (shift - 1))) >> shift
    d = coef.astype(np.int64) * quant.astype(np.int64)[None]
    ws = pass1d(np.swapaxes(d, 1, 2), 13 - 2)          # columns: transform along the row index
    ws = np.swapaxes(ws, 1, 2)
    o = pass1d(ws, 13 + 2 + 3)                          # rows
    v = o & 1023
    v = np.where(v >= 512, v - 1024, v) + 128
    return np.clip(v, 0, 255).astype(np.uint8)


def idct_islow_nonwrapping(coef, quant):
    """the non-wrapping variant in idct_islow_wrapping's form: table(s) [8, 8] or [n, 8, 8] -> (samples, None)"""
    q = np.asarray(quant)
    if q.ndim == 2:
        return _idct_islow_numpy(np.asarray(coef), q), None
    return np.stack([_idct_islow_numpy(np.asarray(coef)[i:i + 1], q[i])[0] for i in range(len(q))]), None


# ---- blob -> component planes ----
def split_blobs(layout, blobs):
    """blobs uint8 [B, blob_bytes] (or one blob) -> (per component: coefficients int16 [B, bh, bw, 8, 8] and tables uint16 [B, 8, 8],
    the B "YCbCr" flags)"""
    blobs = np.ascontiguousarray(blobs, np.uint8)
    if blobs.ndim == 1:
        blobs = blobs[None]
    B = blobs.shape[0]
    nc = layout.channels
    blocks = sum(layout.bw[c] * layout.bh[c] for c in range(nc))
    assert blobs.shape[1] == BLOB_HEADER + 128 * blocks, (blobs.shape, blocks)
    comps, at = [], BLOB_HEADER
    for c in range(nc):
        bw, bh = layout.bw[c], layout.bh[c]
        coef = blobs[:, at:at + bw * bh * 128].copy().view(np.int16).reshape(B, bh, bw, 8, 8)
        quant = blobs[:, 128 * c:128 * c + 128].copy().view(np.uint16).reshape(B, 8, 8)
        comps.append((coef, quant))
        at += bw * bh * 128
    ycc = blobs[:, 384:388].copy().view(np.int32)[:, 0]
    return comps, ycc


def component_planes(layout, blobs, idct=idct_islow_wrapping):
    """-> (planes: per component uint8 [B, bh * 8, bw * 8]; pre: the same shape before the range limit, or None; the flags)"""
    comps, ycc = split_blobs(layout, blobs)
    planes, pres = [], []
    for coef, quant in comps:
        B, bh, bw = coef.shape[:3]
        s, pre = idct(coef.reshape(B * bh * bw, 8, 8), np.repeat(quant, bh * bw, axis=0))

        def lay(a):
            return a.reshape(B, bh, bw, 8, 8).transpose(0, 1, 3, 2, 4).reshape(B, bh * 8, bw * 8)
        planes.append(lay(s))
        pres.append(None if pre is None else lay(pre))
    return planes, pres, ycc


# ---- jdsample.c ----
def upsample_method(hx, vx, cw):
    """jinit_upsampler's choice at do_fancy_upsampling = TRUE for a component that needs hx x vx expansion and is cw samples wide"""
    if hx == 1 and vx == 1:
        return "fullsize"
    if hx == 2 and vx == 1:
        return "h2v1_fancy" if cw > 2 else "replicate"      # the triangle filter needs three columns
    if hx == 2 and vx == 2:
        return "h2v2_fancy" if cw > 2 else "replicate"
    if hx == 1 and vx == 2:
        return "h1v2_fancy"                                  # libjpeg-turbo; no width condition
    return "replicate"                                       # int_upsample, any integral ratio


def _interleave(a, b, axis):
    """a0 b0 a1 b1 ... along axis"""
    out = np.stack([a, b], axis=axis + 1 if axis >= 0 else axis)
    shape = list(a.shape)
    shape[axis] *= 2
    return out.reshape(shape)


def _h2v1_rows(s):
    """h2v1_fancy_upsample on rows s [..., w] (int64): even outputs lean on the left neighbour with bias 1, odd ones on the right
    with bias 2; the first and the last output column are the edge samples themselves"""
    even = s.copy()
    even[..., 1:] = (3 * s[..., 1:] + s[..., :-1] + 1) >> 2
    odd = s.copy()
    odd[..., :-1] = (3 * s[..., :-1] + s[..., 1:] + 2) >> 2
    return _interleave(even, odd, s.ndim - 1)


def _near_far_rows(s):
    """for every output row of a 2x vertical expansion of s [..., h, w]: the nearer input row and the farther one (the row above for
    an upper output row, below for a lower one; the image's first and last row stand in for the missing neighbours)"""
    up = np.concatenate([s[..., :1, :], s[..., :-1, :]], axis=-2)
    down = np.concatenate([s[..., 1:, :], s[..., -1:, :]], axis=-2)
    return _interleave(s, s, s.ndim - 2), _interleave(up, down, s.ndim - 2)


def _h2v2_rows(s):
    """h2v2_fancy_upsample: column sums 3 * near + far per output row, then the horizontal triangle with biases 8 (even) and 7 (odd)"""
    near, far = _near_far_rows(s)
    c = 3 * near + far
    even = (c * 4 + 8) >> 4
    even[..., 1:] = (3 * c[..., 1:] + c[..., :-1] + 8) >> 4
    odd = (c * 4 + 7) >> 4
    odd[..., :-1] = (3 * c[..., :-1] + c[..., 1:] + 7) >> 4
    return _interleave(even, odd, s.ndim - 1)


def _h1v2_rows(s):
    """h1v2_fancy_upsample: vertical triangle, bias 1 for the upper and 2 for the lower output row"""
    near, far = _near_far_rows(s)
    bias = np.tile(np.array([1, 2], np.int64), s.shape[-2])[:, None]
    return (3 * near + far + bias) >> 2


def upsample(plane, cw, chgt, hx, vx, W, H):
    """a component's plane [..., bh * 8, bw * 8] -> its samples at full resolution [..., H, W]"""
    s = plane[..., :chgt, :cw].astype(np.int64)   # the samples the component has; the rest of the plane is block padding
    m = upsample_method(hx, vx, cw)
    if m == "fullsize":
        full = s
    elif m == "h2v1_fancy":
        full = _h2v1_rows(s)
    elif m == "h2v2_fancy":
        full = _h2v2_rows(s)
    elif m == "h1v2_fancy":
        full = _h1v2_rows(s)
    else:
        full = np.repeat(np.repeat(s, vx, axis=-2), hx, axis=-1)
    assert full.shape[-2] >= H and full.shape[-1] >= W, (full.shape, W, H)
    return full[..., :H, :W]


# ---- jdcolor.c ----
def _ycc_tables():
    """build_ycc_rgb_table, SCALEBITS 16"""
    def fix(x):
        return int(x * (1 << 16) + 0.5)
    x = np.arange(256, dtype=np.int64) - 128
    half = 1 << 15
    return (fix(1.40200) * x + half) >> 16, (fix(1.77200) * x + half) >> 16, -fix(0.71414) * x, -fix(0.34414) * x + half


def ycc_to_rgb(y, cb, cr):
    """ycc_rgb_convert on planes of samples 0..255 (any integer type) -> uint8 [..., 3]"""
    cr_r, cb_b, cr_g, cb_g = _ycc_tables()
    y = y.astype(np.int64)
    r = y + cr_r[cr]
    g = y + ((cb_g[cb] + cr_g[cr]) >> 16)
    b = y + cb_b[cb]
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


# ---- the whole stage ----
def pixels(layout, blobs, idct=idct_islow_wrapping):
    """blobs [B, blob_bytes] of one layout -> pixels uint8 [B, H, W] (one channel) or [B, H, W, 3]"""
    planes, _, ycc = component_planes(layout, blobs, idct)
    W, H = layout.width, layout.height
    if layout.channels == 1:
        return np.ascontiguousarray(planes[0][:, :H, :W])
    full = [upsample(planes[c], layout.cw[c], layout.chgt[c], layout.hx[c], layout.vx[c], W, H) for c in range(3)]
    converted = ycc_to_rgb(*full)
    copied = np.stack(full, -1).astype(np.uint8)
    return np.where((ycc != 0)[:, None, None, None], converted, copied)
