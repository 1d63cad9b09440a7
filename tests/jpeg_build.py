"""Constructed inputs of the JPEG readers, made without an encoder: from arrays of quantised coefficients to the hesaff_jpeg_layout and
the coefficient blob the device stage takes (include/hesaff_amd.h), and to a baseline file that codes exactly those coefficients.
Test infrastructure for tests/test_jpeg_constructed_host.py (CPU) and tests/test_jpeg_constructed.py (GPU).

Coefficients travel as one int16 array [bh, bw, 8, 8] per component: blocks row by row, natural (row, column) order inside a block,
bw x bh as layout_for reports them (whole MCUs).  Quantisation tables are uint16 [8, 8] per component, natural order."""
import struct

import numpy as np

from hesaff_amd._binding import JpegLayout

BLOB_HEADER = 1024
ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])


def _ceil_div(a, b):
    return -(-a // b)


def layout_for(W, H, samp):
    """(h, v) per component -> the hesaff_jpeg_layout hesaff_read_jpeg_coefficients reports for such a file: bw / bh in whole MCUs,
    cw / chgt = ceil(size * factor / largest factor), hx / vx = largest factor / factor.  One component: a scan that is not
    interleaved, ceil(size / 8) blocks, factors (1, 1)."""
    samp = [tuple(s) for s in samp]
    assert len(samp) in (1, 3) and (len(samp) == 3 or samp == [(1, 1)]), samp
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    assert all(hmax % h == 0 and vmax % v == 0 for h, v in samp), samp
    mcux, mcuy = _ceil_div(W, 8 * hmax), _ceil_div(H, 8 * vmax)
    L = JpegLayout()
    L.width, L.height, L.channels = W, H, len(samp)
    for i, (h, v) in enumerate(samp):
        L.h[i], L.v[i], L.hx[i], L.vx[i] = h, v, hmax // h, vmax // v
        L.bw[i], L.bh[i] = mcux * h, mcuy * v
        L.cw[i], L.chgt[i] = _ceil_div(W * h, hmax), _ceil_div(H * v, vmax)
    return L


def layout_tuple(L):
    """every field of a layout, for comparing two"""
    return (L.width, L.height, L.channels) + tuple(tuple(getattr(L, n)) for n in ("h", "v", "hx", "vx", "bw", "bh", "cw", "chgt"))


def blocks_per_image(L):
    return sum(L.bw[i] * L.bh[i] for i in range(L.channels))


def blob_for(layout, coefs, quants, ycc):
    """-> the blob as a uint8 array: the components' tables (uint16, natural order) at byte 0, the int32 "YCbCr" flag at byte 384 (0
    for a grey image whatever `ycc` says, as the reader writes it), int16 coefficients from byte 1024, component after component"""
    return blobs_for(layout, [np.asarray(c)[None] for c in coefs], [np.asarray(q)[None] for q in quants], [ycc])[0]


def blobs_for(layout, coefs, quants, ycc):
    """the blobs of B images of one layout, uint8 [B, blob_bytes]: per component coefficients [B, bh, bw, 8, 8] and tables [B, 8, 8];
    ycc: one flag per image"""
    nc = layout.channels
    assert len(coefs) == nc and len(quants) == nc
    B = len(ycc)
    blobs = np.zeros((B, BLOB_HEADER + 128 * blocks_per_image(layout)), np.uint8)
    at = BLOB_HEADER
    for c in range(nc):
        cf, q = np.asarray(coefs[c]), np.asarray(quants[c])
        assert cf.shape == (B, layout.bh[c], layout.bw[c], 8, 8) and q.shape == (B, 8, 8), (cf.shape, q.shape, layout.bh[c], layout.bw[c])
        assert cf.min() >= -32768 and cf.max() <= 32767 and q.min() >= 0 and q.max() <= 65535
        blobs[:, 128 * c:128 * c + 128] = np.ascontiguousarray(q.astype("<u2")).reshape(B, 64).view(np.uint8)
        raw = np.ascontiguousarray(cf.astype("<i2")).reshape(B, -1).view(np.uint8)
        blobs[:, at:at + raw.shape[1]] = raw
        at += raw.shape[1]
    flags = np.array([1 if (f and nc == 3) else 0 for f in ycc], "<i4")
    blobs[:, 384:388] = flags.view(np.uint8).reshape(B, 4)
    return blobs


class _Bits:
    """the entropy-coded segment: bits most significant first, a zero byte stuffed behind every 0xFF, the last byte padded with ones"""
    def __init__(self):
        self.out = bytearray()
        self.acc = 0
        self.n = 0

    def put(self, value, nbits):
        self.acc = (self.acc << nbits) | (value & ((1 << nbits) - 1))
        self.n += nbits
        while self.n >= 8:
            self.n -= 8
            b = (self.acc >> self.n) & 0xFF
            self.out.append(b)
            if b == 0xFF:
                self.out.append(0)
        self.acc &= (1 << self.n) - 1

    def align(self):
        if self.n:
            self.put((1 << (8 - self.n)) - 1, 8 - self.n)


# one DC and one AC table in which every symbol has an 8-bit code: the k-th symbol of the list has the code k
DC_SYMBOLS = list(range(12))                                                                   # bit counts 0 .. 11
AC_SYMBOLS = [0x00, 0xF0] + [(run << 4) | size for run in range(16) for size in range(1, 11)]   # EOB, ZRL, (run, size 1 .. 10)
_DC_CODE = {s: k for k, s in enumerate(DC_SYMBOLS)}
_AC_CODE = {s: k for k, s in enumerate(AC_SYMBOLS)}


def _value_bits(v, size):
    return v if v >= 0 else v + (1 << size) - 1


def _code_block(bits, blk, pred):
    """one block (int, 64 values in natural order) behind the DC prediction `pred` -> the new prediction"""
    zz = [int(x) for x in blk.reshape(64)[ZIGZAG]]
    diff = zz[0] - pred
    size = abs(diff).bit_length()
    assert size <= 11, "a DC difference of baseline coding has at most 11 bits: %d" % diff
    bits.put(_DC_CODE[size], 8)
    if size:
        bits.put(_value_bits(diff, size), size)
    run = 0
    last = max([k for k in range(1, 64) if zz[k]], default=0)
    for k in range(1, last + 1):
        v = zz[k]
        if v == 0:
            run += 1
            continue
        while run > 15:
            bits.put(_AC_CODE[0xF0], 8)
            run -= 16
        size = abs(v).bit_length()
        assert size <= 10, "an AC value of baseline coding has at most 10 bits: %d" % v
        bits.put(_AC_CODE[(run << 4) | size], 8)
        bits.put(_value_bits(v, size), size)
        run = 0
    if last < 63:
        bits.put(_AC_CODE[0x00], 8)
    return zz[0]


def _segment(marker, payload):
    return bytes([0xFF, marker]) + struct.pack(">H", len(payload) + 2) + bytes(payload)


def write_jpeg(W, H, samp, coefs, quants, adobe=None, q16=False, restart=0, interleaved=True):
    """-> the bytes of a sequential Huffman file (SOF0; SOF1 with 16-bit tables) that codes exactly `coefs`: one scan, interleaved
    unless there is one component; component i uses quantisation table i; `adobe`: the transform byte of an APP14 "Adobe" segment
    (None: no such segment, so three components are YCbCr); `restart`: MCUs per restart interval (0: none).  interleaved=False: one
    scan per component over its ceil(cw / 8) x ceil(chgt / 8) blocks (A.2.3) - blocks of `coefs` beyond those are not coded."""
    L = layout_for(W, H, samp)
    nc = L.channels
    out = bytearray(b"\xff\xd8")
    if adobe is not None:
        out += _segment(0xEE, b"Adobe" + struct.pack(">HHHB", 100, 0, 0, adobe))
    for c in range(nc):
        q = np.asarray(quants[c]).reshape(64)[ZIGZAG].astype(np.int64)
        assert q.min() >= 1 and q.max() <= (65535 if q16 else 255)
        out += _segment(0xDB, bytes([(16 if q16 else 0) | c]) + (q.astype(">u2").tobytes() if q16 else q.astype(np.uint8).tobytes()))
    sof = struct.pack(">BHHB", 8, H, W, nc)
    for c in range(nc):
        sof += bytes([c + 1, (L.h[c] << 4) | L.v[c], c])
    out += _segment(0xC1 if q16 else 0xC0, sof)
    for cls, symbols in ((0, DC_SYMBOLS), (1, AC_SYMBOLS)):
        counts = [0] * 16
        counts[7] = len(symbols)
        out += _segment(0xC4, bytes([cls << 4]) + bytes(counts) + bytes(symbols))
    if restart:
        out += _segment(0xDD, struct.pack(">H", restart))
    cf = [np.asarray(coefs[c]).astype(np.int64) for c in range(nc)]
    for c in range(nc):
        assert cf[c].shape == (L.bh[c], L.bw[c], 8, 8), (cf[c].shape, L.bh[c], L.bw[c])
    hmax, vmax = max(L.h[:nc]), max(L.v[:nc])
    scans = [list(range(nc))] if interleaved else [[c] for c in range(nc)]
    for scan in scans:
        sos = bytes([len(scan)])
        for c in scan:
            sos += bytes([c + 1, 0x00])
        out += _segment(0xDA, sos + bytes([0, 63, 0]))
        if len(scan) == 1:
            mx, my = _ceil_div(L.cw[scan[0]], 8), _ceil_div(L.chgt[scan[0]], 8)
        else:
            mx, my = _ceil_div(W, 8 * hmax), _ceil_div(H, 8 * vmax)
        bits = _Bits()
        pred = [0] * nc
        for mcu in range(mx * my):
            if restart and mcu and mcu % restart == 0:
                bits.align()
                bits.out += bytes([0xFF, 0xD0 + (mcu // restart - 1) % 8])
                pred = [0] * nc
            mr, mc = divmod(mcu, mx)
            for c in scan:
                h, v = (1, 1) if len(scan) == 1 else (L.h[c], L.v[c])
                for by in range(v):
                    for bx in range(h):
                        pred[c] = _code_block(bits, cf[c][mr * v + by, mc * h + bx], pred[c])
        bits.align()
        out += bits.out
    out += b"\xff\xd9"
    return bytes(out)


# ---- the sampling layouts of the constructed tests: (h, v) per component ----
def _luma_full(hx, vx):
    return [(hx, vx), (1, 1), (1, 1)]


SAMPLINGS = {"grey": [(1, 1)]}
SAMPLINGS.update({"chroma_%dx%d" % (hx, vx): _luma_full(hx, vx) for hx in (1, 2, 3, 4) for vx in (1, 2, 3, 4)})   # chroma ratio hx x vx
SAMPLINGS.update({
    "luma_2x1": [(1, 1), (2, 1), (2, 1)], "luma_2x2": [(1, 1), (2, 2), (2, 2)],              # a sub-sampled luma
    "three_ratios_a": [(2, 2), (2, 1), (1, 2)], "three_ratios_b": [(4, 1), (2, 1), (1, 1)],   # three different ratios
    "third_only": [(2, 2), (2, 2), (1, 1)],                                                   # only the third component sub-sampled
    "luma_1x2_mixed": [(2, 1), (1, 2), (1, 1)],                                               # the vertical triangle on the luma
})


def mcu_blocks(samp):
    """blocks of an interleaved MCU; a scan may hold at most 10 (B.2.3)"""
    return sum(h * v for h, v in samp) if len(samp) > 1 else 1


FILE_SAMPLINGS = {k: v for k, v in SAMPLINGS.items() if mcu_blocks(v) <= 10}     # what a file with one interleaved scan can have
OVERSIZED_SAMPLINGS = {k: v for k, v in SAMPLINGS.items() if mcu_blocks(v) > 10}  # luma 3x3, 3x4, 4x3, 4x4: refused by the readers


# ---- coefficient families ----
def dc_ramps(layout, B, rng, first=0, dc_lo=-60, dc_hi=60):
    """per component DC values [B, bh, bw] such that neighbouring blocks, components and images differ: a ramp over an image's
    blocks from a start that depends on the image (numbered from `first`), inside [dc_lo, dc_hi]"""
    span = dc_hi - dc_lo + 1
    out, k = [], 7 * (first + np.arange(B)) + rng.integers(0, span, B)
    for c in range(layout.channels):
        n = layout.bw[c] * layout.bh[c]
        out.append(((k[:, None] + 5 * np.arange(n)[None]) % span + dc_lo).reshape(B, layout.bh[c], layout.bw[c]))
        k = k + 5 * n + 11
    return out


def legal_batch(layout, B, rng, first=0, ac=10, density=0.3):
    """the legal family for B images: DC within +-60 on a ramp that differs from image to image, AC within +-ac at the given density,
    and per image its own tables with quantisers 1 .. 8 - the transform stays far inside 32 bits and (nearly) inside 0 .. 255.
    -> (coefficients per component [B, bh, bw, 8, 8] int16, tables per component [B, 8, 8] uint16)"""
    coefs = []
    for c, dc in enumerate(dc_ramps(layout, B, rng, first)):
        shape = (B, layout.bh[c], layout.bw[c], 8, 8)
        cf = np.where(rng.random(shape) < density, rng.integers(-ac, ac + 1, shape), 0)
        cf[..., 0, 0] = dc
        coefs.append(cf.astype(np.int16))
    return coefs, [rng.integers(1, 9, (B, 8, 8)).astype(np.uint16) for _ in range(layout.channels)]


def legal_coefs(layout, image, rng):
    """one image of the legal family (numbered `image`) -> coefficients per component [bh, bw, 8, 8]"""
    return [c[0] for c in legal_batch(layout, 1, rng, first=image)[0]]


def legal_quants(layout, rng):
    return [rng.integers(1, 9, (8, 8)).astype(np.uint16) for _ in range(layout.channels)]


def flat_coefs(layout, values):
    """DC-only blocks: with quantiser 1 a DC of 8 k gives a flat block of value 128 + k.  values: per component the sample value
    0 .. 255 of its blocks, one number or an array [bh, bw]"""
    out = []
    for c in range(layout.channels):
        cf = np.zeros((layout.bh[c], layout.bw[c], 8, 8), np.int16)
        cf[..., 0, 0] = 8 * (np.asarray(values[c], np.int64) - 128)
        out.append(cf)
    return out


def chunk_set(n=70, seed=5, amp=40):
    """n 4:2:0 images of 40 x 40 (54 blocks each) for the file pipeline: the legal family at a lower density, with strong low
    frequencies in the luma - structures of a block's size, in which the detector finds keys
    -> (layout, sampling, coefficients per component [n, bh, bw, 8, 8], tables per component [n, 8, 8])"""
    rng = np.random.default_rng(seed)
    samp = SAMPLINGS["chroma_2x2"]
    L = layout_for(40, 40, samp)
    coefs, quants = legal_batch(L, n, rng, ac=6, density=0.15)
    lo = rng.integers(-amp, amp + 1, coefs[0].shape[:3] + (3, 3))
    lo[..., 0, 0] = coefs[0][..., 0, 0]
    coefs[0][..., :3, :3] = lo
    return L, samp, coefs, quants


def chunk_files(n=70):
    """the files of chunk_set, as bytes"""
    L, samp, coefs, quants = chunk_set(n)
    return [write_jpeg(40, 40, samp, [c[i] for c in coefs], [q[i] for q in quants]) for i in range(n)]
