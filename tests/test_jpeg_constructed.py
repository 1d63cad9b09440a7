"""The device half of the JPEG reader (hesaff_amd/csrc/kernels_jpeg.h: k_jpeg_idct, k_jpeg_pixels) on constructed coefficients, at the
edges of its domain that no encoder-made file reaches: several images inside one wavefront, transforms that leave 32 bits or the
10-bit range-limit window, every sampling ratio at the widths where the up-sampling method changes, the Adobe RGB copy, the colour
conversion at its clamps.  Every comparison is np.array_equal between ctx.jpeg_pixels(layout, blobs) and the plain numpy statement of
the stage (tests/jpeg_ref.py), which tests/test_jpeg_constructed_host.py pins to hesaff_read_jpeg and libjpeg-turbo on the CPU.

Every block of every image carries other coefficients (a DC ramp per image plus seeded AC values) and every image of a batch its own
quantisation tables, so a block written to the wrong place, read from the wrong image or dequantised with a neighbour's table shows.
The layouts that make_jpeg_geom refuses are checked on the CPU (tests/native/jpeg_plan_check.cpp), not here."""
import numpy as np
import pytest

import hesaff_amd
from tests import jpeg_build as JB
from tests import jpeg_ref as JR

pytestmark = pytest.mark.gpu


def _legal_blobs(L, B, rng, ycc=1):
    coefs, quants = JB.legal_batch(L, B, rng)
    return JB.blobs_for(L, coefs, quants, [ycc] * B if np.isscalar(ycc) else ycc)


# ---- block addressing in k_jpeg_idct ----
ADDRESSING = [
    # id, sampling, W, H, blocks per image, batch sizes
    ("1_block_grey_8x8", "grey", 8, 8, 1, (1, 63, 64, 65, 257, 600)),
    ("1_block_grey_1x1", "grey", 1, 1, 1, (1, 63, 64, 65, 257, 600)),
    ("1_block_grey_5x3", "grey", 5, 3, 1, (1, 63, 64, 65, 257, 600)),
    ("3_blocks_444_8x8", "chroma_1x1", 8, 8, 3, (21, 22, 86, 171)),
    ("6_blocks_420_16x16", "chroma_2x2", 16, 16, 6, (11, 43)),
    ("54_blocks_420_40x40", "chroma_2x2", 40, 40, 54, (5, 19)),
    ("63_blocks_grey_56x72", "grey", 56, 72, 63, (5,)),
    ("64_blocks_grey_64x64", "grey", 64, 64, 64, (5,)),
    ("65_blocks_grey_40x104", "grey", 40, 104, 65, (5,)),
]


@pytest.mark.parametrize("case", ADDRESSING, ids=[c[0] for c in ADDRESSING])
def test_blocks_of_many_images_in_one_wavefront(ctx, case):
    """A wavefront of k_jpeg_idct takes 64 consecutive blocks of the chunk and walks image borders from its first block's image: 63
    steps with one block per image, none inside a large image, one or two with 54 to 65 blocks; totals on and next to multiples of
    64 (a wavefront) and 256 (a thread block); with three or six blocks per image a component border and an image border inside one
    wavefront; per image its own tables.  One call per batch size against the reference, and the smallest batch again one image
    per call.  (The grid-stride loop of k_jpeg_idct repeats only beyond 2^28 blocks - a chunk of 32 GB of coefficients - and is
    not tested.)"""
    _, name, W, H, blocks, sizes = case
    L = JB.layout_for(W, H, JB.SAMPLINGS[name])
    assert JB.blocks_per_image(L) == blocks
    rng = np.random.default_rng(1000 + blocks + W)
    blobs = _legal_blobs(L, max(sizes), rng)
    assert blobs.nbytes < (1 << 20)
    assert len({b[JR.BLOB_HEADER:].tobytes() for b in blobs}) == len(blobs) and len({b[:384].tobytes() for b in blobs}) == len(blobs)
    want = JR.pixels(L, blobs)
    for B in sizes:
        got = ctx.jpeg_pixels(L, blobs[:B])
        bad = [i for i in range(B) if not np.array_equal(got[i], want[i])]
        assert not bad, (case[0], B, "images that differ", bad[:20])
    B = {1: 65, 3: 22, 6: 11}.get(blocks, 5)
    single = np.stack([ctx.jpeg_pixels(L, blobs[i])[0] for i in range(B)])
    assert np.array_equal(single, want[:B])


# ---- transform arithmetic ----
def _grey_blobs(coef, quant):
    """coef [B, 8, 8, 8, 8] and quant [B, 8, 8] of 64 x 64 grey images -> (layout, blobs)"""
    L = JB.layout_for(64, 64, JB.SAMPLINGS["grey"])
    return L, JB.blobs_for(L, [coef], [quant], [0] * len(coef))


def test_transform_of_single_coefficients(ctx):
    """one non-zero coefficient per block, at each of the 64 positions (block k of an image holds position k), with the values +-1,
    +-1023, +-32767 and -32768 under the quantisers 1, 255 and 65535: every product of a dequantised value with every constant of
    both passes, from far inside 32 bits to far outside"""
    values, quantisers = (1, -1, 1023, -1023, 32767, -32767, -32768), (1, 255, 65535)
    coef = np.zeros((len(values) * len(quantisers), 64, 64), np.int64)
    quant = np.zeros((len(coef), 8, 8), np.int64)
    for i, v in enumerate(values):
        for j, q in enumerate(quantisers):
            coef[i * len(quantisers) + j, np.arange(64), np.arange(64)] = v
            quant[i * len(quantisers) + j] = q
    L, blobs = _grey_blobs(coef.reshape(-1, 8, 8, 8, 8), quant)
    want = JR.pixels(L, blobs)
    assert len(np.unique(want)) > 100   # the family reaches most sample values
    got = ctx.jpeg_pixels(L, blobs)
    bad = [(values[i // 3], quantisers[i % 3]) for i in range(len(coef)) if not np.array_equal(got[i], want[i])]
    assert not bad, bad


def test_transform_of_legal_coefficients(ctx):
    """DC within +-60, AC within +-10 at density 0.3, quantisers 1 .. 8: what a photograph holds; next to no sample is clamped"""
    rng = np.random.default_rng(11)
    L = JB.layout_for(64, 64, JB.SAMPLINGS["grey"])
    blobs = _legal_blobs(L, 5, rng, ycc=0)
    want = JR.pixels(L, blobs)
    assert float(((want == 0) | (want == 255)).mean()) <= 0.01
    assert np.array_equal(JR.pixels(L, blobs, idct=JR.idct_islow_nonwrapping), want)
    assert np.array_equal(ctx.jpeg_pixels(L, blobs), want)


def test_range_limit_window(ctx):
    """Results on every side of libjpeg's range limit: inside [-128, 127] (a sample as it is), [-512, -129] and [128, 511] (clamped to
    0 and 255), and |x| >= 512, where the 10-bit window wraps and a plain clamp of x + 128 would be wrong.  DC values within +-1500
    under a quantiser of 8 spread the blocks' levels over +-1500; the reference's values before the limit say where each sample fell."""
    rng = np.random.default_rng(12)
    B = 5
    coef = np.where(rng.random((B, 8, 8, 8, 8)) < 0.3, rng.integers(-10, 11, (B, 8, 8, 8, 8)), 0)
    coef[..., 0, 0] = rng.integers(-1500, 1501, (B, 8, 8))
    L, blobs = _grey_blobs(coef, np.full((B, 8, 8), 8))
    planes, pre, _ = JR.component_planes(L, blobs)
    x = pre[0]
    zones = [(x >= -128) & (x <= 127), (x >= -512) & (x <= -129), (x >= 128) & (x <= 511), np.abs(x) >= 512]
    assert all(float(z.mean()) >= 0.01 for z in zones), [float(z.mean()) for z in zones]
    want = JR.pixels(L, blobs)
    clamped = np.clip(x + 128, 0, 255).astype(np.uint8)
    assert float((clamped != planes[0]).mean()) >= 0.01   # the window is not a clamp on this input
    assert np.array_equal(JR.pixels(L, blobs, idct=JR.idct_islow_nonwrapping), want)   # ... and nothing here leaves 32 bits
    assert np.array_equal(ctx.jpeg_pixels(L, blobs), want)


def test_transform_wraps_at_32_bits(ctx):
    """full int16 coefficients under 16-bit quantisers: sums and products leave 32 bits in both passes, and the device wraps like the
    host reader's W32 (tests/test_jpeg_constructed_host.py pins that through a file); the int64 statement differs on a quarter of
    the samples at least, so wrapping is what is compared"""
    rng = np.random.default_rng(13)
    B = 5
    L, blobs = _grey_blobs(rng.integers(-32768, 32768, (B, 8, 8, 8, 8)), rng.integers(1, 65536, (B, 8, 8)))
    want = JR.pixels(L, blobs)
    assert float((JR.pixels(L, blobs, idct=JR.idct_islow_nonwrapping) != want).mean()) >= 0.25
    assert np.array_equal(ctx.jpeg_pixels(L, blobs), want)


# ---- up-sampling, pixel packing and colour ----
WIDTHS = (1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13)
HEIGHTS = (1, 2, 3, 5, 8, 9, 17)
SIZES = [(W, H) for W in WIDTHS for H in HEIGHTS]
COLOUR = sorted(k for k in JB.SAMPLINGS if k != "grey")


def _mixed_batch(L, rng):
    """three images of one layout: the legal family as YCbCr and as Adobe RGB, and flat blocks of random sample values (quantiser 1)
    as YCbCr - every block of a component another level from all of 0 .. 255"""
    coefs, quants = JB.legal_batch(L, 3, rng)
    flat = JB.flat_coefs(L, [rng.integers(0, 256, (L.bh[c], L.bw[c])) for c in range(L.channels)])
    for c in range(L.channels):
        coefs[c][2] = flat[c]
        quants[c][2] = 1
    return JB.blobs_for(L, coefs, quants, [1, 0, 1])


@pytest.mark.parametrize("name", COLOUR)
def test_upsampling_at_every_ratio_and_width(ctx, name):
    """Chroma ratios 1 .. 4 in both directions under a full-resolution luma, a sub-sampled luma, three different ratios in one image,
    only the third component sub-sampled: jdsample.c's five methods, chosen per component from the ratio and from cw > 2.  Widths 1 ..
    9, 12 and 13 take cw across 2 | 3 for a ratio of 2 and reach both the packed-word and the byte path of k_jpeg_pixels; three
    images per call put the image stride off a multiple of 4 wherever 3 W H is.  Odd sizes leave the last chroma row and column
    beside decoded block padding that is unlike the edge: a read past cw or chgt changes a pixel."""
    samp = JB.SAMPLINGS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    methods = set()
    for (W, H) in SIZES:
        L = JB.layout_for(W, H, samp)
        methods |= {JR.upsample_method(L.hx[c], L.vx[c], L.cw[c]) for c in range(3)}
        blobs = _mixed_batch(L, rng)
        want = JR.pixels(L, blobs)
        got = ctx.jpeg_pixels(L, blobs)
        assert np.array_equal(got, want), (name, W, H, [bool(np.array_equal(got[i], want[i])) for i in range(3)])
    if {(2, 1), (2, 2)} & _ratios(samp):
        assert "replicate" in methods and ({"h2v1_fancy", "h2v2_fancy"} & methods)   # both sides of cw > 2 were run


def _ratios(samp):
    hmax, vmax = max(h for h, _ in samp), max(v for _, v in samp)
    return {(hmax // h, vmax // v) for h, v in samp}


@pytest.mark.parametrize("name", ["grey", "chroma_1x1", "chroma_2x1", "chroma_2x2", "chroma_1x2", "chroma_3x1", "luma_2x2"])
def test_rows_wider_than_one_thread_block(ctx, name):
    """W = 1024 fills one block of k_jpeg_pixels (256 threads of four pixels); 1028 and 1029 start a second, with whole words and with
    a byte tail"""
    rng = np.random.default_rng(sum(map(ord, name)) + 1)
    for W in (1024, 1028, 1029):
        L = JB.layout_for(W, 3, JB.SAMPLINGS[name])
        blobs = _legal_blobs(L, 2, rng, ycc=[1, 0])
        assert np.array_equal(ctx.jpeg_pixels(L, blobs), JR.pixels(L, blobs)), (name, W)


def test_colour_conversion_at_its_clamps(ctx):
    """jdcolor.c's conversion on flat blocks (quantiser 1, DC 8 (v - 128)): (Y, Cb, Cr) over {0, 1, 127, 128, 129, 254, 255}^3, all 256
    values of Cb and of Cr at Y = 0, 128 and 255 beside a neutral other chroma, and all 256 values of Cb beside a Cr that moves with
    it (the green channel rounds the sum of both terms once).  One 4:4:4 image of 61 x 35 blocks, one block per triple; as YCbCr and
    as Adobe RGB, where the three samples are the pixel.  A constant of the conversion that is off by enough to change any of its 256
    results changes one here; 91881, the Cr -> R factor, gives the same 256 results anywhere from 91879 to 91892."""
    edge = (0, 1, 127, 128, 129, 254, 255)
    t = [(y, cb, cr) for y in edge for cb in edge for cr in edge]
    t += [(y, v, 128) for y in (0, 128, 255) for v in range(256)] + [(y, 128, v) for y in (0, 128, 255) for v in range(256)]
    t += [(128, v, (7 * v + 3) % 256) for v in range(256)]
    t = np.array(t)
    assert len(t) == 61 * 35
    L = JB.layout_for(61 * 8, 35 * 8, JB.SAMPLINGS["chroma_1x1"])
    flat = JB.flat_coefs(L, [t[:, c].reshape(35, 61) for c in range(3)])
    ones = [np.ones((2, 8, 8), np.uint16)] * 3
    blobs = JB.blobs_for(L, [np.stack([f, f]) for f in flat], ones, [1, 0])
    assert blobs.nbytes < (1 << 21)
    want = JR.pixels(L, blobs)
    assert np.array_equal(want[1][::8, ::8].reshape(-1, 3), t)   # the copy: the samples themselves, so the blocks are what was asked for
    rgb = want[0][::8, ::8].reshape(-1, 3)
    assert (rgb == 0).any(axis=0).all() and (rgb == 255).any(axis=0).all()   # every channel reaches both clamps
    got = ctx.jpeg_pixels(L, blobs)
    for i, what in enumerate(("YCbCr", "Adobe RGB")):
        bad = np.unique((got[i] != want[i]).any(axis=2)[::8, ::8].reshape(-1).nonzero()[0])
        assert np.array_equal(got[i], want[i]), (what, "triples that differ", [tuple(x) for x in t[bad][:10]])


# ---- the chunk path ----
def test_a_chunk_of_small_images_through_process_files(ctx, tmp_path):
    """70 constructed 4:2:0 files of 40 x 40 (54 blocks each, so every wavefront of the chunk's inverse DCT holds two images) through
    hesaff_process_files: every output file equals the output for the image's PPM twin, written from the host reader's pixels.
    tests/test_jpeg_constructed_host.py checks on the CPU that the oracle finds keys in this set."""
    jpgs, ppms = [], []
    for i, data in enumerate(JB.chunk_files()):
        q = str(tmp_path / ("c%02d.jpg" % i))
        open(q, "wb").write(data)
        pix = hesaff_amd.read_image(q)
        assert pix.shape == (40, 40, 3)
        p = str(tmp_path / ("c%02d.ppm" % i))
        open(p, "wb").write(b"P6\n40 40\n255\n" + pix.tobytes())
        jpgs.append(q); ppms.append(p)
    assert len(jpgs) == 70
    st_j = ctx.process_files(jpgs, decode_threads=2, write_threads=2)
    st_p = ctx.process_files(ppms, decode_threads=2, write_threads=2)
    keys = 0
    for q, p, sj, sp in zip(jpgs, ppms, st_j, st_p):
        assert sj[0] == 0 and sp[0] == 0 and sj == sp, (q, sj, sp)
        assert open(q + ".hesaff.sift", "rb").read() == open(p + ".hesaff.sift", "rb").read(), q
        keys += sj[3]
    assert keys >= 1
