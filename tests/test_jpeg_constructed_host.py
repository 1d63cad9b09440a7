"""CPU suite of the constructed JPEG inputs: pins the plain reference of the device stage (tests/jpeg_ref.py) and the writer of
constructed files (tests/jpeg_build.py) to hesaff_read_jpeg, to hesaff_read_jpeg_coefficients and - where Pillow imports - to
libjpeg-turbo, before tests/test_jpeg_constructed.py holds the kernels of kernels_jpeg.h to that reference on the GPU.  Also here:
the geometry of hesaff_amd/csrc/jpeg_plan.h under AddressSanitizer + UBSan (a stand-alone program with its own main; nothing is
preloaded) and the refusal of interleaved scans of more than 10 blocks per MCU.  Nothing here needs a GPU."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from tests import jpeg_build as JB
from tests import jpeg_ref as JR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
SAN = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer"]
IO = -4
SIZES = [(1, 1), (2, 3), (3, 2), (5, 7), (8, 8), (9, 5), (12, 9), (13, 17), (16, 16), (17, 33)]   # (W, H)


def _pillow():
    try:
        from PIL import Image
        return Image
    except ImportError:
        return None


def _pillow_pixels(Image, path):
    im = Image.open(path)
    return np.asarray(im if im.mode == "L" else im.convert("RGB"))


@pytest.mark.parametrize("name", sorted(JB.FILE_SAMPLINGS))
def test_constructed_files_reader_reference_and_libjpeg_agree(name, tmp_path):
    """For every sampling layout a file can have, ten sizes from 1 x 1 to 17 x 33, YCbCr and Adobe transform 0, legal-range
    coefficients that differ block by block:
      * the reference's pixels of blob_for(...) equal hesaff_read_jpeg's of write_jpeg(...), in its wrapping and non-wrapping form;
      * hesaff_read_jpeg_coefficients of that file returns, byte for byte, the layout and the blob layout_for / blob_for made (the
        entropy decoder's block placement at this layout);
      * where Pillow imports, all of them equal libjpeg-turbo's decode (only this leg needs Pillow)."""
    Image = _pillow()
    samp = JB.FILE_SAMPLINGS[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    p = str(tmp_path / "c.jpg")
    n = 0
    for (W, H) in SIZES:
        for adobe in ((None,) if len(samp) == 1 else (None, 0)):
            L = JB.layout_for(W, H, samp)
            coefs, quants = JB.legal_coefs(L, n, rng), JB.legal_quants(L, rng)
            restart = 2 if (W, H) == (17, 33) else 0   # one size with restart markers: a check of the writer more than of the reader
            open(p, "wb").write(JB.write_jpeg(W, H, samp, coefs, quants, adobe=adobe, restart=restart))
            blob = JB.blob_for(L, coefs, quants, ycc=adobe is None)
            want = JR.pixels(L, blob)[0]
            got = hesaff_amd.read_image(p)
            assert got.shape == want.shape and np.array_equal(got, want), (name, W, H, adobe)
            assert np.array_equal(JR.pixels(L, blob, idct=JR.idct_islow_nonwrapping)[0], want), (name, W, H, adobe)
            lay, rblob = hesaff_amd.read_jpeg_coefficients(p)
            assert JB.layout_tuple(lay) == JB.layout_tuple(L), (name, W, H)
            assert rblob.shape == blob.shape and np.array_equal(rblob, blob), (name, W, H, adobe)
            if Image is not None:
                assert np.array_equal(_pillow_pixels(Image, p), want), (name, W, H, adobe)
            n += 1
    assert n == (10 if len(samp) == 1 else 20)


def _wrap_case(rng, W=48, H=48):
    """the wrap family as a file can carry it: a grey image, 16-bit quantisers, |coefficient| <= 1023 at every position"""
    L = JB.layout_for(W, H, [(1, 1)])
    coefs = [rng.integers(-1023, 1024, (L.bh[0], L.bw[0], 8, 8)).astype(np.int16)]
    quants = [rng.integers(1, 65536, (8, 8)).astype(np.uint16)]
    return L, coefs, quants


def test_transform_wraps_at_32_bits_through_a_file(tmp_path):
    """A grey file with a 16-bit quantisation table and |coefficient| <= 1023 drives the transform out of 32 bits.  The host reader
    equals the wrapping reference (jpeg_decode.cpp W32: the project's definition of such streams), and the int64 restatement, which
    does not wrap, differs from it on at least a quarter of the pixels - so this input does tell the two apart."""
    rng = np.random.default_rng(32)
    L, coefs, quants = _wrap_case(rng)
    p = str(tmp_path / "wrap.jpg")
    open(p, "wb").write(JB.write_jpeg(48, 48, [(1, 1)], coefs, quants, q16=True))
    blob = JB.blob_for(L, coefs, quants, ycc=False)
    lay, rblob = hesaff_amd.read_jpeg_coefficients(p)
    assert JB.layout_tuple(lay) == JB.layout_tuple(L) and np.array_equal(rblob, blob)
    want = JR.pixels(L, blob)[0]
    assert np.array_equal(hesaff_amd.read_image(p), want)
    plain = JR.pixels(L, blob, idct=JR.idct_islow_nonwrapping)[0]
    differ = float((plain != want).mean())
    print("non-wrapping variant differs on %.1f %% of %d pixels" % (100 * differ, want.size))
    assert differ >= 0.25, differ


@pytest.mark.parametrize("name", ["jpeg_gray_q90", "jpeg_420_q85", "jpeg_422_q70_rst", "jpeg_prog_420_q80", "jpeg_prog_gray_q60"])
def test_reference_decodes_the_committed_fixtures(name):
    """The reference on encoder-made coefficients: colour, 4:2:0 and 4:2:2, sequential and progressive, equal to the committed
    libjpeg-turbo decode."""
    lay, blob = hesaff_amd.read_jpeg_coefficients(os.path.join(GOLD, name + ".jpg"))
    want = hesaff_amd.read_pnm(os.path.join(GOLD, name + (".pgm" if lay.channels == 1 else ".ppm")))
    assert np.array_equal(JR.pixels(lay, blob)[0], want)
    assert np.array_equal(JR.pixels(lay, blob, idct=JR.idct_islow_nonwrapping)[0], want)


@pytest.mark.parametrize("name", sorted(JB.OVERSIZED_SAMPLINGS))
def test_interleaved_scan_of_more_than_ten_blocks_is_refused(name, tmp_path):
    """Luma 3x3, 4x3, 3x4 or 4x4 beside two 1x1 chroma components: 11 to 18 blocks in an interleaved MCU.  libjpeg refuses such a scan
    (JERR_BAD_MCU_SIZE), so cv::imread has no pixels for the file; both readers return HESAFF_ERR_IO.  The same frame coded as one
    scan per component is legal, as in libjpeg, and decodes to the reference's pixels."""
    Image = _pillow()
    samp = JB.OVERSIZED_SAMPLINGS[name]
    assert 11 <= JB.mcu_blocks(samp) <= 18
    rng = np.random.default_rng(sum(map(ord, name)))
    W, H = 37, 29
    L = JB.layout_for(W, H, samp)
    coefs, quants = JB.legal_coefs(L, 0, rng), JB.legal_quants(L, rng)
    p = str(tmp_path / "big_mcu.jpg")
    open(p, "wb").write(JB.write_jpeg(W, H, samp, coefs, quants))
    for reader in (hesaff_amd.read_image, hesaff_amd.read_jpeg_coefficients):
        with pytest.raises(hesaff_amd.HesaffError) as e:
            reader(p)
        assert e.value.code == IO
    if Image is not None:
        with pytest.raises(Exception):
            Image.open(p).load()
    # one scan per component: blocks beyond ceil(cw / 8) x ceil(chgt / 8) are in no scan and stay zero
    for c in range(3):
        keep = np.zeros((L.bh[c], L.bw[c]), bool)
        keep[:-(-L.chgt[c] // 8), :-(-L.cw[c] // 8)] = True
        coefs[c][~keep] = 0
    open(p, "wb").write(JB.write_jpeg(W, H, samp, coefs, quants, interleaved=False))
    blob = JB.blob_for(L, coefs, quants, ycc=True)
    want = JR.pixels(L, blob)[0]
    assert np.array_equal(hesaff_amd.read_image(p), want)
    lay, rblob = hesaff_amd.read_jpeg_coefficients(p)
    assert JB.layout_tuple(lay) == JB.layout_tuple(L) and np.array_equal(rblob, blob)
    if Image is not None:
        assert np.array_equal(_pillow_pixels(Image, p), want)


def test_exactly_ten_blocks_per_mcu_still_decode(tmp_path):
    """luma 4x2 and two 1x1 chroma: the largest legal interleaved MCU"""
    samp = [(4, 2), (1, 1), (1, 1)]
    assert JB.mcu_blocks(samp) == 10
    rng = np.random.default_rng(10)
    W, H = 37, 29
    L = JB.layout_for(W, H, samp)
    coefs, quants = JB.legal_coefs(L, 0, rng), JB.legal_quants(L, rng)
    p = str(tmp_path / "ten.jpg")
    open(p, "wb").write(JB.write_jpeg(W, H, samp, coefs, quants))
    blob = JB.blob_for(L, coefs, quants, ycc=True)
    assert np.array_equal(hesaff_amd.read_image(p), JR.pixels(L, blob)[0])
    lay, rblob = hesaff_amd.read_jpeg_coefficients(p)
    assert JB.layout_tuple(lay) == JB.layout_tuple(L) and np.array_equal(rblob, blob)


def test_the_chunk_set_has_keys_and_decodes_to_the_reference(oracle, tmp_path):
    """The 70 files tests/test_jpeg_constructed.py sends through hesaff_process_files: 54 blocks each, fewer than a wavefront takes; the
    host reader's pixels are the reference's, and the oracle finds keys in them - so equal output files there mean equal keys, not
    equally empty files."""
    L, samp, coefs, quants = JB.chunk_set()
    assert JB.blocks_per_image(L) == 54
    want = JR.pixels(L, JB.blobs_for(L, coefs, quants, [1] * 70))
    p = str(tmp_path / "c.jpg")
    keys = 0
    for i, data in enumerate(JB.chunk_files()):
        open(p, "wb").write(data)
        pix = hesaff_amd.read_image(p)
        assert np.array_equal(pix, want[i]), i
        keys += oracle.OracleRun(oracle.gray_from_u8(pix)).n_keys
    print("keys over the set:", keys)
    assert keys >= 1


def test_jpeg_plan_arithmetic(tmp_path):
    """tests/native/jpeg_plan_check.cpp under AddressSanitizer + UBSan: every bound of make_jpeg_geom on both sides, the up-sampling
    method of every ratio at cw = 1, 2, 3, offsets and sizes of the constructed tests' layouts, and - for every accepted layout of an
    exhaustive sweep over W, H in 1 .. 20 and all integral factor triples - that no sample index k_jpeg_pixels can form leaves the
    component's plane.  jpeg_plan.h is compiled here without HIP."""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "jpeg_plan_check")
    r = subprocess.run(SAN + ["-o", exe, os.path.join(ROOT, "tests", "native", "jpeg_plan_check.cpp"), "-lpthread"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "jpeg_plan_check ok" in r.stdout, (r.stdout[-2000:], r.stderr[-6000:])


def test_the_plan_check_restates_the_table_layouts():
    """the layouts jpeg_plan_check.cpp lists are the ones layout_for makes for the GPU suite's block-addressing table"""
    src = open(os.path.join(ROOT, "tests", "native", "jpeg_plan_check.cpp")).read()
    for W, H, name, blocks in [(8, 8, "grey", 1), (1, 1, "grey", 1), (5, 3, "grey", 1), (8, 8, "chroma_1x1", 3), (16, 16, "chroma_2x2", 6),
                               (40, 40, "chroma_2x2", 54), (56, 72, "grey", 63), (64, 64, "grey", 64), (40, 104, "grey", 65)]:
        L = JB.layout_for(W, H, JB.SAMPLINGS[name])
        assert JB.blocks_per_image(L) == blocks, (W, H, name)
        row = "{%d, %d, %d, {%s}, {%s}, %d}" % (W, H, L.channels, ", ".join(str(L.h[i]) for i in range(L.channels)),
                                               ", ".join(str(L.v[i]) for i in range(L.channels)), blocks)
        assert row in src, row
