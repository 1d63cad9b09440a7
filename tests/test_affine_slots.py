"""k_affine_stage's sixteen keypoint slots per wavefront (hs_affine_groups): slot and batch remainders, every kind of keypoint in
every slot, border windows beside inside windows in one batch, a refill of every slot of every block, batches without an active slot.
All through ctx.find_affine_shape on one 240 x 320 image against the CPU oracle: converged and iters equal, U bit-equal where the
reference reports a shape (tests/test_gpu_parity.py::test_affine_shape_stage's conventions)."""
import numpy as np
import pytest

from hesaff_amd.synth import band_noise_image

pytestmark = pytest.mark.gpu

SMALL_BANDS = ((1.5, 40.0), (3.0, 40.0), (6.0, 50.0))
SLOTS = 16            # keypoint slots of a wavefront
STAGE_BLOCKS = 1536   # the stage launch's grid limit


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


class _Ref:
    pass


@pytest.fixture(scope="module")
def ref(oracle):
    """The oracle's results for the octave-0 level-1 keypoints of the image, computed once and left unchanged."""
    img = band_noise_image(240, 320, 21, SMALL_BANDS)
    o = oracle.OracleRun(oracle.gray_from_u8(img), keep_planes=True)
    f, i = o.hessian()
    U, ci = o.affine()
    sel = np.where((i[:, 1] == 0) & (i[:, 2] == 1))[0]
    r = _Ref()
    r.blur = o.plane(0, 0, 1)
    r.kp = np.ascontiguousarray(f[sel][:, :4])
    r.conv = ci[sel, 0].copy()
    r.iters = ci[sel, 1].copy()
    r.U = U[sel].copy()
    # the list the tests cut and permute holds every kind of keypoint: ones that never converge, early and late ones
    assert len(sel) == 379
    assert (r.conv == 0).sum() >= 1
    its = r.iters[r.conv == 1]
    assert len(np.unique(its)) >= 5 and (its >= 6).any() and (its <= 3).any()
    for a in (r.blur, r.kp, r.conv, r.iters, r.U):
        a.setflags(write=False)
    return r


def _check(ctx, ref, rows, what):
    """Runs the keypoints ref.kp[rows] (any order, repeats allowed) and compares each row with the oracle's result of its source."""
    rows = np.asarray(rows, np.int64)
    conv, Ug, it = ctx.find_affine_shape(ref.blur, ref.kp[rows])
    assert np.array_equal(conv, ref.conv[rows]), (what, np.flatnonzero(conv != ref.conv[rows])[:8])
    ok = ref.conv[rows] == 1
    assert np.array_equal(it[ok], ref.iters[rows][ok]), (what, np.flatnonzero(it[ok] != ref.iters[rows][ok])[:8])
    a = np.ascontiguousarray(Ug[ok], np.float32); b = np.ascontiguousarray(ref.U[rows][ok], np.float32)
    ne = (_bits(a) != _bits(b)) & ~((a == 0) & (b == 0))   # +0 / -0 are the same value for every later operation
    assert not ne.any(), (what, "U differs in %d rows, first %s" % (ne.any(axis=1).sum(), np.flatnonzero(ne.any(axis=1))[:8]))


@pytest.mark.parametrize("n", [1, 3, 4, 5, 15, 16, 17, 31, 33, 63, 64, 65, 379])
def test_slot_and_batch_remainders(ctx, ref, n):
    """The first n keypoints: partial batches, partial items, and (n = 17: one keypoint in block 1; n <= 4 in any block) batches
    whose four slots are all idle while another batch of the wavefront goes on iterating."""
    _check(ctx, ref, np.arange(n), "first %d" % n)


@pytest.mark.parametrize("rot", range(SLOTS))
def test_every_kind_in_every_slot(ctx, ref, rot):
    """The list rotated by 0..15: each slot and batch sees early, late (iters >= 6) and never converging keypoints, and finished
    slots refill while their batch neighbours still iterate."""
    _check(ctx, ref, np.roll(np.arange(len(ref.kp)), -rot), "rotated by %d" % rot)


def test_border_windows_beside_inside_windows(ctx, ref, oracle):
    """One border window per batch of four slots makes the batch take the bounds-tested taps for its three interior windows too."""
    x, y, s, pd = (ref.kp[:, j] for j in range(4))
    rows, cols = ref.blur.shape
    edge = np.minimum(np.minimum(x / pd, y / pd), np.minimum(cols - 1 - x / pd, rows - 1 - y / pd))
    # on the first iteration the 19 x 19 window reaches 9 * s / (1.6 * pd) pixels from the centre (affine.h:40: initialSigma 1.6)
    border = np.flatnonzero(edge < 9 * s / (1.6 * pd) - 1.0)
    inner = np.flatnonzero(edge > 40.0)
    assert len(border) >= 8 and len(inner) >= 3 * len(border)
    assert 0 in border      # the first of the selection: y ~ 4.8, s ~ 2.3
    order = []
    for j, b in enumerate(border):
        order += [b] + list(inner[3 * j:3 * j + 3])
    _check(ctx, ref, order, "one border window per batch")
    _check(ctx, ref, order[1:], "the border window in another slot of the batch")
    # one keypoint on a 13 x 13 plane, the smallest an octave can be: every iteration's window crosses the border
    small = np.ascontiguousarray(ref.blur[120:133, 40:53])
    want_conv, want_U, want_it = oracle.OracleHandle().find_affine_shape(small, 6.3, 6.2, 0.4, 1.0)
    assert want_conv == 1 and want_it == 5
    conv, Ug, it = ctx.find_affine_shape(small, np.array([[6.3, 6.2, 0.4, 1.0]], np.float32))
    assert conv.tolist() == [1] and it.tolist() == [want_it]
    assert np.array_equal(_bits(Ug[0]), _bits(want_U))


def test_refill_in_every_block(ctx, ref):
    """2 x 16 x 1536 + 5 rows: the grid is at its limit, every slot of every block takes a second keypoint and the last item is partial."""
    n = 2 * SLOTS * STAGE_BLOCKS + 5
    _check(ctx, ref, np.arange(n) % len(ref.kp), "%d rows" % n)
