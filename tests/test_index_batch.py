"""GPU suite of batched index queries (hesaff_index_query_batch*, include/hesaff_amd.h; kernels_index_batch.h).  Every comparison is
bit for bit and is made twice: per query against the definition in numpy (tests/index_ref.py, tests/embedding_ref.py), and against
the bytes the single-query call returns for the same words on the same context."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import hesaff_amd
from tests import embedding_ref as E
from tests import index_ref as R
from tests import vocabulary_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
EXE = os.path.join(ROOT, "hesaff_amd", "bin", "hesaff")
E2E_IMAGES = ["band_160x120", "band_96x96", "band_160x120", "tiny_20x15", "band_96x96"]
E2E_KEYS = [221, 74, 221, 0, 74]
ARG = -2
MASK64 = (1 << 64) - 1
DEFAULT_BUDGET = 1 << 30


# ---- index_batch_plan.h in Python: the layout of a chunk's scratch and the chunk rule ----

def hash_bits(total):
    bits = 10
    while (1 << bits) < 2 * total:
        bits += 1
    return bits


def hash_slot(query, word, bits):
    return ((((query << 20) | word) * 0x9E3779B97F4A7C15) & MASK64) >> (64 - bits)


def chunk_bytes(b, n_images, keep, words):
    end = 0
    slots = 1 << hash_bits(words)
    for count, size in ((b * n_images, 8), (b, 16), (slots, 4), (slots, 8), (b * n_images, 8), (b * keep * 12, 1)):
        if count:
            end = (end + 255) // 256 * 256 + count * size
    return end


def chunks_of(counts, n_images, keep, budget):
    out, first = [], 0
    while first < len(counts):
        b, words = 1, counts[first]
        while first + b < len(counts) and chunk_bytes(b + 1, n_images, keep, words + counts[first + b]) <= budget:
            words += counts[first + b]
            b += 1
        out.append(b)
        first += b
    return out


# ---- helpers ----

def _params(**kw):
    p = hesaff_amd.default_params()
    for k, v in kw.items():
        setattr(p, k, v)
    return p


@pytest.fixture(scope="module")
def bctx():
    with hesaff_amd.HesaffContext(_params(max_batch=5), device=0) as c:
        yield c


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _rows(words, stride):
    """(word, dist2) rows of a word array; dist2 is never read as a word"""
    words = np.asarray(words, np.int32)
    if stride == 1:
        return words
    return np.stack([words, np.full(len(words), -7, np.int32)], axis=1) if len(words) else np.zeros((0, 2), np.int32)


def _collection(N, K, seed):
    """N images of 0 .. 40 random words; with N >= 3 the first, the middle and the last image have no key; word K - 1 lies in
    exactly one image"""
    rng = np.random.RandomState(seed)
    images = [rng.randint(0, max(K - 1, 1), rng.randint(0, 41)).astype(np.int32) for _ in range(N)]
    if N >= 3:
        for i in (0, N // 2, N - 1):
            images[i] = np.zeros(0, np.int32)
    one = 1 if N >= 3 else 0
    images[one] = np.concatenate([images[one], [K - 1, K - 1]]).astype(np.int32)
    return images


def _batch_of(Q, K, seed, images):
    """Q queries: of 0 words first, in the middle and last (Q >= 3); one query twice; two queries that share every word; 4099 keys in
    one word; an indexed image; random words with repeats"""
    rng = np.random.RandomState(seed)
    qs = [rng.randint(0, K, rng.randint(1, 41)).astype(np.int32) for _ in range(Q)]
    if Q >= 8:
        qs[1] = images[min(1, len(images) - 1)].copy()
        qs[3] = qs[2].copy()                          # one query repeated
        qs[5] = rng.permutation(qs[4]).astype(np.int32)   # every word shared, in another order
        qs[6] = np.full(4099, K - 1, np.int32)
    if Q >= 3:
        for i in (0, Q // 2, Q - 1):
            qs[i] = np.zeros(0, np.int32)
    return qs


def _device(arrays, stride):
    import torch
    flat = np.concatenate([_rows(a, stride) for a in arrays]) if sum(len(a) for a in arrays) else np.zeros((1,) if stride == 1 else (1, 2), np.int32)
    t = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
    torch.cuda.synchronize()
    return t, flat


def _run_batch(ctx, queries, top, device=False, stride=1, sigs=None, T=None):
    if device:
        import torch
        t, flat = _device(queries, stride)
        ts = None
        if sigs is not None:
            flat_sigs = np.concatenate(list(sigs) + [np.zeros(1, np.uint64)]).astype(np.uint64)   # (never empty: one signature beyond the batch's)
            ts = torch.from_numpy(flat_sigs.view(np.int64)).cuda()
            torch.cuda.synchronize()
        out = ctx.query_index_batch_device(t.data_ptr(), [len(q) for q in queries], stride, top, sigs_ptr=None if ts is None else ts.data_ptr(), hamming=T)
        assert np.array_equal(t.cpu().numpy(), flat)   # the source is only read
        return out
    return ctx.query_index_batch([_rows(q, stride) for q in queries], top, signatures=sigs, hamming=T)


def _singles(ctx, queries, top, sigs=None, T=None):
    """the single-query call per query, in order: the rows, and the scores the last one leaves"""
    im, sc = [], []
    for j, q in enumerate(queries):
        a, b = ctx.query_index(q, top) if sigs is None else ctx.query_index(q, top, signatures=sigs[j], hamming=T)
        im.append(a); sc.append(b)
    return np.array(im, np.int32).reshape(len(queries), -1), np.array(sc, np.float64).reshape(len(queries), -1), ctx.index_scores()


def _same_scores(a, b):
    return a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2] == b[2]


def _check_batch(ctx, queries, top, what, refs=None, n_images=None, **how):
    """a batch against the single calls on the same context and, with refs (per query what R.query / E.query returns for the full
    ranking), against the definition"""
    sim, ssc, sstate = _singles(ctx, queries, top, how.get("sigs"), how.get("T"))
    im, sc = _run_batch(ctx, queries, top, **how)
    assert im.dtype == np.int32 and sc.dtype == np.float64 and im.shape == sc.shape == sim.shape, (what, im.shape, sim.shape)
    assert im.tobytes() == sim.tobytes(), (what, "ranked images against the single calls", np.nonzero((im != sim).any(axis=1))[0][:8].tolist())
    assert sc.tobytes() == ssc.tobytes(), (what, "ranked scores against the single calls")
    assert _same_scores(ctx.index_scores(), sstate), (what, "the last query's dot, score and nq2")
    if refs is not None:
        keep = min(top, n_images)
        for q, ref in enumerate(refs):
            assert im[q].tolist() == ref[0][:keep].tolist(), (what, "query %d: ranked images against the definition" % q)
            assert np.array_equal(_bits(sc[q]), _bits(ref[1][:keep])), (what, "query %d: ranked scores against the definition" % q)
        dot, score, nq2 = ctx.index_scores()
        assert nq2 == refs[-1][4] and np.array_equal(dot, refs[-1][2]) and np.array_equal(_bits(score), _bits(refs[-1][3])), (what, "state against the definition")
    return im, sc


# ---------------------------------------------------------------- shapes

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 33, 4099])
def test_batch_shapes(bctx, K):
    """N in {1, 3, 65, 257, 1025} at this K with keyless images; Q = 67 (queries of 0 words first, in the middle and last, one query
    twice, two that share every word, 4099 keys in one word), Q = 2 and Q = 1; top = 1, N, above N and 1024; word_stride 1 and 2;
    host and device forms"""
    bctx.set_index_batch_budget(0)
    for N in (1, 3, 65, 257, 1025):
        images = _collection(N, K, seed=300 + N)
        bctx.build_index(images, K)
        ref = R.build(images, K)
        queries = _batch_of(67, K, seed=11 + N, images=images)
        refs = [R.query(ref, q, N) for q in queries]
        tops = sorted({1, N, N + 1, 1024} if N == 1025 else {1, N, N + 1})
        for top in tops:
            if top > 1024:
                continue
            what = "N = %d, K = %d, top = %d" % (N, K, top)
            im, sc = _check_batch(bctx, queries, top, what, refs=refs, n_images=N)
            assert im.shape == (67, min(top, N))
            assert im[2].tobytes() == im[3].tobytes() and sc[2].tobytes() == sc[3].tobytes(), (what, "one query twice")
            assert im[4].tobytes() == im[5].tobytes() and sc[4].tobytes() == sc[5].tobytes(), (what, "two queries of the same words")
            assert (sc[0] == 0.0).all() and im[0].tolist() == list(range(min(top, N))), (what, "a query of 0 words")
        top = min(N, 7)
        host = _run_batch(bctx, queries, top)
        for device, stride in ((True, 1), (False, 2), (True, 2)):
            got = _run_batch(bctx, queries, top, device=device, stride=stride)
            assert got[0].tobytes() == host[0].tobytes() and got[1].tobytes() == host[1].tobytes(), (N, K, device, stride)
        for Q in (1, 2):
            for first in (1, 6, 0):   # an indexed image, the 4099-key query, a query of 0 words
                _check_batch(bctx, queries[first:first + Q], top, "N = %d, K = %d, Q = %d from %d" % (N, K, Q, first), refs=refs[first:first + Q], n_images=N)
                _check_batch(bctx, queries[first:first + Q], top, "device", refs=refs[first:first + Q], n_images=N, device=True)


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("embedded", [False, True])
def test_batch_forms_at_one_small_shape(bctx, embedded, device, stride):
    """hesaff_index_query_batch[_embedded][_device] at word_stride 1 and 2 over 3 images and K = 5: a batch of 3 queries with the
    middle one empty, a batch of queries that hold no word at all, and the first or the last word at -1 or K, refused under the
    entry point's own name with the last query's scores left as they were.  Everything here is host plumbing and per-key device
    code with no tile size in it, so the shape is small."""
    bctx.set_index_batch_budget(0)
    K, T = 5, 24 if embedded else None
    images = [np.array([0, 3, 3, 4, 1, 0, 3], np.int32), np.zeros(0, np.int32), np.array([4, 2], np.int32)]
    isigs = [np.array([1, 2, 3, 0xFF, 5, 1, 7], np.uint64), np.zeros(0, np.uint64), np.array([0xF0, 9], np.uint64)]
    queries = [np.array([3, 0, 3, 4], np.int32), np.zeros(0, np.int32), np.array([2, 4, 4], np.int32)]
    qsigs = [np.array([3, 1, 6, 0xF1], np.uint64), np.zeros(0, np.uint64), np.array([9, 0xF0, 0xF0F0F0], np.uint64)]
    bctx.build_index(images, K, signatures=isigs if embedded else None)
    ref = R.build(images, K)
    how = dict(device=device, stride=stride, sigs=qsigs if embedded else None, T=T)
    what = "embedded %s, device %s, stride %d" % (embedded, device, stride)
    refs = [E.query(ref, images, isigs, q, g, T, 3) if embedded else R.query(ref, q, 3) for q, g in zip(queries, qsigs)]
    im, sc = _check_batch(bctx, queries, 2, what, refs=refs, n_images=3, **how)
    assert im[1].tolist() == [0, 1] and (sc[1] == 0.0).all(), (what, "the query of 0 words")
    none = dict(how, sigs=[g[:0] for g in qsigs] if embedded else None)
    im, sc = _check_batch(bctx, [q[:0] for q in queries], 2, what + ", no word at all", **none)
    assert im.tolist() == [[0, 1]] * 3 and (sc == 0.0).all(), (what, "a batch of 0 words")
    state = bctx.index_scores()
    name = "hesaff_index_query_batch%s%s" % ("_embedded" if embedded else "", "_device" if device else "")
    for at, w in ((0, -1), (0, K), (-1, -1), (-1, K)):
        bad = [q.copy() for q in queries]
        bad[0 if at == 0 else 2][at] = w
        with pytest.raises(hesaff_amd.HesaffError, match=name + r": a word lies outside 0 \.\. vocabulary_size - 1$"):
            _run_batch(bctx, bad, 2, **how)
    assert _same_scores(bctx.index_scores(), state), (what, "after the refusals")
    _check_batch(bctx, queries, 2, what + ", after the refusals", refs=refs, n_images=3, **how)


@pytest.mark.gpu
def test_batch_word_patterns(bctx):
    """a word of every image (idf 0) beside a word of one image; words with df = 0; every query word distinct"""
    bctx.set_index_batch_budget(0)
    everywhere = [np.array([0, 5], np.int32), np.array([0, 0, 6], np.int32), np.array([0], np.int32), np.array([0, 7, 7], np.int32)]
    bctx.build_index(everywhere, 9)
    ref = R.build(everywhere, 9)
    assert ref[2][0] == 0 and ref[1][5] == 1 and ref[1][8] == 0
    queries = [np.array(q, np.int32) for q in ([0], [0, 0, 7], [5, 6, 7], [8], [8, 8, 5, 8], [0, 8], [5])]
    for top in (1, 4, 9):
        im, sc = _check_batch(bctx, queries, top, "idf 0 and df 0, top %d" % top, refs=[R.query(ref, q, 4) for q in queries], n_images=4)
        assert (sc[0] == 0.0).all() and (sc[3] == 0.0).all() and (sc[5] == 0.0).all()
    distinct = [np.arange(4099, dtype=np.int32), np.arange(4099, dtype=np.int32)[::-1].copy(), np.arange(0, 4099, 2, dtype=np.int32)]
    bctx.build_index(distinct, 4099)
    ref = R.build(distinct, 4099)
    queries = [np.arange(1, 4099, 2, dtype=np.int32), np.arange(4099, dtype=np.int32), np.zeros(0, np.int32), np.arange(0, 4099, 2, dtype=np.int32)]
    _check_batch(bctx, queries, 3, "every key a different word", refs=[R.query(ref, q, 3) for q in queries], n_images=3)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [511, 512, 513])
def test_batch_around_the_minimum_table_size(bctx, T):
    """T words in a chunk around the smallest table (1024 slots for T <= 512, 2048 beyond): distinct words of query 0 and 1 chosen
    from K = 4099 so that their first slots are the LAST of the chunk's table - several keys per slot, and the probing wraps"""
    bits = hash_bits(T)
    assert (1 << bits) == (1024 if T <= 512 else 2048)
    half = T // 2
    picks = []
    for query, n in ((0, half), (1, T - half)):
        words = sorted(range(4099), key=lambda w: -hash_slot(query, w, bits))[:n]
        slots = [hash_slot(query, w, bits) for w in words]
        assert len(set(slots)) < len(slots)
        picks.append(np.array(words, np.int32))
    assert min(hash_slot(i, int(w), bits) for i, p in enumerate(picks) for w in p) + T > (1 << bits)   # the run wraps
    rng = np.random.RandomState(T)
    images = [rng.randint(0, 4099, 60).astype(np.int32) for _ in range(30)] + [picks[0][:50].copy(), picks[1][::3].copy()]
    bctx.build_index(images, 4099)
    ref = R.build(images, 4099)
    queries = [rng.permutation(picks[0]).astype(np.int32), rng.permutation(picks[1]).astype(np.int32)]
    refs = [R.query(ref, q, 32) for q in queries]
    bctx.set_index_batch_budget(0)
    _check_batch(bctx, queries, 5, "T = %d" % T, refs=refs, n_images=32)
    assert bctx.index_batch_chunks == 1
    _check_batch(bctx, queries, 5, "T = %d, device" % T, refs=refs, n_images=32, device=True)
    # the same words twice over: the counts are 2, the table the same
    _check_batch(bctx, [np.concatenate([q, q]) for q in queries[:1]] + queries[1:], 5, "T = %d, doubled" % T, n_images=32)
    bctx.set_index_batch_budget(1)   # every query a chunk of its own: both are query 0 of their chunk
    _check_batch(bctx, queries, 5, "T = %d, one query per chunk" % T, refs=refs, n_images=32)
    assert bctx.index_batch_chunks == 2
    bctx.set_index_batch_budget(0)


# ---------------------------------------------------------------- chunks

@pytest.mark.gpu
def test_chunk_boundaries_do_not_show(bctx):
    """one Q = 67 batch at budgets that give chunks of one query, of two, an uneven split and one chunk: byte-equal outputs; the
    getter returns what was set, and 0 restores the default"""
    N, K, top = 257, 33, 10
    images = _collection(N, K, seed=5)
    bctx.build_index(images, K)
    rng = np.random.RandomState(77)
    queries = [rng.randint(0, K, rng.randint(0, 8)).astype(np.int32) for _ in range(67)]   # under 512 words in all: the table stays at 1024 slots
    counts = [len(q) for q in queries]
    ref = R.build(images, K)
    refs = [R.query(ref, q, N) for q in queries]
    bctx.set_index_batch_budget(0)
    assert bctx.index_batch_budget == DEFAULT_BUDGET
    want = _check_batch(bctx, queries, top, "the default budget", refs=refs, n_images=N)
    assert bctx.index_batch_chunks == 1 == len(chunks_of(counts, N, top, DEFAULT_BUDGET))
    for budget, chunks in ((1, 67), (chunk_bytes(2, N, top, 0), 34), (chunk_bytes(5, N, top, 0), 14), (chunk_bytes(67, N, top, sum(counts)), 1),
                           (chunk_bytes(67, N, top, sum(counts)) - 1, 2)):
        plan = chunks_of(counts, N, top, budget)
        assert len(plan) == chunks, (budget, plan)
        bctx.set_index_batch_budget(budget)
        assert bctx.index_batch_budget == budget
        for device in (False, True):
            got = _run_batch(bctx, queries, top, device=device)
            assert bctx.index_batch_chunks == chunks, (budget, device, bctx.index_batch_chunks)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), (budget, device)
        dot, score, nq2 = bctx.index_scores()
        assert nq2 == refs[-1][4] and np.array_equal(dot, refs[-1][2]) and np.array_equal(_bits(score), _bits(refs[-1][3])), budget
    assert chunks_of(counts, N, top, chunk_bytes(5, N, top, 0)) == [5] * 13 + [2]
    bctx.set_index_batch_budget(0)
    assert bctx.index_batch_budget == DEFAULT_BUDGET


@pytest.mark.gpu
def test_batch_ms_are_event_times(bctx):
    images = _collection(65, 33, seed=9)
    bctx.build_index(images, 33)
    queries = _batch_of(8, 33, seed=3, images=images)
    bctx.set_index_batch_budget(1)
    bctx.set_profiling(1)
    try:
        bctx.query_index_batch(queries, 5)
        parts, whole = bctx.index_batch_ms, bctx.index_ms[1]
        print("index_batch_ms (group, score, select) and query_ms of 8 one-query chunks:", parts, whole)
        assert bctx.index_batch_chunks == 8 and all(0.0 < v < 1000.0 for v in parts) and sum(parts) <= whole < 1000.0
    finally:
        bctx.set_profiling(0)
        bctx.set_index_batch_budget(0)
    bctx.query_index_batch(queries, 5)
    assert bctx.index_batch_ms == (0.0, 0.0, 0.0) and bctx.index_ms[1] == 0.0 and bctx.index_batch_chunks == 1


# ---------------------------------------------------------------- the state a batch leaves

@pytest.fixture(scope="module")
def e2e(bctx):
    """the five golden images detected with a vocabulary of 40 rows set: keys and (word, dist2) rows"""
    vocab = V.family("uniform", 40, seed=71)
    imgs = [hesaff_amd.read_pnm(os.path.join(GOLD, n + ".pgm")) for n in E2E_IMAGES]
    plain = bctx.detect_batch(imgs)
    bctx.set_vocabulary(vocab)
    try:
        res = bctx.detect_batch(imgs)
        words = [bctx.words(i) for i in range(len(imgs))]
    finally:
        bctx.set_vocabulary(None)
    assert [len(k) for _, k in res] == E2E_KEYS and [len(w) for w in words] == E2E_KEYS
    return imgs, plain, res, words, vocab


@pytest.mark.gpu
def test_state_after_a_batch(bctx, e2e, tmp_path):
    """a single query after a batch equals the same query before it; a batch after add_to_index equals singles on the grown index;
    save_index after a batch writes what it wrote before, and the file loads to an index that answers the same; detection with the
    batch scratch alive is byte-equal to detection without"""
    imgs, plain, res, words, vocab = e2e
    N, K = 65, 33
    images = _collection(N, K, seed=41)
    queries = _batch_of(9, K, seed=42, images=images)
    bctx.build_index(images, K)
    before_file, after_file = str(tmp_path / "before.index"), str(tmp_path / "after.index")
    bctx.save_index(before_file)
    one = bctx.query_index(queries[1], 5)
    one_state = bctx.index_scores()
    bctx.set_index_batch_budget(chunk_bytes(4, N, 5, 0))
    first = _check_batch(bctx, queries, 5, "before the add", refs=[R.query(R.build(images, K), q, N) for q in queries], n_images=N)
    assert bctx.index_batch_chunks > 1
    again = bctx.query_index(queries[1], 5)
    assert again[0].tobytes() == one[0].tobytes() and again[1].tobytes() == one[1].tobytes() and _same_scores(bctx.index_scores(), one_state)
    bctx.query_index_batch(queries, 5)
    bctx.save_index(after_file)
    assert open(before_file, "rb").read() == open(after_file, "rb").read()
    # detection with the scratch alive
    det = bctx.detect_batch(imgs)
    for (na, a), (nb, b) in zip(det, plain):
        assert na == nb and a.tobytes() == b.tobytes()
    same = bctx.query_index_batch(queries, 5)
    assert same[0].tobytes() == first[0].tobytes() and same[1].tobytes() == first[1].tobytes()
    # the grown index
    more = _collection(7, K, seed=43)
    bctx.add_to_index(more)
    grown = R.build(images + more, K)
    got = _check_batch(bctx, queries, 70, "after the add", refs=[R.query(grown, q, N + 7) for q in queries], n_images=N + 7)
    assert got[0].shape == (9, 70)
    # the saved file: the index before the add
    bctx.load_index(after_file)
    back = _check_batch(bctx, queries, 5, "after the load", n_images=N)
    assert back[0].tobytes() == first[0].tobytes() and back[1].tobytes() == first[1].tobytes()
    bctx.set_index_batch_budget(0)


# ---------------------------------------------------------------- embedded batches

@pytest.mark.gpu
def test_embedded_batches(bctx):
    """an embedded index at T = 0, 24 and 64, host and device forms, chunked and whole; T = 64 equals the plain batch"""
    N, K = 65, 33
    rng = np.random.RandomState(61)
    images = _collection(N, K, seed=62)
    # signatures near a per-word centre, so that T = 24 keeps some matches and drops others
    centre = rng.randint(0, 1 << 62, K).astype(np.uint64)

    def sigs_of(words):
        flips = np.array([sum(1 << int(b) for b in rng.choice(64, rng.randint(0, 20), replace=False)) for _ in range(len(words))], np.uint64).reshape(len(words))
        return (centre[words] ^ flips).astype(np.uint64)
    isigs = [sigs_of(w) for w in images]
    bctx.build_embedded_index(images, isigs, K)
    ref = R.build(images, K)
    queries = _batch_of(12, K, seed=63, images=images)
    queries[1] = images[1].copy()
    queries[6] = np.full(300, K - 1, np.int32)
    qsigs = [sigs_of(q) for q in queries]
    qsigs[1] = isigs[1].copy()
    plain = _check_batch(bctx, queries, 9, "plain batch on an embedded index", refs=[R.query(ref, q, N) for q in queries], n_images=N)
    for T in (0, 24, 64):
        refs = [E.query(ref, images, isigs, q, g, T, N) for q, g in zip(queries, qsigs)]
        for budget in (0, chunk_bytes(5, N, 9, 0)):
            bctx.set_index_batch_budget(budget)
            what = "T = %d, budget %d" % (T, budget)
            got = _check_batch(bctx, queries, 9, what, refs=refs, n_images=N, sigs=qsigs, T=T)
            assert bctx.index_batch_chunks == (1 if budget == 0 else len(chunks_of([len(q) for q in queries], N, 9, budget)))
            dev = _run_batch(bctx, queries, 9, device=True, sigs=qsigs, T=T)
            assert dev[0].tobytes() == got[0].tobytes() and dev[1].tobytes() == got[1].tobytes(), what
            if T == 64:
                assert got[0].tobytes() == plain[0].tobytes() and got[1].tobytes() == plain[1].tobytes()
    assert refs[1][0][0] == 1   # the indexed image finds itself
    bctx.set_index_batch_budget(0)


# ---------------------------------------------------------------- refusals

@pytest.mark.gpu
def test_refusals_change_nothing(e2e):
    import torch
    imgs, plain, res, words, vocab = e2e
    N, K, top = 65, 33, 6
    images = _collection(N, K, seed=81)
    queries = _batch_of(9, K, seed=82, images=images)
    counts = np.array([len(q) for q in queries], np.int32)
    flat = np.concatenate(queries).astype(np.int32)
    sigs = np.arange(len(flat), dtype=np.uint64)
    with hesaff_amd.HesaffContext(_params(max_batch=2), device=0) as c:
        L, h = c.L, c.h
        out_im = np.full((9, top), 7, np.int32); out_sc = np.full((9, top), 7.0); n = ctypes.c_int(7)
        ip, sp, np_ = out_im.ctypes.data, out_sc.ctypes.data, ctypes.byref(n)
        cp, wp, gp = counts.ctypes.data, flat.ctypes.data, sigs.ctypes.data
        t = torch.from_numpy(flat).cuda(); tg = torch.from_numpy(sigs.view(np.int64)).cuda()
        torch.cuda.synchronize()
        dp, dg = ctypes.c_void_p(t.data_ptr()), ctypes.c_void_p(tg.data_ptr())
        host, dev, host_e, dev_e = L.hesaff_index_query_batch, L.hesaff_index_query_batch_device, L.hesaff_index_query_batch_embedded, L.hesaff_index_query_batch_embedded_device
        # no index
        assert host(h, 9, cp, wp, 1, top, ip, sp, np_) == ARG and dev(h, 9, cp, dp, 1, top, ip, sp, np_) == ARG
        # the budget is a context setting: it needs no index
        c.set_index_batch_budget(12345)
        assert c.index_batch_budget == 12345
        c.set_index_batch_budget(chunk_bytes(2, N, top, 0))
        assert L.hesaff_index_set_batch_budget(None, 1) == ARG and L.hesaff_index_get_batch_budget(h, None) == ARG
        c.build_index(images, K)
        want = c.query_index_batch(queries, top)
        assert c.index_batch_chunks > 1
        last = c.query_index(queries[1], top)
        state = c.index_scores()
        assert state[2] > 0 and state[0].any()   # (a query that scores: a cleared dot would show)

        def unchanged(what):
            assert (out_im == 7).all() and (out_sc == 7.0).all() and n.value == 7, what
            assert _same_scores(c.index_scores(), state), what
            got = c.query_index_batch(queries, top)
            assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes(), what
            (nh, keys), = c.detect_batch(imgs[1:2])
            assert nh == plain[1][0] and keys.tobytes() == plain[1][1].tobytes(), what
            again = c.query_index(queries[1], top)
            assert again[0].tobytes() == last[0].tobytes() and again[1].tobytes() == last[1].tobytes() and _same_scores(c.index_scores(), state), what
        unchanged("before")
        # required pointers
        assert host(None, 9, cp, wp, 1, top, ip, sp, np_) == ARG and dev(None, 9, cp, dp, 1, top, ip, sp, np_) == ARG
        for call, src in ((host, wp), (dev, dp)):
            assert call(h, 9, None, src, 1, top, ip, sp, np_) == ARG and call(h, 9, cp, None, 1, top, ip, sp, np_) == ARG
            assert call(h, 9, cp, src, 1, top, None, sp, np_) == ARG and call(h, 9, cp, src, 1, top, ip, None, np_) == ARG
            assert call(h, 9, cp, src, 1, top, ip, sp, None) == ARG
        unchanged("required pointers")
        # Q, a count, the total, top, word_stride
        big = np.zeros((1 << 16) + 1, np.int32)
        for call, src in ((host, wp), (dev, dp)):
            for nq in (0, -1, (1 << 16) + 1):
                assert call(h, nq, big.ctypes.data, src, 1, top, ip, sp, np_) == ARG, nq
            for bad in (-1, (1 << 18) + 1):
                b = counts.copy(); b[8] = bad
                assert call(h, 9, b.ctypes.data, src, 1, top, ip, sp, np_) == ARG, bad
            too_many = np.full(1025, 1 << 18, np.int32)   # 2^28 + 2^18 words: refused before a word is read
            assert call(h, 1025, too_many.ctypes.data, src, 1, top, ip, sp, np_) == ARG
            for bad_top in (0, -1, 1025):
                assert call(h, 9, cp, src, 1, bad_top, ip, sp, np_) == ARG, bad_top
            for stride in (0, 3, -1):
                assert call(h, 9, cp, src, stride, top, ip, sp, np_) == ARG, stride
        assert dev(h, 9, cp, ctypes.c_void_p(t.data_ptr() + 2), 1, top, ip, sp, np_) == ARG
        unchanged("bounds, stride and alignment")
        # a word outside 0 .. K - 1 in the last query of a multi-chunk batch
        for w in (-1, K, 1 << 30):
            bad = flat.copy(); bad[-1] = w
            assert counts[-1] == 0 and counts[-2] > 0   # (the batch ends with a query of 0 words: the word is the last query's that has any)
            tb = torch.from_numpy(bad).cuda()
            torch.cuda.synchronize()
            assert host(h, 9, cp, bad.ctypes.data, 1, top, ip, sp, np_) == ARG and dev(h, 9, cp, ctypes.c_void_p(tb.data_ptr()), 1, top, ip, sp, np_) == ARG, w
            tail = np.array([len(queries[7]), 1], np.int32); tw = np.concatenate([queries[7], [w]]).astype(np.int32)
            tb = torch.from_numpy(tw).cuda()
            torch.cuda.synchronize()
            assert host(h, 2, tail.ctypes.data, tw.ctypes.data, 1, top, ip, sp, np_) == ARG and dev(h, 2, tail.ctypes.data, ctypes.c_void_p(tb.data_ptr()), 1, top, ip, sp, np_) == ARG, w
        unchanged("a word outside the vocabulary")
        # the embedded forms on a plain index
        assert host_e(h, 9, cp, wp, 1, gp, 8, top, ip, sp, np_) == ARG and dev_e(h, 9, cp, dp, 1, dg, 8, top, ip, sp, np_) == ARG
        unchanged("embedded forms on a plain index")
        for bad in (np.zeros(3, np.int64), np.zeros((3, 3), np.int32)):
            with pytest.raises(ValueError):
                c.query_index_batch([bad], 3)
        with pytest.raises(ValueError):
            c.query_index_batch([queries[1], _rows(queries[2], 2)], 3)
        # an embedded index: hamming outside 0 .. 64, missing or misaligned signatures
        isigs = [np.arange(len(w), dtype=np.uint64) for w in images]
        c.build_embedded_index(images, isigs, K)
        qs = [np.arange(len(q), dtype=np.uint64) for q in queries]
        want = c.query_index_batch(queries, top, signatures=qs, hamming=30)
        last = c.query_index(queries[1], top)
        state = c.index_scores()
        for T in (-1, 65):
            assert host_e(h, 9, cp, wp, 1, gp, T, top, ip, sp, np_) == ARG and dev_e(h, 9, cp, dp, 1, dg, T, top, ip, sp, np_) == ARG, T
        assert host_e(h, 9, cp, wp, 1, None, 8, top, ip, sp, np_) == ARG and dev_e(h, 9, cp, dp, 1, None, 8, top, ip, sp, np_) == ARG
        assert dev_e(h, 9, cp, dp, 1, ctypes.c_void_p(tg.data_ptr() + 4), 8, top, ip, sp, np_) == ARG
        with pytest.raises(ValueError):
            c.query_index_batch(queries, top, signatures=qs[:-1], hamming=8)
        with pytest.raises(ValueError):
            c.query_index_batch(queries, top, signatures=[g[:-1] if len(g) else g for g in qs], hamming=8)
        with pytest.raises(ValueError):
            c.query_index_batch(queries, top, signatures=qs)
        assert (out_im == 7).all() and (out_sc == 7.0).all() and n.value == 7
        assert _same_scores(c.index_scores(), state)
        got = c.query_index_batch(queries, top, signatures=qs, hamming=30)
        assert got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()
        # clearing: the batch is refused again, the budget stays
        c.clear_index()
        assert host(h, 9, cp, wp, 1, top, ip, sp, np_) == ARG and c.index_batch_budget == chunk_bytes(2, N, top, 0)
        ms = ctypes.c_float(7)
        assert L.hesaff_get_index_batch_ms(h, None, ctypes.byref(ms), ctypes.byref(ms)) == ARG and L.hesaff_get_index_batch_ms(None, ctypes.byref(ms), ctypes.byref(ms), ctypes.byref(ms)) == ARG
        assert ms.value == 7.0


# ---------------------------------------------------------------- end to end

def _words_files(bctx, e2e, tmp_path):
    imgs, plain, res, words, vocab = e2e
    paths = []
    for j, ((_, keys), w) in enumerate(zip(res, words)):
        paths.append(str(tmp_path / ("%d_%s.pgm.hesaff.words" % (j, E2E_IMAGES[j]))))
        hesaff_amd.write_words(paths[-1], keys, w, bctx.params.mrSize, 40)
    lst = tmp_path / "list.txt"
    lst.write_text("\n".join(paths) + "\n")
    return paths, str(lst)


@pytest.mark.gpu
def test_end_to_end_cli_queries(bctx, e2e, tmp_path):
    """hesaff --search list --queries list over the words files of the five golden images: per query a line "# <path>" and then
    exactly the lines --query prints for that file, with and without --verify, from a list and from a saved index"""
    paths, lst = _words_files(bctx, e2e, tmp_path)
    index_file = str(tmp_path / "five.index")
    r = subprocess.run([EXE, "--search", lst, "--save-index", index_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    # (every run is a process that opens the device: one pair of option sets, one source each)
    for extra, source in ((["--top", "2"], ["--search", lst]), (["--verify", "--top", "3", "--tolerance", "4", "--pairs", "2"], ["--index", index_file])):
        singles = []
        for p in paths:
            r = subprocess.run([EXE, "--search", lst, "--query", p] + extra, capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            singles.append(r.stdout)
        want = "".join("# %s\n%s" % (p, s) for p, s in zip(paths, singles))
        r = subprocess.run([EXE] + source + ["--queries", lst] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert r.stdout == want, (extra, source)
        assert want.count("# ") == 5 and all(len(s.strip().split("\n")) == int(extra[extra.index("--top") + 1]) for s in singles)
    assert all(len(l.split("\t")) == 4 for l in singles[0].strip().split("\n"))   # the verified list carries its inlier counts


@pytest.mark.gpu
def test_end_to_end_cpp_members(bctx, e2e, tmp_path):
    """tests/native/index_batch_members.cpp: queryIndexBatch through hesaff.hpp returns per query what queryIndex returns"""
    if shutil.which("g++") is None:
        pytest.skip("g++ not available")
    imgs, plain, res, words, vocab = e2e
    exe = str(tmp_path / "index_batch_members")
    lib_dir = os.path.dirname(hesaff_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "native", "index_batch_members.cpp"), "-L" + lib_dir,
                           "-lhesaff_amd", "-Wl,-rpath," + lib_dir])
    vfile = str(tmp_path / "vocab.bin")
    hesaff_amd.write_vocabulary(vfile, vocab)
    r = subprocess.run([exe, vfile, "4"] + [os.path.join(GOLD, n + ".pgm") for n in E2E_IMAGES], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    ref = R.build([w[:, 0] for w in words], 40)
    want = []
    for q, w in enumerate(words):
        im, sc = R.query(ref, w[:, 0], 4)[:2]
        want += ["B %d %d %d %.17g" % (q, j + 1, i, s) for j, (i, s) in enumerate(zip(im, sc))]
    assert r.stdout.strip().split("\n") == want + ["S equal", "E equal", "C refused"]
