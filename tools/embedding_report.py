#!/usr/bin/env python3
"""What Hamming embedding (hesaff_set_embedding, hesaff_train_embedding*, hesaff_index_query_embedded*, kernels_embed.h) costs, and
what the signatures tell apart.

One process, one context at profiling level 1.  Four parts:
  signatures   `--batch` dense `--width` x `--height` band-noise images through hesaff_detect_batch_device under a vocabulary of K rows
               sampled from their own descriptors, for every K of `--sizes`, with the embedding trained on the same keys: the HIP-event
               time of the signature launch (hesaff_get_embedding_ms) beside that of the word assignment (hesaff_get_assign_ms);
  training     hesaff_train_embedding_device on the keys and words where detection left them: projection, grouping and median steps;
  query        an embedded index over the batch's images, built in place; `--queries` queries, each the keys of an indexed image, at
               every T of `--hamming`, ALTERNATED with the plain query of the same index, so that both see the same device state: the
               median and spread of the HIP-event times (hesaff_get_index_ms);
  histogram    the synthetic viewpoint sequence of tools/repeatability.py (a band-noise image and copies warped by a camera rotation):
               keys of the first image and of a warped copy that fall into the same word - `--histogram-words` words, vocabulary and
               thresholds trained on the sequence itself - are split into true correspondences (the centre of one maps onto the other's
               within `--radius` pixels) and the other same-word pairs, with the histogram of their Hamming distances.

    python tools/embedding_report.py [--batch 32] [--sizes 4096,65536] [--hamming 16,24,64] [--queries 50] [--top 100] [--out report.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "max": float(v.max())}


def popcount64(x):
    x = np.asarray(x, np.uint64)
    return np.unpackbits(x.view(np.uint8).reshape(-1, 8), axis=1).sum(axis=1)


def dense_part(torch, hesaff_amd, ctx, a, K, report):
    from hesaff_amd import synth
    from vocabulary_report import device_copy
    imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
    torch.cuda.synchronize()
    ctx.set_vocabulary(None)
    ch, cd, dkeys, n_keys = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
    keys = device_copy(torch, dkeys, n_keys * 164).view(n_keys, 164)
    K = min(K, n_keys)
    pick = torch.tensor([r * n_keys // K for r in range(K)], device="cuda")
    ctx.set_vocabulary(keys[pick][:, 36:].contiguous().cpu().numpy())
    del keys
    ch, cd, dkeys, n_keys = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
    wptr, rows = ctx.words_device()
    P = hesaff_amd.embedding_projection(a.seed)
    # training on the keys and words where they lie (warm-up, then three timed calls)
    runs = []
    for j in range(4):
        t0 = time.perf_counter()
        tau, counts = ctx.train_embedding_device(dkeys, n_keys, 164, 36, wptr, 2, K, P)
        ms = ctx.embedding_ms
        if j:
            runs.append({"project_ms": ms[1], "group_ms": ms[2], "median_ms": ms[3], "wall_ms": (time.perf_counter() - t0) * 1e3})
    training = {"keys": int(n_keys), "vocabulary_size": int(K), "words_without_keys": int((counts == 0).sum()), "largest_word": int(counts.max()),
                "project_ms": spread([r["project_ms"] for r in runs]), "group_ms": spread([r["group_ms"] for r in runs]),
                "median_ms": spread([r["median_ms"] for r in runs]), "wall_ms": spread([r["wall_ms"] for r in runs])}
    ctx.set_embedding(P, tau)
    assign, embed = [], []
    for j in range(4):
        ch, cd, dkeys, n_keys = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
        if j:
            assign.append(ctx.assign_ms); embed.append(ctx.embedding_ms[0])
    signatures = {"keys": int(n_keys), "vocabulary_size": int(K), "assign_ms": spread(assign), "embed_ms": spread(embed)}
    wptr, rows = ctx.words_device()
    sptr, srows = ctx.signatures_device()
    query = None
    if max(cd) <= (1 << 18):
        ctx.build_embedded_index_device(wptr, sptr, cd, 2, K)
        build_ms = ctx.index_ms[0]
        starts = np.concatenate([[0], np.cumsum(np.asarray(cd, np.int64))])
        rng = np.random.RandomState(7)
        with_keys = np.nonzero(np.asarray(cd) > 0)[0]
        picks = with_keys[rng.randint(0, len(with_keys), a.queries)]
        times = {"plain": []}
        top = min(a.top, a.batch)
        thresholds = [int(t) for t in a.hamming.split(",") if t]
        for T in thresholds:
            times[str(T)] = []
        same_as_plain = 0
        for i in picks:
            lo, n = int(starts[i]), int(cd[i])
            for T in thresholds:   # plain, T, plain, T', ..: the two kinds alternate
                im0, sc0 = ctx.query_index_device(wptr + lo * 8, n, 2, top)
                times["plain"].append(ctx.index_ms[1])
                im, sc = ctx.query_embedded_index_device(wptr + lo * 8, sptr + lo * 8, n, 2, T, top)
                times[str(T)].append(ctx.index_ms[1])
                if T == 64:
                    same_as_plain += int(np.array_equal(im, im0) and sc.tobytes() == sc0.tobytes())
        query = {"images": int(a.batch), "keys": int(n_keys), "vocabulary_size": int(K), "build_event_ms": build_ms, "queries": int(a.queries), "top": int(top),
                 "query_event_ms": {k: spread(v) for k, v in times.items()}}
        if 64 in thresholds:
            query["queries_where_T64_equals_plain"] = same_as_plain
        ctx.clear_index()
    report["signatures"].append(signatures)
    report["training"].append(training)
    if query:
        report["query"].append(query)


def histogram_part(hesaff_amd, ctx, a, K):
    import repeatability as rp
    from hesaff_amd.synth import band_noise_image
    width, height, angles = 800, 640, (10, 20, 30, 40, 50)
    base = band_noise_image(height, width, 1234)
    imgs, Hs = [base], [np.eye(3)]
    for ang in angles:
        H = rp.viewpoint_homography(width, height, ang)
        imgs.append(rp.warp_image(base, H, (width, height))); Hs.append(H)
    ctx.set_vocabulary(None)
    res = ctx.detect_batch(imgs)
    desc = np.ascontiguousarray(np.concatenate([k["desc"] for _, k in res]))
    K = min(K, len(desc))
    vocab = ctx.train_vocabulary(desc, K, 10)[0]
    ctx.set_vocabulary(vocab)
    words = ctx.assign_words(desc)
    P = hesaff_amd.embedding_projection(a.seed)
    tau, counts = ctx.train_embedding(desc, words, P)
    ctx.set_embedding(P, tau)
    res = ctx.detect_batch(imgs)
    out = []
    k0 = res[0][1]
    w0, g0 = ctx.words(0)[:, 0], ctx.signatures(0)
    for j, ang in enumerate(angles, start=1):
        kj = res[j][1]
        wj, gj = ctx.words(j)[:, 0], ctx.signatures(j)
        p = rp.project(Hs[j], np.c_[k0["x"].astype(np.float64), k0["y"].astype(np.float64)])
        true_h = np.zeros(65, np.int64); other_h = np.zeros(65, np.int64)
        order = np.argsort(wj, kind="stable")
        sw = wj[order]
        lo = np.searchsorted(sw, w0, "left"); hi = np.searchsorted(sw, w0, "right")
        for i in np.nonzero(hi > lo)[0]:
            cand = order[lo[i]:hi[i]]
            d2 = (kj["x"][cand].astype(np.float64) - p[i, 0]) ** 2 + (kj["y"][cand].astype(np.float64) - p[i, 1]) ** 2
            ham = popcount64(gj[cand] ^ g0[i]).astype(np.int64)
            near = d2 <= a.radius * a.radius
            true_h += np.bincount(ham[near], minlength=65)
            other_h += np.bincount(ham[~near], minlength=65)
        out.append({"viewpoint_deg": ang, "keys": [int(len(k0)), int(len(kj))], "true_pairs": int(true_h.sum()), "other_same_word_pairs": int(other_h.sum()),
                    "true_hamming_histogram": true_h.tolist(), "other_hamming_histogram": other_h.tolist(),
                    "true_within": {str(T): int(true_h[:T + 1].sum()) for T in (16, 24, 32, 64)},
                    "other_within": {str(T): int(other_h[:T + 1].sum()) for T in (16, 24, 32, 64)}})
    ctx.set_vocabulary(None)
    return {"data": "synthetic: band-noise %dx%d image and copies warped by a camera rotation about the vertical axis" % (width, height),
            "vocabulary_size": int(K), "radius_px": a.radius, "pairs": out}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32, help="dense images of the first three parts (0: skip them)")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--hamming", default="16,24,64")
    ap.add_argument("--queries", type=int, default=50)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--radius", type=float, default=2.0)
    ap.add_argument("--histogram-words", type=int, default=4096, help="vocabulary size of the histogram part (0: skip it)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import hesaff_amd
    p = hesaff_amd.default_params()
    p.max_batch = max(a.batch, 8)
    report = {"library": hesaff_amd.lib_path(), "signatures": [], "training": [], "query": []}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        if a.batch > 0:
            for K in [int(s) for s in a.sizes.split(",") if s]:
                dense_part(torch, hesaff_amd, ctx, a, K, report)
        if a.histogram_words > 0:
            report["histogram"] = histogram_part(hesaff_amd, ctx, a, a.histogram_words)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    bad = [q for q in report["query"] if "queries_where_T64_equals_plain" in q and q["queries_where_T64_equals_plain"] != q["queries"]]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
