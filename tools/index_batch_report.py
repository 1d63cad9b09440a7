#!/usr/bin/env python3
"""What a batch of index queries (hesaff_index_query_batch_device, kernels_index_batch.h) costs beside a loop of single calls
(hesaff_index_query_device) over the same queries on the same index, and what the batch budget does to it.

One process, one context at profiling level 1.  Two indexes, those of tools/index_report.py:
  synthetic   `--images` images of `--keys` Zipf-distributed words over K = `--vocabulary` words, generated and indexed on the device;
  dense       the (word, dist2) rows of `--batch` dense 3840 x 2160 band-noise images under a vocabulary sampled from their own
              descriptors, indexed in place.
Per index and per Q of `--sizes` (the dense index: every Q up to its images), the same Q queries - the words of Q consecutive indexed
images, where they lie on the device - go through the loop of single calls (A) and through one batch call (B), alternated A B A B ...
`--rounds` times in this one job; the wall time of each pass is taken around the calls, results included.  Reported: queries per
second of both (median over the rounds, and the spread), the batch's three parts (HIP events, summed over its chunks) and its whole
event time, the chunk count, and whether every ranked row of the batch equals the single call's, byte for byte.  Then the largest Q
again at every budget of `--budgets` (MiB).  Exit status 1 when a row differs.

    python tools/index_batch_report.py [--images 100000] [--keys 2000] [--vocabulary 65536] [--batch 32] [--sizes 1,16,256,4096]
                                       [--budgets 64,1024,4096] [--top 100] [--rounds 2] [--out report.json]
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

from index_report import spread, zipf_words   # noqa: E402


def single_loop(ctx, base, stride, starts, counts, first, Q, top):
    t0 = time.perf_counter()
    rows = [ctx.query_index_device(base + int(starts[first + q]) * 4 * stride, int(counts[first + q]), stride, top) for q in range(Q)]
    wall = time.perf_counter() - t0
    return wall, np.stack([r[0] for r in rows]), np.stack([r[1] for r in rows])


def batch_call(ctx, base, stride, starts, counts, first, Q, top):
    t0 = time.perf_counter()
    im, sc = ctx.query_index_batch_device(base + int(starts[first]) * 4 * stride, counts[first:first + Q], stride, top)
    wall = time.perf_counter() - t0
    return wall, im, sc, {"parts_ms": ctx.index_batch_ms, "event_ms": ctx.index_ms[1], "chunks": ctx.index_batch_chunks}


def compare(ctx, name, base, stride, counts, sizes, budgets_mib, top, rounds, seed):
    counts = np.asarray(counts, np.int32)
    starts = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    N = len(counts)
    info = ctx.index_info
    out = {"index": name, "images": int(info[0]), "vocabulary_size": int(info[1]), "keys": int(info[2]), "postings": int(info[3]), "top": top, "sizes": [], "budgets": []}
    rng = np.random.RandomState(seed)
    ctx.set_index_batch_budget(0)
    first = 0
    for Q in [q for q in sizes if q <= N]:
        first = int(rng.randint(0, N - Q + 1))
        single_loop(ctx, base, stride, starts, counts, first, min(Q, 4), top)     # warm-up of both routes
        batch_call(ctx, base, stride, starts, counts, first, Q, top)               # (and the scratch of this Q is allocated)
        a_wall, b_wall, parts, differ = [], [], None, 0
        for _ in range(rounds):
            wa, a_im, a_sc = single_loop(ctx, base, stride, starts, counts, first, Q, top)
            wb, b_im, b_sc, parts = batch_call(ctx, base, stride, starts, counts, first, Q, top)
            a_wall.append(wa); b_wall.append(wb)
            differ += int((a_im.tobytes() != b_im.tobytes()) or (a_sc.tobytes() != b_sc.tobytes()))
        out["sizes"].append({"queries": Q, "words": int(starts[first + Q] - starts[first]), "single_loop_queries_per_s": spread([Q / w for w in a_wall]),
                             "batch_queries_per_s": spread([Q / w for w in b_wall]), "batch_over_loop": float(np.median(a_wall) / np.median(b_wall)),
                             "batch_group_score_select_ms": list(parts["parts_ms"]), "batch_event_ms": parts["event_ms"], "chunks": parts["chunks"],
                             "passes_where_a_row_differs": differ})
    Q = max(q for q in sizes if q <= N)
    _, want_im, want_sc = single_loop(ctx, base, stride, starts, counts, first, Q, top)
    for mib in budgets_mib:
        ctx.set_index_batch_budget(mib << 20)
        batch_call(ctx, base, stride, starts, counts, first, Q, top)   # (allocates the scratch of this budget)
        walls, parts, differ = [], None, 0
        for _ in range(rounds):
            w, im, sc, parts = batch_call(ctx, base, stride, starts, counts, first, Q, top)
            walls.append(w)
            differ += int((im.tobytes() != want_im.tobytes()) or (sc.tobytes() != want_sc.tobytes()))
        out["budgets"].append({"budget_mib": mib, "queries": Q, "batch_queries_per_s": spread([Q / w for w in walls]), "batch_group_score_select_ms": list(parts["parts_ms"]),
                               "batch_event_ms": parts["event_ms"], "chunks": parts["chunks"], "passes_where_a_row_differs": differ})
    ctx.set_index_batch_budget(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100000)
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--vocabulary", type=int, default=65536)
    ap.add_argument("--batch", type=int, default=32, help="dense UHD images of the second index (0: skip it)")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--dense-words", type=int, default=65536)
    ap.add_argument("--sizes", default="1,16,256,4096")
    ap.add_argument("--budgets", default="64,1024,4096", help="MiB")
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    sizes = [int(s) for s in a.sizes.split(",") if s]
    budgets = [int(s) for s in a.budgets.split(",") if s]
    p = hesaff_amd.default_params()
    p.max_batch = max(a.batch, 1)
    report = {"library": hesaff_amd.lib_path(), "indexes": []}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        if a.images > 0:
            words = zipf_words(torch, a.images * a.keys, a.vocabulary, seed=a.vocabulary)
            torch.cuda.synchronize()
            counts = np.full(a.images, a.keys, np.int32)
            ctx.build_index_device(words.data_ptr(), counts, 1, a.vocabulary)
            report["indexes"].append(compare(ctx, "synthetic: %d images of %d Zipf words" % (a.images, a.keys), words.data_ptr(), 1, counts, sizes, budgets, a.top,
                                             a.rounds, seed=1))
            ctx.clear_index()
            del words
        if a.batch > 0:
            from vocabulary_report import device_copy
            imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
            torch.cuda.synchronize()
            ch, cd, dkeys, n_keys = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
            keys = device_copy(torch, dkeys, n_keys * 164).view(n_keys, 164)
            K = min(a.dense_words, n_keys)
            pick = torch.tensor([r * n_keys // K for r in range(K)], device="cuda")
            ctx.set_vocabulary(keys[pick][:, 36:].contiguous().cpu().numpy())
            del keys
            ch, cd, dkeys, n_keys = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
            ptr, rows = ctx.words_device()
            rows_t = device_copy(torch, ptr, rows * 8)   # a copy: the context's rows change with its next detecting call
            if max(cd) > (1 << 18):
                report["indexes"].append({"index": "dense", "skipped": "an image has %d keys, more than 2^18" % max(cd)})
            else:
                ctx.build_index_device(rows_t.data_ptr(), cd, 2, K)
                dense_sizes = sorted({q for q in sizes if q <= a.batch} | {a.batch})
                report["indexes"].append(compare(ctx, "dense: the words of %d %dx%d band-noise images" % (a.batch, a.width, a.height), rows_t.data_ptr(), 2, cd,
                                                 dense_sizes, budgets, min(a.top, a.batch), a.rounds, seed=2))
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    bad = [r for ix in report["indexes"] for r in ix.get("sizes", []) + ix.get("budgets", []) if r["passes_where_a_row_differs"]]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
