#!/usr/bin/env python3
"""What the image index (hesaff_index_build_device / hesaff_index_query_device, kernels_index.h) costs, and how it compares with the
same scoring written in torch.

One process, one context at profiling level 1.  Two workloads:
  synthetic   `--images` images of `--keys` words each, the words Zipf-distributed (weight 1 / rank) over K words, for every K of
              `--sizes`; generated on the device, indexed where they lie;
  dense       the (word, dist2) rows that hesaff_detect_batch_device leaves on the device for `--batch` dense 3840 x 2160
              band-noise images under a vocabulary of `--dense-words` rows sampled from their own descriptors, indexed in place.
Per workload: the build's HIP-event time (hesaff_get_index_ms; the whole build - the hash step and the list steps are told apart in
a kernel trace of this run, not here), then `--queries` queries, each the words of an indexed image, with the median and the spread
of their HIP-event times and of their wall times (the call, the staging of nothing - the words are on the device - and the copy of
the ranked result).

The torch route scores the same queries from the same postings on the same device: the distinct (image, word) pairs and their tf
from torch.unique over the keys, word-major; per query the postings of its words are gathered, weighted in int64 and summed with
index_add_; the score is the same three binary64 operations; topk gives the cut, and the tie rule of the definition (lower image
first) orders what equals it.  Its ranked images and scores must be identical to the library's: the tool counts the queries that
differ and exits with status 1 when there is one.

    python tools/index_report.py [--images 100000] [--keys 2000] [--sizes 65536,1048576] [--batch 32] [--queries 100] [--top 100] [--out report.json]
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


def zipf_words(torch, total, K, seed):
    """`total` int32 words in 0 .. K - 1 on the device, P(w) proportional to 1 / (w + 1)"""
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    cdf = torch.cumsum(1.0 / torch.arange(1, K + 1, device="cuda", dtype=torch.float64), 0)
    cdf = cdf / cdf[-1]
    out = torch.empty(total, dtype=torch.int32, device="cuda")
    step = 1 << 24
    for lo in range(0, total, step):
        n = min(step, total - lo)
        u = torch.rand(n, generator=g, device="cuda", dtype=torch.float64)
        out[lo:lo + n] = torch.searchsorted(cdf, u).clamp_(max=K - 1).to(torch.int32)
    return out


class TorchIndex:
    """the postings of the same keys, word-major, and the integer tables, all in torch"""

    def __init__(self, torch, words, counts, K, idf, norm2):
        self.torch = torch
        N = len(counts)
        image = torch.repeat_interleave(torch.arange(N, device="cuda"), torch.as_tensor(counts, device="cuda").long())
        key = (words.long() << 20) | image          # word-major: a word's postings are neighbours
        pairs, tf = torch.unique(key, return_counts=True)
        self.p_image = pairs & ((1 << 20) - 1)
        self.p_tf = tf
        df = torch.bincount(pairs >> 20, minlength=K)
        self.offsets = torch.cat([torch.zeros(1, dtype=torch.long, device="cuda"), torch.cumsum(df, 0)])
        self.idf2 = torch.from_numpy(idf.astype(np.int64)).cuda() ** 2
        self.idf = torch.from_numpy(idf.astype(np.int64)).cuda()
        self.norm2 = torch.from_numpy(norm2.astype(np.int64)).cuda().double()   # (below 2^62: int64 holds it)
        self.N, self.K = N, K
        self.df = df

    def query(self, words, top):
        torch = self.torch
        qw, qc = torch.unique(words.long(), return_counts=True)
        nq2 = ((qc * self.idf[qw]) ** 2).sum()
        starts = self.offsets[qw]
        lens = self.offsets[qw + 1] - starts
        total = int(lens.sum().item())
        first = torch.cumsum(lens, 0) - lens
        idx = torch.repeat_interleave(starts - first, lens) + torch.arange(total, device="cuda")
        weight = torch.repeat_interleave(qc * self.idf2[qw], lens) * self.p_tf[idx]
        dot = torch.zeros(self.N, dtype=torch.long, device="cuda").index_add_(0, self.p_image[idx], weight)
        score = torch.where(dot > 0, dot.double() / torch.sqrt(nq2.double() * self.norm2), torch.zeros((), dtype=torch.double, device="cuda"))
        keep = min(top, self.N)
        vals, _ = torch.topk(score, keep)
        cut = vals[-1]
        above = torch.nonzero(score > cut)[:, 0]
        on = torch.nonzero(score == cut)[:, 0][:keep - len(above)]   # (ascending: the lower image first)
        images = torch.cat([above, on])
        order = torch.argsort(-score[images], stable=True)           # (`above` is ascending, so equal scores keep the lower image first)
        images = images[order]
        return images.to(torch.int32), score[images]


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "p10": float(np.percentile(v, 10)), "p90": float(np.percentile(v, 90)), "max": float(v.max())}


def run_workload(torch, ctx, name, words, stride, counts, K, n_queries, top, seed):
    """words: an int32 device tensor ([T] or [T, 2]); -> the workload's report"""
    counts = np.asarray(counts, np.int32)
    starts = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    ctx.build_index_device(words.data_ptr(), counts, stride, K)   # warm-up: the first launch of every kernel
    builds = []
    for _ in range(3):
        t0 = time.perf_counter()
        ctx.build_index_device(words.data_ptr(), counts, stride, K)
        builds.append({"event_ms": ctx.index_ms[0], "wall_ms": (time.perf_counter() - t0) * 1e3})
    info = ctx.index_info
    df, idf, norm2 = ctx.index_tables()
    packed = words if stride == 1 else words[:, 0].contiguous()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ev[0].record()
    ti = TorchIndex(torch, packed, counts, K, idf, norm2)
    ev[1].record()
    torch.cuda.synchronize()
    torch_build_ms = ev[0].elapsed_time(ev[1])
    tables_equal = bool(np.array_equal(ti.df.cpu().numpy().astype(np.uint32), df)) and int(ti.p_tf.numel()) == info[3]
    rng = np.random.RandomState(seed)
    with_keys = np.nonzero(counts > 0)[0]
    picks = with_keys[rng.randint(0, len(with_keys), n_queries)]
    lib_event, lib_wall, torch_ms, differ = [], [], [], 0
    for j, i in enumerate(picks):
        lo, n = int(starts[i]), int(counts[i])
        ptr = words.data_ptr() + lo * 4 * stride
        t0 = time.perf_counter()
        im, sc = ctx.query_index_device(ptr, n, stride, top)
        lib_wall.append((time.perf_counter() - t0) * 1e3)
        lib_event.append(ctx.index_ms[1])
        q = packed[lo:lo + n]
        if j == 0:
            ti.query(q, top)   # warm-up of the torch route
        ev[0].record()
        t_im, t_sc = ti.query(q, top)
        ev[1].record()
        torch.cuda.synchronize()
        torch_ms.append(ev[0].elapsed_time(ev[1]))
        same = np.array_equal(t_im.cpu().numpy(), im) and np.array_equal(t_sc.cpu().numpy().view(np.uint64), sc.view(np.uint64))
        differ += 0 if same else 1
    return {"workload": name, "images": int(info[0]), "vocabulary_size": int(info[1]), "keys": int(info[2]), "postings": int(info[3]),
            "words_with_idf_0": int(((idf == 0) & (df > 0)).sum()), "longest_list": int(df.max()),
            "build_event_ms": spread([b["event_ms"] for b in builds]), "build_wall_ms": spread([b["wall_ms"] for b in builds]),
            "torch_build_ms_unique_and_offsets": torch_build_ms, "torch_postings_equal": tables_equal,
            "queries": n_queries, "top": top, "query_event_ms": spread(lib_event), "query_wall_ms": spread(lib_wall), "torch_query_ms": spread(torch_ms),
            "queries_where_torch_differs": differ}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100000)
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--batch", type=int, default=32, help="dense UHD images of the second workload (0: skip it)")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--dense-words", type=int, default=65536)
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--top", type=int, default=100)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = max(a.batch, 1)
    report = {"library": hesaff_amd.lib_path(), "workloads": []}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        total = a.images * a.keys
        for K in [int(s) for s in a.sizes.split(",") if s]:
            words = zipf_words(torch, total, K, seed=K)
            torch.cuda.synchronize()
            report["workloads"].append(run_workload(torch, ctx, "synthetic: %d images of %d Zipf words" % (a.images, a.keys), words, 1,
                                                    np.full(a.images, a.keys, np.int32), K, a.queries, a.top, seed=K + 1))
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
            rows_t = device_copy(torch, ptr, rows * 8).view(torch.int32).view(rows, 2)   # a copy for the torch route; the library reads the original
            if max(cd) > (1 << 18):
                report["workloads"].append({"workload": "dense", "skipped": "an image has %d keys, more than 2^18" % max(cd)})
            else:
                r = run_workload(torch, ctx, "dense: the words of %d %dx%d band-noise images" % (a.batch, a.width, a.height), rows_t, 2, cd, K,
                                 a.queries, min(a.top, a.batch), seed=7)
                im, sc = ctx.query_index_device(ptr, int(cd[0]), 2, 1)   # and once on the rows where detection left them
                r["in_place_query_of_image_0"] = [int(im[0]), float(sc[0])]
                report["workloads"].append(r)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    bad = [w for w in report["workloads"] if w.get("queries_where_torch_differs") or w.get("torch_postings_equal") is False]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
