#!/usr/bin/env python3
"""What spatial verification (hesaff_verify_matches_device, kernels_verify.h) costs, and how it compares with the same computation
written in torch.

One process, one context at profiling level 1.  Two workloads, each for every shortlist length of `--candidates`:
  synthetic   a query of 4096 keys with distinct words; every candidate holds a moved, jittered copy of them and `--distractors`
              keys of other words, so found = M = 4096 per candidate: the hypothesis kernel at its cap;
  dense       the words files of `--batch` dense 3840 x 2160 band-noise images under a vocabulary of `--dense-words` rows sampled
              from their own descriptors (the first `--max-keys` keys of each image); the query is image 0, the shortlist the images
              in turn: M is what such images give.
Per workload and shortlist length: hesaff_get_verify_ms of `--rounds` calls - pairs_ms (grouping the query, counting tf, building
the pairs) and hypotheses_ms (all hypotheses, the result, the ranking) - alternated with the torch route.

The torch route does the same on the same rows on the same device for the first `--torch-candidates` candidates, one after the
other: frames and liveness, tfq / tf by bincount, the pairs of words with tfq = tf = 1 (P = 1) in j order, then for all hypotheses
at once the [M, M] error matrix in float32 elementwise operations (no contraction: every operation is its own kernel) and the
count of inliers.  Its inliers, best hypothesis and pair counts must equal the library's: the tool counts the candidates that differ
and exits with status 1 when there is one.  Its times are per candidate; the library's are divided by the shortlist length beside them.

    python tools/verify_report.py [--candidates 100,1000] [--batch 8] [--rounds 3] [--tolerance 6] [--out report.json]
"""
import argparse
import json
import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_frames(torch, rows):
    """rows: float32 [n, 6] (the word's bits in column 5) -> (x, y, p, q, r, live)"""
    x, y, a, b, c = (rows[:, k] for k in range(5))
    r = torch.sqrt(c); q = b / r; t = a - q * q; p = torch.sqrt(t)
    lo, hi = 2.0 ** -20, 2.0 ** 20
    live = (c > 0) & (t > 0) & (p >= lo) & (p <= hi) & (r >= lo) & (r <= hi) & (a <= 2.0 ** 40) & (x.abs() <= hi) & (y.abs() <= hi)
    return x, y, p, q, r, live


def torch_candidate(torch, qrows, qwords, crows, cwords, K, tol):
    """one candidate at P = 1 -> (inliers, used, found, best h), everything on the device until the four numbers"""
    xq, yq, pq, qq, rq, lq = torch_frames(torch, qrows)
    xd, yd, pd, qd, rd, lc = torch_frames(torch, crows)
    tfq = torch.bincount(qwords[lq], minlength=K)
    tfc = torch.bincount(cwords[lc], minlength=K)
    where = torch.full((K,), -1, dtype=torch.long, device="cuda")
    live_q = torch.nonzero(lq)[:, 0]
    where[qwords[live_q]] = live_q                      # (read only where tfq = 1)
    j = torch.nonzero(lc & (tfq[cwords] == 1) & (tfc[cwords] == 1))[:, 0]
    found = int(j.numel())
    j = j[:4096]
    i = where[cwords[j]]
    if found == 0:
        return 0, 0, 0, -1
    L11 = pq[i] / pd[j]; L22 = rq[i] / rd[j]; L21 = (qq[i] - qd[j] * L11) / rd[j]
    dx = xq[i][None, :] - xq[i][:, None]; dy = yq[i][None, :] - yq[i][:, None]
    u = L11[:, None] * dx; v = L21[:, None] * dx + L22[:, None] * dy
    ex = (xd[j][:, None] + u) - xd[j][None, :]; ey = (yd[j][:, None] + v) - yd[j][None, :]
    e2 = ex * ex + ey * ey
    tol2 = torch.tensor(tol, dtype=torch.float32, device="cuda") * torch.tensor(tol, dtype=torch.float32, device="cuda")
    inl = (e2 <= tol2).sum(dim=1)
    top = int(inl.max().item())
    best = int(torch.nonzero(inl == top)[0, 0].item())   # the lowest h that attains it
    return top, int(j.numel()), found, best


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def run(torch, ctx, name, query, cands, K, tol, rounds, torch_candidates):
    """query: structured rows (numpy); cands: a list of them -> the report of one shortlist"""
    counts = np.array([len(c) for c in cands], np.int32)
    flat = np.concatenate(cands)
    tq = torch.from_numpy(query.view(np.uint8).copy()).cuda()
    tc = torch.from_numpy(flat.view(np.uint8)).cuda()
    torch.cuda.synchronize()
    starts = np.concatenate([[0], np.cumsum(counts.astype(np.int64))])
    qf = tq.view(torch.float32).view(-1, 6); qw = tq.view(torch.int32).view(-1, 6)[:, 5].long()
    cf = tc.view(torch.float32).view(-1, 6); cw = tc.view(torch.int32).view(-1, 6)[:, 5].long()
    nt = min(torch_candidates, len(cands))
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def torch_route():
        res = []
        ev[0].record()
        for r in range(nt):
            lo, hi = int(starts[r]), int(starts[r + 1])
            res.append(torch_candidate(torch, qf, qw, cf[lo:hi], cw[lo:hi], K, tol))
        ev[1].record()
        torch.cuda.synchronize()
        return res, ev[0].elapsed_time(ev[1]) / nt
    out, hyp, order = ctx.verify_matches_device(tq.data_ptr(), len(query), tc.data_ptr(), counts, K, tol, 1)   # warm-up of both routes
    torch_route()
    pairs_ms, hyp_ms, torch_ms = [], [], []
    for _ in range(rounds):
        out, hyp, order = ctx.verify_matches_device(tq.data_ptr(), len(query), tc.data_ptr(), counts, K, tol, 1)
        ms = ctx.verify_ms
        pairs_ms.append(ms[0]); hyp_ms.append(ms[1])
        res, per_candidate = torch_route()
        torch_ms.append(per_candidate)
    differ = 0
    for r, (inl, used, found, best) in enumerate(res):
        pr = ctx.verify_pairs(r)
        h = -1 if out[r, 3] < 0 else int(np.nonzero((pr[:, 0] == out[r, 3]) & (pr[:, 1] == out[r, 4]))[0][0])
        differ += 0 if (inl, used, found, best) == (int(out[r, 0]), int(out[r, 1]), int(out[r, 2]), h) else 1
    R = len(cands)
    return {"workload": name, "candidates": R, "query_keys": int(len(query)), "candidate_keys": int(counts.sum()), "vocabulary_size": int(K),
            "used_median": float(np.median(out[:, 1])), "used_max": int(out[:, 1].max()), "inliers_median": float(np.median(out[:, 0])),
            "pairs_ms": spread(pairs_ms), "hypotheses_ms": spread(hyp_ms),
            "pairs_plus_hypotheses_ms_per_candidate": (float(np.median(pairs_ms)) + float(np.median(hyp_ms))) / R,
            "hypothesis_evaluations_per_second": float((out[:, 1].astype(np.float64) ** 2).sum() / (np.median(hyp_ms) * 1e-3)),
            "torch_candidates": nt, "torch_ms_per_candidate": spread(torch_ms), "candidates_where_torch_differs": differ}


def synthetic(rng, R, distractors):
    from hesaff_amd import WORDS_ROW_DTYPE as ROW

    def rows(n, words):
        k = np.zeros(n, ROW)
        p = (0.05 + 0.1 * rng.rand(n)).astype(np.float32); r = (0.05 + 0.1 * rng.rand(n)).astype(np.float32); q = (0.04 * (rng.rand(n) - 0.5)).astype(np.float32)
        k["x"] = (rng.rand(n) * 3000).astype(np.float32); k["y"] = (rng.rand(n) * 2000).astype(np.float32)
        k["a"] = p * p + q * q; k["b"] = q * r; k["c"] = r * r; k["word"] = words
        return k
    K = 4096 + distractors
    query = rows(4096, rng.permutation(4096))
    cands = []
    for _ in range(R):
        c = query.copy()
        c["x"] += (2.0 * rng.randn(4096)).astype(np.float32) + np.float32(11); c["y"] += (2.0 * rng.randn(4096)).astype(np.float32) - np.float32(5)
        c = np.concatenate([c, rows(distractors, 4096 + rng.permutation(distractors))])
        cands.append(c[rng.permutation(len(c))])
    return query, cands, K


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--candidates", default="100,1000")
    ap.add_argument("--distractors", type=int, default=2048)
    ap.add_argument("--batch", type=int, default=8, help="dense UHD images of the second workload (0: skip it)")
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--dense-words", type=int, default=65536)
    ap.add_argument("--max-keys", type=int, default=65536)
    ap.add_argument("--tolerance", type=float, default=6.0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--torch-candidates", type=int, default=16)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = max(a.batch, 1)
    sizes = [int(s) for s in a.candidates.split(",") if s]
    report = {"library": hesaff_amd.lib_path(), "tolerance": a.tolerance, "max_pairs": 1, "workloads": []}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        for R in sizes:
            query, cands, K = synthetic(np.random.RandomState(R), R, a.distractors)
            report["workloads"].append(run(torch, ctx, "synthetic: M = 4096", query, cands, K, a.tolerance, a.rounds, a.torch_candidates))
        if a.batch > 0:
            from vocabulary_report import device_copy
            imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
            torch.cuda.synchronize()
            ch, cd, dkeys, n_keys = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
            keys = device_copy(torch, dkeys, n_keys * 164).view(n_keys, 164)
            K = min(a.dense_words, n_keys)
            pick = torch.tensor([r * n_keys // K for r in range(K)], device="cuda")
            ctx.set_vocabulary(keys[pick][:, 36:].contiguous().cpu().numpy())
            ch, cd, dkeys, n_keys = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
            ptr, n_rows = ctx.words_device()
            h_keys = device_copy(torch, dkeys, n_keys * 164).cpu().numpy().view(hesaff_amd.KEYPOINT_DTYPE)
            h_words = device_copy(torch, ptr, n_rows * 8).cpu().numpy().view(np.int32).reshape(-1, 2)
            ctx.set_vocabulary(None)
            del imgs, keys
            images, lo = [], 0
            with tempfile.TemporaryDirectory() as d:   # the rows as the library writes them: through a words file
                for i, n in enumerate(cd):
                    path = os.path.join(d, "%d.hesaff.words" % i)
                    m = min(int(n), a.max_keys)
                    hesaff_amd.write_words(path, h_keys[lo:lo + m], h_words[lo:lo + m], p.mrSize, K)
                    images.append(hesaff_amd.read_words(path)[1])
                    lo += int(n)
            for R in sizes:
                cands = [images[r % len(images)] for r in range(R)]
                w = run(torch, ctx, "dense: %d keys at most of each of %d %dx%d band-noise images, %d words" % (a.max_keys, a.batch, a.width, a.height, K),
                        images[0], cands, K, a.tolerance, a.rounds, a.torch_candidates)
                w["keys_per_image"] = [int(n) for n in cd]
                report["workloads"].append(w)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    sys.exit(1 if any(w["candidates_where_torch_differs"] for w in report["workloads"]) else 0)


if __name__ == "__main__":
    main()
