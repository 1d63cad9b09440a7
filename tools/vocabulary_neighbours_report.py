#!/usr/bin/env python3
"""What the R nearest words per key (hesaff_set_vocabulary_neighbours, k_assign_neighbours in kernels_neighbours.h) cost on the bench's
dense image family, how often the kernel leaves its hot loop, and what the mode buys a query.

One process, one context at profiling level 1.  The keys of B dense 3840 x 2160 band-noise images (hesaff_detect_batch_device) are
copied once into a packed [n, 128] tensor; a vocabulary of K rows is K of those keys spread evenly (row r = key r n // K).

timing      per K of `--sizes` and R of `--ranks`: hesaff_assign_words_device over all keys (R = 1: k_assign_words; R > 1:
            k_assign_neighbours, which writes the words and the neighbours), the counts alternating `--rounds` times after a warm-up of
            each; assign_ms medians, their ratio to R = 1, and to R x (R = 1) - the cost of finding rank after rank by sweeps, the
            scheme the single pass replaces.  Rank 0 must equal the R = 1 rows: the tool asserts it.
slow path   the share of (wavefront, tile) pairs in which at least one lane's hot compare, score <= the list's last score, fires.  Not
            counted on the device - the shipped kernel carries no counter: derived on the host, exactly, for `--waves` wavefronts of 64
            consecutive keys, from the scores, the C/D map (a lane sees rows 8 g + 4 h .. + 3 of a tile, g = 0..3, in that order) and
            the list capacity the launcher picks for R (2, 4, 8).
recall      `--perturbed` keys drawn evenly, `--bytes` of their 128 bytes moved by up to +-`--noise` (fixed seed): the share whose
            unperturbed word is among the perturbed key's R neighbours.
query       an index of the B images' words (and signatures, thresholds trained on the keys); the query is `--query-keys` perturbed
            keys of image 0 under their R nearest words each, R = 1 and R = 3, plain and with --hamming T: rank and score of image 0.

    python tools/vocabulary_neighbours_report.py [--batch 32] [--rounds 3] [--ranks 1,2,4,8] [--sizes 4096,65536,1048576] [--out report.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median(v):
    return float(np.median(v))


def slow_path_share(desc, vocab, cap):
    """desc uint8 [64 w, 128], vocab uint8 [K, 128] -> (share of (wave, tile) pairs with a firing compare, fires per lane list and
    tile pair): the lists of k_assign_neighbours<cap> replayed on the host.  Only scores matter for the compare; pad rows never fire
    once a list is full and are counted like the device meets them (score 2^30)."""
    d = (desc ^ 0x80).view(np.int8).astype(np.int32)
    w = (vocab ^ 0x80).view(np.int8).astype(np.int32)
    K = len(w)
    tiles = (K + 31) // 32
    norm = np.full(tiles * 32, 1 << 30, np.int64)
    norm[:K] = (w * w).sum(axis=1)
    wp = np.zeros((tiles * 32, 128), np.int32)
    wp[:K] = w
    waves = len(d) // 64
    entered = fires = 0
    for v in range(waves):
        score = norm[None, :] - 2 * (d[64 * v:64 * v + 64] @ wp.T).astype(np.int64)      # [64, tiles * 32]
        # a list belongs to (key, half): its rows of a tile in arrival order are 8 g + 4 h + q
        s = score.reshape(64, tiles, 4, 2, 4).transpose(0, 3, 1, 2, 4).reshape(128, tiles, 16)
        worst = np.full((128, cap), np.iinfo(np.int64).max, np.int64)                    # sorted ascending
        for t in range(tiles):
            any_fire = False
            for e in range(16):
                x = s[:, t, e]
                fire = x <= worst[:, -1]
                if fire.any():
                    any_fire = True
                    fires += int(fire.sum())
                    # an equal score is inserted only where its row is lower, which it never is inside a lane (rows ascend): the
                    # compare fires all the same, which is what is counted
                    ins = x < worst[:, -1]
                    if ins.any():
                        merged = np.sort(np.concatenate([worst[ins], x[ins, None]], axis=1), axis=1)[:, :cap]
                        worst[ins] = merged
            entered += int(any_fire)
    return entered / float(waves * tiles), fires / float(waves * 128 * tiles)


def perturb(desc, n_bytes, noise, seed):
    rng = np.random.RandomState(seed)
    out = desc.astype(np.int32)
    for i in range(len(out)):
        pos = rng.choice(128, n_bytes, replace=False)
        out[i, pos] += rng.randint(-noise, noise + 1, n_bytes)
    return np.clip(out, 0, 255).astype(np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=3, help="timed alternations per neighbour count")
    ap.add_argument("--ranks", default="1,2,4,8")
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--waves", type=int, default=4, help="wavefronts replayed for the slow-path share (0: skip)")
    ap.add_argument("--slow-path-sizes", default="4096,65536")
    ap.add_argument("--perturbed", type=int, default=20000, help="keys of the recall part (0: skip it and the query part)")
    ap.add_argument("--bytes", type=int, default=16)
    ap.add_argument("--noise", type=int, default=24)
    ap.add_argument("--query-keys", type=int, default=40000)
    ap.add_argument("--hamming", type=int, default=24)
    ap.add_argument("--quality-size", type=int, default=65536, help="K of the recall and query parts")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(v) for v in a.sizes.split(",") if v]
    ranks = [int(v) for v in a.ranks.split(",") if v]
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    from vocabulary_report import device_copy
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "the packed descriptors of %d x %dx%d dense band-noise images, default parameters; per K a warm-up of every neighbour "
                          "count, then %d alternations" % (a.batch, a.width, a.height, a.rounds), "library": hesaff_amd.lib_path(), "timing": {},
              "slow_path": {}}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
        torch.cuda.synchronize()
        ch, cd, dkeys, total = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
        keys = device_copy(torch, dkeys, total * 164).view(total, 164)
        desc = keys[:, 36:].contiguous()
        del keys, imgs
        torch.cuda.synchronize()
        cd = np.asarray(cd, np.int64)
        report["keys"] = int(total)
        report["keys_per_image_mean"] = float(cd.mean())
        ctx.set_profiling(1)
        words = torch.empty((total, 2), dtype=torch.int32, device="cuda")
        plain = torch.empty((total, 2), dtype=torch.int32, device="cuda")

        def vocabulary(K):
            pick = torch.tensor([r * total // K for r in range(K)], device="cuda")
            return desc[pick].cpu().numpy()

        for K in sizes:
            ctx.set_vocabulary(vocabulary(K))

            def assign(R, out):
                ctx.set_vocabulary_neighbours(R)
                ctx.assign_words_device(desc.data_ptr(), total, 128, 0, out.data_ptr())
                return ctx.assign_ms
            for R in ranks:
                assign(R, plain if R == 1 else words)   # warm-up
                if R > 1:
                    ptr, rows, r = ctx.neighbours_device()
                    assert rows == total and r == R
                    assert bool((words == plain).all().item()), "rank 0 at R = %d differs from the plain assignment" % R
            ms = {R: [] for R in ranks}
            for _ in range(a.rounds):
                for R in ranks:
                    ms[R].append(assign(R, words))
            base = median(ms[1]) if 1 in ms else None
            r = {}
            for R in ranks:
                q = {"assign_ms": median(ms[R]), "assign_ms_rounds": ms[R]}
                if base:
                    q["ratio_to_plain"] = q["assign_ms"] / base
                    q["ratio_to_R_sweeps"] = q["assign_ms"] / (R * base)
                    q["per_image_ms"] = q["assign_ms"] / a.batch
                r[str(R)] = q
            report["timing"][str(K)] = r
            print(json.dumps({"timing": {str(K): r}}), flush=True)
            ctx.set_vocabulary_neighbours(1)
        # the slow path, replayed on the host
        if a.waves > 0:
            first = [int(v) * (total // a.waves) // 64 * 64 for v in range(a.waves)]
            sample = np.concatenate([desc[f:f + 64].cpu().numpy() for f in first])
            for K in [int(v) for v in a.slow_path_sizes.split(",") if v]:
                vocab = vocabulary(K)
                r = {}
                for R in ranks:
                    if R == 1:
                        continue
                    cap = 2 if R <= 2 else 4 if R <= 4 else 8
                    share, fires = slow_path_share(sample, vocab, cap)
                    r[str(R)] = {"list_capacity": cap, "share_of_wave_tiles_entering": share, "firing_compares_per_list_and_tile": fires}
                report["slow_path"][str(K)] = r
                print(json.dumps({"slow_path": {str(K): r}}), flush=True)
        # what the mode buys
        if a.perturbed > 0:
            K = a.quality_size
            ctx.set_vocabulary(vocabulary(K))
            ctx.set_vocabulary_neighbours(1)
            ctx.assign_words_device(desc.data_ptr(), total, 128, 0, plain.data_ptr())
            pick = (np.arange(a.perturbed, dtype=np.int64) * total // a.perturbed)
            own = desc[torch.from_numpy(pick).cuda()].cpu().numpy()
            true_word = plain[torch.from_numpy(pick).cuda(), 0].cpu().numpy()
            moved = perturb(own, a.bytes, a.noise, seed=99)
            ctx.set_vocabulary_neighbours(8)
            nb = ctx.assign_neighbours(moved)
            recall = {str(R): float((nb[:, :R, 0] == true_word[:, None]).any(axis=1).mean()) for R in ranks}
            report["recall"] = {"vocabulary_size": K, "keys": int(a.perturbed), "bytes_moved": a.bytes, "noise": a.noise,
                                "mean_dist2_of_the_perturbation": float(((moved.astype(np.int64) - own) ** 2).sum(axis=1).mean()),
                                "share_with_the_unperturbed_word_among_R": recall}
            print(json.dumps({"recall": report["recall"]}), flush=True)
            # the query: image 0's first keys, perturbed, against an index of all images
            starts = np.concatenate([[0], np.cumsum(cd)])
            host_words = plain[:, 0].cpu().numpy()
            P = hesaff_amd.embedding_projection(0)
            tau, _ = ctx.train_embedding_device(desc.data_ptr(), total, 128, 0, plain.data_ptr(), 2, K, P)
            ctx.set_embedding(P, tau)
            sig = torch.empty(total, dtype=torch.int64, device="cuda")
            ctx.embed_device(desc.data_ptr(), total, 128, 0, plain.data_ptr(), 2, sig.data_ptr())
            host_sigs = sig.cpu().numpy().view(np.uint64)
            per_image = [host_words[starts[i]:starts[i + 1]] for i in range(a.batch)]
            per_image_sigs = [host_sigs[starts[i]:starts[i + 1]] for i in range(a.batch)]
            nq = int(min(a.query_keys, cd[0]))
            q_desc = perturb(desc[:nq].cpu().numpy(), a.bytes, a.noise, seed=100)
            ctx.build_index(per_image, K, signatures=per_image_sigs)
            query = {"vocabulary_size": K, "images": int(a.batch), "query_keys": nq, "hamming": a.hamming, "ranks": {}}
            for R in (1, 3):
                ctx.set_vocabulary_neighbours(R)
                qn = ctx.assign_neighbours(q_desc)
                qs = np.stack([ctx.embed(q_desc, np.ascontiguousarray(qn[:, r])) for r in range(R)], axis=1)
                qw = np.ascontiguousarray(qn[:, :, 0].reshape(-1))
                out = {}
                for name, kw in (("plain", {}), ("hamming", {"signatures": np.ascontiguousarray(qs.reshape(-1)), "hamming": a.hamming})):
                    im, sc = ctx.query_index(qw, a.batch, **kw)
                    at = int(np.nonzero(im == 0)[0][0]) if (im == 0).any() else -1
                    out[name] = {"rank_of_the_true_image": at + 1 if at >= 0 else None, "score_of_the_true_image": float(sc[at]) if at >= 0 else 0.0,
                                 "best_other_score": float(max([s for i, s in zip(im, sc) if i != 0] or [0.0]))}
                query["ranks"][str(R)] = out
            report["query"] = query
            print(json.dumps({"query": query}), flush=True)
            ctx.clear_index()
            ctx.set_embedding(None)
            ctx.set_vocabulary_neighbours(1)
        ctx.set_vocabulary(None)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
