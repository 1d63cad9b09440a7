#!/usr/bin/env python3
"""What an iteration of vocabulary training (hesaff_train_vocabulary_device, kernels_train.h) costs on the bench's dense image family,
stage by stage, and how it compares with the same iteration written in torch.

One process, one context at profiling level 1.  The keys of B dense 3840 x 2160 band-noise images (hesaff_detect_batch_device) are
copied once into a packed [n, 128] tensor; both routes read that tensor.  Per vocabulary size K, after one warm-up iteration, `steps`
iterations run one call each (iterations = 1, init = the rows the call before returned; the first from the sampled rows), so that
hesaff_get_training_ms holds the HIP-event times of exactly one iteration: assignment, accumulation (histogram, scan, scatter, sums)
and update.  The vocabulary's round trip through the host between the calls lies outside the events.

The torch route runs the same iteration from the same rows: DESIGN.md's bf16 `mm` + argmin for the assignment
(tools/vocabulary_report.py: torch_route), index_add_ into an integer accumulator and bincount for the sums, the integer update.  Its
new rows must equal the library's row for row (mismatches are counted); its stages are timed with HIP events.

    python tools/vocabulary_training_report.py [--batch 32] [--steps 5] [--sizes 4096,65536] [--out report.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def torch_iteration(torch, torch_route, desc, vocab_dev, block):
    """one Lloyd iteration in torch -> (new rows uint8 [K, 128], distortion, empty, [assign, accumulate, update] ms)"""
    K = vocab_dev.shape[0]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
    ev[0].record()
    rows, _ = torch_route(torch, desc, vocab_dev, block)
    ev[1].record()
    word = rows[:, 0].long()
    wide = torch.int32 if desc.shape[0] * 255 < (1 << 31) else torch.int64
    sums = torch.zeros((K, 128), dtype=wide, device="cuda")
    sums.index_add_(0, word, desc.to(wide))
    counts = torch.bincount(word, minlength=K)
    ev[2].record()
    c = counts[:, None]
    mean = (2 * sums.long() + c) // torch.clamp(2 * c, min=1)
    new = torch.where(c > 0, mean, vocab_dev.long()).to(torch.uint8)
    ev[3].record()
    torch.cuda.synchronize()
    return new, int(rows[:, 1].long().sum().item()), int((counts == 0).sum().item()), [ev[q].elapsed_time(ev[q + 1]) for q in range(3)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=5, help="timed iterations per vocabulary size")
    ap.add_argument("--sizes", default="4096,65536")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    from vocabulary_report import device_copy, torch_route
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "the packed descriptors of %d x %dx%d dense band-noise images, default parameters; per K one warm-up iteration, then %d "
                          "iterations of one call each" % (a.batch, a.width, a.height, a.steps), "library": hesaff_amd.lib_path(), "sizes": {}}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
        torch.cuda.synchronize()
        ch, cd, dkeys, total = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
        keys = device_copy(torch, dkeys, total * 164).view(total, 164)
        desc = keys[:, 36:].contiguous()
        del keys, imgs
        torch.cuda.synchronize()
        report["keys"] = total
        ctx.set_profiling(1)
        for K in sizes:
            pick = torch.tensor([r * total // K for r in range(K)], device="cuda")
            vocab = desc[pick].cpu().numpy()
            block = max(256, min(total, (1 << 29) // K))
            ctx.train_vocabulary_device(desc.data_ptr(), total, 128, 0, K, 1, init=vocab)   # warm-up
            torch_iteration(torch, torch_route, desc[:4 * block], torch.from_numpy(vocab).cuda(), block)
            r = {"iterations": [], "row_block_of_the_torch_route": block}
            for _ in range(a.steps):
                new, dist, empty = ctx.train_vocabulary_device(desc.data_ptr(), total, 128, 0, K, 1, init=vocab)
                ms = ctx.training_ms
                t_new, t_dist, t_empty, t_ms = torch_iteration(torch, torch_route, desc, torch.from_numpy(vocab).cuda(), block)
                mism = int((t_new.cpu().numpy() != new).any(axis=1).sum())
                r["iterations"].append({"distortion": int(dist[0]), "empty": int(empty[0]), "assign_ms": ms[0], "accumulate_ms": ms[1], "update_ms": ms[2],
                                        "accumulate_share": ms[1] / sum(ms), "torch_ms": t_ms, "torch_rows_that_differ": mism,
                                        "torch_distortion_equal": t_dist == int(dist[0]), "torch_empty_equal": t_empty == int(empty[0])})
                vocab = new
            for name in ("assign_ms", "accumulate_ms", "update_ms", "accumulate_share"):
                r[name] = float(np.median([it[name] for it in r["iterations"]]))
            r["torch_ms"] = [float(np.median([it["torch_ms"][q] for it in r["iterations"]])) for q in range(3)]
            r["distortion_non_increasing"] = all(x["distortion"] >= y["distortion"] for x, y in zip(r["iterations"], r["iterations"][1:]))
            report["sizes"][str(K)] = r
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
