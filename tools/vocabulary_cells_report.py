#!/usr/bin/env python3
"""What visual-word assignment through vocabulary cells (hesaff_set_vocabulary_cells, kernels_cells.h) costs on the bench's dense image
family against the flat assignment of the same rows, how often the two agree, and what a training iteration inside the cells costs
against a flat one.

One process, one context at profiling level 1.  The keys of B dense 3840 x 2160 band-noise images (hesaff_detect_batch_device) are
copied once into a packed [n, 128] tensor.  Per (K, C): C coarse rows are trained on the keys (`--coarse-iterations` flat iterations),
K rows are spread over the keys (row r = key r n // K) and sorted into cells (hesaff_build_vocabulary_cells), and one training
iteration inside the cells makes them means of their keys.  Those K rows are then assigned flat and through the layer, the two
settings alternated `--rounds` times after a warm-up of each: hesaff_get_assign_ms for both, hesaff_get_assign_cells_ms for the three
parts.  The training iteration is timed the same way, alternating hesaff_train_vocabulary_cells_device and
hesaff_train_vocabulary_device from the same rows (hesaff_get_training_ms; the once-per-call coarse step and grouping of the cell
route lie outside its events, so the whole call is also timed on the host clock, copies of the rows included on both sides).

    python tools/vocabulary_cells_report.py [--batch 32] [--rounds 3] [--sizes 65536:256,1048576:1024] [--out report.json]
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


def median(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=3, help="timed alternations per setting")
    ap.add_argument("--sizes", default="65536:256,1048576:1024", help="K:C pairs")
    ap.add_argument("--coarse-iterations", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split(":")) for s in a.sizes.split(",")]
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    from vocabulary_report import device_copy
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "the packed descriptors of %d x %dx%d dense band-noise images, default parameters; per (K, C) a warm-up of either setting, "
                          "then %d alternations" % (a.batch, a.width, a.height, a.rounds), "library": hesaff_amd.lib_path(), "sizes": {}}
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
        out = [torch.empty((total, 2), dtype=torch.int32, device="cuda") for _ in range(2)]
        for K, C in sizes:
            coarse = ctx.train_vocabulary_device(desc.data_ptr(), total, 128, 0, C, a.coarse_iterations)[0]
            pick = torch.tensor([r * total // K for r in range(K)], device="cuda")
            v0, _, coarse, first = ctx.build_vocabulary_cells(desc[pick].cpu().numpy(), coarse)
            r = {"cells_with_rows": len(coarse), "rows_per_cell_max": int(np.diff(first.astype(np.int64)).max()), "evaluations_ratio": (len(coarse) + K / len(coarse)) / K}

            # a training iteration, cells against flat, from the same rows
            def train_cells():
                t = time.perf_counter()
                res = ctx.train_vocabulary_cells_device(desc.data_ptr(), total, 128, 0, v0, coarse, first, 1)
                return res, ctx.training_ms, (time.perf_counter() - t) * 1e3

            def train_flat():
                t = time.perf_counter()
                res = ctx.train_vocabulary_device(desc.data_ptr(), total, 128, 0, K, 1, init=v0)
                return res, ctx.training_ms, (time.perf_counter() - t) * 1e3
            train_cells(); train_flat()   # warm-up
            tc, tf = [], []
            for _ in range(a.rounds):
                tc.append(train_cells())
                tf.append(train_flat())
            rows = tc[-1][0][0]
            r["training_iteration"] = {
                "cells": {"assign_ms": median([x[1][0] for x in tc]), "accumulate_ms": median([x[1][1] for x in tc]), "update_ms": median([x[1][2] for x in tc]),
                          "call_ms_host_clock": median([x[2] for x in tc]), "distortion": int(tc[-1][0][1][0]), "empty": int(tc[-1][0][2][0])},
                "flat": {"assign_ms": median([x[1][0] for x in tf]), "accumulate_ms": median([x[1][1] for x in tf]), "update_ms": median([x[1][2] for x in tf]),
                         "call_ms_host_clock": median([x[2] for x in tf]), "distortion": int(tf[-1][0][1][0]), "empty": int(tf[-1][0][2][0])}}

            # the assignment of the trained rows, flat against cells
            ctx.set_vocabulary(rows)

            def assign(layer, o):
                if layer:
                    ctx.set_vocabulary_cells(coarse, first)
                else:
                    ctx.set_vocabulary_cells(None)
                ctx.assign_words_device(desc.data_ptr(), total, 128, 0, o.data_ptr())
                return ctx.assign_ms, ctx.assign_cells_ms
            assign(False, out[0]); assign(True, out[1])   # warm-up
            flat_ms, cells_ms, parts = [], [], []
            for _ in range(a.rounds):
                flat_ms.append(assign(False, out[0])[0])
                ms, pp = assign(True, out[1])
                cells_ms.append(ms); parts.append(pp)
            r["assign"] = {"flat_ms": median(flat_ms), "flat_ms_rounds": flat_ms, "cells_ms": median(cells_ms), "cells_ms_rounds": cells_ms,
                           "coarse_ms": median([q[0] for q in parts]), "group_ms": median([q[1] for q in parts]), "fine_ms": median([q[2] for q in parts]),
                           "factor": median(flat_ms) / median(cells_ms), "cells_below_flat": max(cells_ms) < min(flat_ms)}
            same = int((out[0][:, 0] == out[1][:, 0]).sum().item())
            r["agreement"] = {"share_of_keys_with_the_flat_word": same / total,
                              "dist2_sum_ratio_cells_over_flat": float(out[1][:, 1].double().sum().item() / out[0][:, 1].double().sum().item()),
                              "no_key_nearer_through_cells": bool((out[1][:, 1] >= out[0][:, 1]).all().item())}
            ctx.set_vocabulary(None)
            report["sizes"]["%d:%d" % (K, C)] = r
            print(json.dumps({"%d:%d" % (K, C): r}), flush=True)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
