#!/usr/bin/env python3
"""What removing images from the image index costs (hesaff_index_remove; kernels_index_remove.h), against the rebuild of the
remaining images it replaces and against a plain copy of the same bytes.

One process, one context at profiling level 1, HIP events through hesaff_get_index_remove_ms and hesaff_get_index_ms.  The
collection is tools/index_growth_report.py's: `--images` images of `--keys` words each, Zipf-distributed (weight 1 / rank) over K
words, for every K of `--sizes`, generated on the device and indexed where they lie.  For every m of `--removals`, m image numbers
are drawn without replacement (seeded), and after a warm-up `--rounds` rounds run: build the N images (setup, not timed), REMOVE the
m (timed, with its parts: count, tables, compact, keys), then REBUILD the N - m that remain from a packed copy of their words
(timed) - the two routes alternate inside one job.  In EVERY round the tables of the two routes are compared (df, idf, norm2 and
the counts, bit for bit): a difference ends the run with status 1.

The compaction reads every old posting and writes every surviving one, 8 bytes each.  Its rate is set against a hipMemcpyAsync
device-to-device of the old postings' bytes in the same run, counted the same way (bytes read plus bytes written over the time).

    python tools/index_remove_report.py [--images 100000] [--keys 2000] [--sizes 65536,1048576] [--removals 1,100,10000] [--rounds 3] [--out report.json]
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

from index_growth_report import copy_rate, median   # noqa: E402
from index_report import zipf_words   # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100000)
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--removals", default="1,100,10000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import hesaff_amd
    removals = [int(s) for s in a.removals.split(",") if s]
    sizes = [int(s) for s in a.sizes.split(",") if s]
    N = a.images
    report = {"library": hesaff_amd.lib_path(), "images": N, "keys_per_image": a.keys, "rounds": a.rounds, "sizes": []}
    differ = 0
    p = hesaff_amd.default_params()
    p.max_batch = 1
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        for K in sizes:
            words = zipf_words(torch, N * a.keys, K, seed=K)
            torch.cuda.synchronize()
            counts = np.full(N, a.keys, np.int32)
            entry = {"vocabulary_size": K, "removals": []}
            for m in removals:
                gone = np.random.RandomState(m).choice(N, m, replace=False).astype(np.int32)
                keep = np.ones(N, bool)
                keep[gone] = False
                left = words.view(N, a.keys)[torch.from_numpy(keep).cuda()].contiguous()   # the words of the images that remain, packed
                torch.cuda.synchronize()
                left_counts = np.full(N - m, a.keys, np.int32)
                rows, same_all = [], True
                for r in range(a.rounds + 1):   # (round 0: the warm-up)
                    ctx.build_index_device(words.data_ptr(), counts, 1, K)
                    old_postings = ctx.index_info[3]
                    t0 = time.perf_counter()
                    ctx.remove_from_index(gone)
                    wall = (time.perf_counter() - t0) * 1e3
                    parts = ctx.index_remove_ms()
                    info = ctx.index_info
                    removed = [x.copy() for x in ctx.index_tables()]
                    t0 = time.perf_counter()
                    ctx.build_index_device(left.data_ptr(), left_counts, 1, K)
                    build_wall = (time.perf_counter() - t0) * 1e3
                    build_event = ctx.index_ms[0]
                    same = ctx.index_info == info and all(np.array_equal(x, y) for x, y in zip(removed, ctx.index_tables()))
                    same_all = same_all and same
                    differ += 0 if same else 1
                    del removed
                    if r:
                        rows.append({"count": parts[0], "tables": parts[1], "compact": parts[2], "keys": parts[3], "remove_events": sum(parts), "remove_wall": wall,
                                     "rebuild_event": build_event, "rebuild_wall": build_wall})
                compact_ms = median([x["compact"] for x in rows])
                moved = 8 * (int(old_postings) + int(info[3]))
                entry["removals"].append({"m": m, "old_postings": int(old_postings), "postings": int(info[3]), "tables_equal_to_rebuild_in_every_round": bool(same_all),
                                          "ms": {key: {"median": median([x[key] for x in rows]), "all": [round(x[key], 4) for x in rows]} for key in rows[0]},
                                          "compact_bytes": moved, "compact_GBps": moved / (compact_ms * 1e-3) / 1e9})
                del left
            ctx.clear_index()
            copy_ms, copy_gbps = copy_rate(torch, 8 * int(old_postings), a.rounds)
            entry["copy_of_the_old_postings"] = {"bytes_read_and_written": 16 * int(old_postings), "ms": copy_ms, "GBps": copy_gbps}
            report["sizes"].append(entry)
            del words
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
