#!/usr/bin/env python3
"""What growing and reloading the image index costs (hesaff_index_add_device, hesaff_index_save / hesaff_index_load;
kernels_index_grow.h), against the rebuild it replaces and against a plain copy of the same bytes.

One process, one context at profiling level 1, HIP events through hesaff_get_index_growth_ms and hesaff_get_index_ms.  The
collection is tools/index_report.py's: `--images` images of `--keys` words each, Zipf-distributed (weight 1 / rank) over K words,
for every K of `--sizes`, generated on the device and indexed where they lie.  For every m of `--adds`, after a warm-up, `--rounds`
rounds of: build the N images (setup, not timed), ADD the next m images (timed, with its parts: insert, tables, merge, scatter),
then REBUILD the N + m images (timed) - the two routes alternate inside one job.  After the first add of every m the tables of the
grown index are compared with the rebuilt index's (df, idf, norm2, bit for bit): a difference ends the run with status 1.

The merge kernel moves every old posting once: 8 bytes read and 8 written.  Its rate is set against a hipMemcpyAsync
device-to-device of the same number of bytes in the same run, counted the same way (bytes read plus bytes written over the time).

Save and load: wall times of hesaff_index_save and hesaff_index_load of the N-image index at the first K, and the load's device
pass by its events.

    python tools/index_growth_report.py [--images 100000] [--keys 2000] [--sizes 65536,1048576] [--adds 1,100,10000] [--rounds 3] [--out report.json]
"""
import argparse
import ctypes
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from index_report import zipf_words   # noqa: E402


def median(values):
    return float(np.median(np.asarray(values, np.float64)))


def hip_runtime():
    """the HIP runtime this process has already loaded (torch's), by its path"""
    with open("/proc/self/maps") as f:
        for line in f:
            if "libamdhip64" in line:
                return ctypes.CDLL(line.split()[-1])
    raise RuntimeError("no HIP runtime is loaded")


def copy_rate(torch, n_bytes, rounds):
    """GB/s (read + written) of a device-to-device hipMemcpyAsync of n_bytes, the median of `rounds` after a warm-up"""
    hip = hip_runtime()
    hip.hipMemcpyAsync.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p]
    src = torch.empty(n_bytes, dtype=torch.uint8, device="cuda").fill_(1)
    dst = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    ms = []
    for r in range(rounds + 1):
        ev[0].record()
        rc = hip.hipMemcpyAsync(dst.data_ptr(), src.data_ptr(), n_bytes, 3, stream)   # 3: hipMemcpyDeviceToDevice
        ev[1].record()
        torch.cuda.synchronize()
        if rc != 0:
            raise RuntimeError("hipMemcpyAsync failed: %d" % rc)
        if r:
            ms.append(ev[0].elapsed_time(ev[1]))
    return median(ms), 2.0 * n_bytes / (median(ms) * 1e-3) / 1e9


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=100000)
    ap.add_argument("--keys", type=int, default=2000)
    ap.add_argument("--sizes", default="65536,1048576")
    ap.add_argument("--adds", default="1,100,10000")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import hesaff_amd
    adds = [int(s) for s in a.adds.split(",") if s]
    sizes = [int(s) for s in a.sizes.split(",") if s]
    N = a.images
    report = {"library": hesaff_amd.lib_path(), "images": N, "keys_per_image": a.keys, "rounds": a.rounds, "sizes": []}
    differ = 0
    p = hesaff_amd.default_params()
    p.max_batch = 1
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        for which, K in enumerate(sizes):
            words = zipf_words(torch, (N + max(adds)) * a.keys, K, seed=K)
            torch.cuda.synchronize()
            base = words.data_ptr()
            entry = {"vocabulary_size": K, "adds": []}
            for m in adds:
                old_counts = np.full(N, a.keys, np.int32)
                new_counts = np.full(m, a.keys, np.int32)
                all_counts = np.full(N + m, a.keys, np.int32)
                new_ptr = base + 4 * N * a.keys
                rows = []
                for r in range(a.rounds + 1):   # (round 0: the warm-up)
                    ctx.build_index_device(base, old_counts, 1, K)
                    old_postings = ctx.index_info[3]
                    t0 = time.perf_counter()
                    ctx.add_to_index_device(new_ptr, new_counts, 1)
                    add_wall = (time.perf_counter() - t0) * 1e3
                    parts = ctx.index_growth_ms[:4]
                    info = ctx.index_info
                    if r == 0:
                        grown = [x.copy() for x in ctx.index_tables()]
                    t0 = time.perf_counter()
                    ctx.build_index_device(base, all_counts, 1, K)
                    build_wall = (time.perf_counter() - t0) * 1e3
                    build_event = ctx.index_ms[0]
                    if r == 0:
                        same = ctx.index_info == info and all(np.array_equal(x, y) for x, y in zip(grown, ctx.index_tables()))
                        differ += 0 if same else 1
                        del grown
                        continue
                    rows.append({"insert": parts[0], "tables": parts[1], "merge": parts[2], "scatter": parts[3], "add_events": sum(parts), "add_wall": add_wall,
                                 "rebuild_event": build_event, "rebuild_wall": build_wall})
                merge_ms = median([x["merge"] for x in rows])
                entry["adds"].append({"m": m, "old_postings": int(old_postings), "postings": int(info[3]), "tables_equal_to_rebuild": bool(same),
                                      "ms": {key: {"median": median([x[key] for x in rows]), "all": [round(x[key], 4) for x in rows]} for key in rows[0]},
                                      "merge_bytes": 16 * int(old_postings), "merge_GBps": 16.0 * old_postings / (merge_ms * 1e-3) / 1e9})
            ctx.clear_index()
            copy_ms, copy_gbps = copy_rate(torch, 8 * int(old_postings), a.rounds)
            entry["copy_of_the_same_bytes"] = {"bytes_read_and_written": 16 * int(old_postings), "ms": copy_ms, "GBps": copy_gbps}
            if which == 0:
                ctx.build_index_device(base, old_counts, 1, K)
                want = [x.copy() for x in ctx.index_tables()]
                with tempfile.TemporaryDirectory() as d:
                    path = os.path.join(d, "index.bin")
                    save, load, device = [], [], []
                    for r in range(a.rounds):
                        ctx.build_index_device(base, old_counts, 1, K)
                        t0 = time.perf_counter()
                        ctx.save_index(path)
                        save.append((time.perf_counter() - t0) * 1e3)
                        ctx.clear_index()
                        t0 = time.perf_counter()
                        ctx.load_index(path)
                        load.append((time.perf_counter() - t0) * 1e3)
                        device.append(ctx.index_growth_ms[4])
                    same = all(np.array_equal(x, y) for x, y in zip(want, ctx.index_tables()))
                    differ += 0 if same else 1
                    entry["save_and_load"] = {"file_bytes": os.path.getsize(path), "save_wall_ms": {"median": median(save), "all": save},
                                              "load_wall_ms": {"median": median(load), "all": load}, "load_device_pass_ms": {"median": median(device), "all": device},
                                              "tables_equal_after_load": bool(same)}
                ctx.clear_index()
            report["sizes"].append(entry)
            del words
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    sys.exit(1 if differ else 0)


if __name__ == "__main__":
    main()
