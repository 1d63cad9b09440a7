#!/usr/bin/env python3
"""What "detect, choose, describe the chosen" costs: hesaff_describe_regions against hesaff_detect_regions, host to host, on the
bench's dense image family.

Legs, alternated within one process (one round = every leg once; the median over the rounds is reported):
  detect                  hesaff_detect_regions
  from_points_all         hesaff_describe_regions(HESAFF_FROM_POINTS) on every record detection returned
  from_shapes_converged   hesaff_describe_regions(HESAFF_FROM_SHAPES) on the records with outcome >= 1
  from_shapes_top10       hesaff_describe_regions(HESAFF_FROM_SHAPES) on the strongest 10 % of those by |response|, per image
  parent_detect           hesaff_detect_regions of another build of the library (--parent-lib: the commit before this entry point
                          existed), twice per round: the yardstick and its own spread
Only the C call is timed; each returns after the library's own synchronisation, with the results in host memory.

    python tools/describe_report.py [--images 64] [--rounds 10] [--parent-lib /path/to/libhesaff_amd.so] [--out profiles/....json]
Prints one JSON line.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=64)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--max-batch", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--parent-lib", default=None, help="libhesaff_amd.so of the parent commit (same ABI version)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.rounds < 10:
        ap.error("--rounds: at least 10 timed calls per leg")
    import torch
    import hesaff_amd
    from hesaff_amd import _binding
    from hesaff_amd.synth import band_noise_batch_torch
    n = a.images
    imgs = [np.ascontiguousarray(t.cpu().numpy()) for t in band_noise_batch_torch(n, a.height, a.width, seed=1234, device="cuda")]
    torch.cuda.synchronize()
    p = hesaff_amd.default_params()
    p.max_batch = a.max_batch
    ctx = hesaff_amd.HesaffContext(p, device=0)
    L = ctx.L
    _, _, ptrs, ws, hs, st, chs = ctx._u8_list(imgs)
    res = (_binding._RegionResult * n)()

    def detect(lib, handle):
        t0 = time.perf_counter()
        rc = lib.hesaff_detect_regions(handle, n, ptrs, ws, hs, st, chs, res)
        dt = time.perf_counter() - t0
        assert rc == 0, rc
        return dt

    detect(L, ctx.h)
    regions = [ctx._regions_at(r.regions, r.count_hessian) for r in res]
    n_keys = sum(r.count_desc for r in res)
    conv = [r[r["outcome"] >= 1] for r in regions]
    top = []
    for r in conv:
        k = max(1, len(r) // 10)
        keep = np.sort(np.argsort(-np.abs(r["response"]), kind="stable")[:k])   # the strongest tenth, in detection order
        top.append(r[keep])
    lists = {"from_points_all": (regions, 1), "from_shapes_converged": (conv, 2), "from_shapes_top10": (top, 2)}
    packed = {k: ctx._region_lists(v[0], n) for k, v in lists.items()}

    def describe(name):
        _, rptrs, counts = packed[name]
        t0 = time.perf_counter()
        rc = L.hesaff_describe_regions(ctx.h, n, ptrs, ws, hs, st, chs, rptrs, counts, lists[name][1], res)
        dt = time.perf_counter() - t0
        assert rc == 0, (rc, L.hesaff_last_error(ctx.h))
        return dt, sum(r.count_desc for r in res)

    parent = None
    if a.parent_lib:
        PL = C.CDLL(a.parent_lib)
        assert PL.hesaff_abi_version() == _binding.ABI_VERSION
        PL.hesaff_create.argtypes = [C.POINTER(C.c_void_p), C.POINTER(_binding.Params), C.c_int]
        PL.hesaff_destroy.argtypes = [C.c_void_p]; PL.hesaff_destroy.restype = None
        PL.hesaff_detect_regions.argtypes = L.hesaff_detect_regions.argtypes
        ph = C.c_void_p()
        assert PL.hesaff_create(C.byref(ph), C.byref(p), 0) == 0
        parent = (PL, ph)

    legs = ["detect"] + list(lists)
    times = {k: [] for k in legs + (["parent_detect", "parent_detect_again"] if parent else [])}
    described = {}
    for rnd in range(a.warmup + a.rounds):
        row = {}
        if parent:
            row["parent_detect"] = detect(*parent)
        row["detect"] = detect(L, ctx.h)
        for name in lists:
            row[name], described[name] = describe(name)
        if parent:
            row["parent_detect_again"] = detect(*parent)
        if rnd >= a.warmup:
            for k, v in row.items():
                times[k].append(v * 1e3)
    if parent:
        parent[0].hesaff_destroy(parent[1])
    ctx.close()
    med = {k: float(np.median(v)) for k, v in times.items()}
    report = {
        "workload": "%d x %dx%d band-noise images (the bench's generator, seed 1234), max_batch %d, host to host, default parameters"
                    % (n, a.width, a.height, a.max_batch),
        "rounds": a.rounds, "warmup_rounds": a.warmup,
        "hessian_keypoints": int(sum(len(r) for r in regions)), "described_by_detection": int(n_keys),
        "records": {k: int(sum(len(r) for r in v[0])) for k, v in lists.items()},
        "described": {k: int(v) for k, v in described.items()},
        "median_ms": med,
        "min_ms": {k: float(np.min(v)) for k, v in times.items()},
        "max_ms": {k: float(np.max(v)) for k, v in times.items()},
        "relative_to_detect": {k: med[k] / med["detect"] for k in lists},
    }
    if parent:
        both = np.array(times["parent_detect"] + times["parent_detect_again"])
        report["parent"] = {"lib": os.path.basename(os.path.dirname(os.path.abspath(a.parent_lib))) + "/" + os.path.basename(a.parent_lib),
                            "median_ms": float(np.median(both)), "min_ms": float(both.min()), "max_ms": float(both.max()),
                            "spread_of_the_two_positions_ms": abs(med["parent_detect"] - med["parent_detect_again"]),
                            "detect_relative_to_parent": med["detect"] / float(np.median(both))}
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
