#!/usr/bin/env python3
"""What a per-image keypoint limit (hesaff_set_keypoint_limit) costs and saves, on the bench's two image families.

One process, one context: device-resident hesaff_detect_batch_device on B images of 3840 x 2160 at profiling level 1, the dense
family (synth.BANDS) and the natural-density one (synth.BANDS_NATURAL).  Every limit is warmed up first; the timed steps then
ALTERNATE the limits within the same run (0, 500, 2000, 8000, 0, 500, ...), so that drift of the device hits every limit alike.

Prints one JSON line.  Per family and limit: the median total_ms with its spread (min, max), the medians of detect_ms, affine_ms,
patch_ms and sift_ms, kept Hessian keypoints and descriptors per image, images/s (from the median total_ms), and against limit 0 of
the same run: selection_ms = detect_ms - detect_ms[0] (the cost of the selection kernels) and step_ratio = total_ms / total_ms[0].
"condition_ok": the dense family's median total_ms at limit 2000 is below the minimum total_ms at limit 0.

    python tools/keypoint_limit_report.py [--batch 32] [--steps 5] [--limits 0,500,2000,8000] [--out report.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("total_ms", "detect_ms", "affine_ms", "patch_ms", "sift_ms", "pyramid_ms", "pack_ms")


def measure(ctx, imgs, width, height, limits, steps):
    """-> {limit: {stage: [ms per timed step], "hessian": per image, "desc": per image}}"""
    n = imgs.shape[0]
    out = {}
    for lim in limits:   # warm-up: buffers grown, every kernel loaded, for every limit
        ctx.set_keypoint_limit(lim)
        ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
        out[lim] = {s: [] for s in STAGES}
        out[lim]["hessian"] = float(ch.sum()) / n
        out[lim]["desc"] = float(cd.sum()) / n
    for _ in range(steps):
        for lim in limits:
            ctx.set_keypoint_limit(lim)
            ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
            assert float(ch.sum()) / n == out[lim]["hessian"] and float(cd.sum()) / n == out[lim]["desc"], "counts changed between steps"
            t = ctx.timings()
            for s in STAGES:
                out[lim][s].append(float(getattr(t, s)))
    ctx.set_keypoint_limit(0)
    return out


def summarise(raw, limits, batch):
    rows = {}
    base = raw[0] if 0 in raw else None
    for lim in limits:
        r = raw[lim]
        row = {"hessian_per_image": r["hessian"], "desc_per_image": r["desc"]}
        for s in STAGES:
            row[s] = float(np.median(r[s]))
        row["total_ms_min"] = float(min(r["total_ms"])); row["total_ms_max"] = float(max(r["total_ms"]))
        row["images_per_s"] = batch / (row["total_ms"] * 1e-3)
        if base is not None:
            row["selection_ms"] = row["detect_ms"] - float(np.median(base["detect_ms"]))
            row["step_ratio"] = row["total_ms"] / float(np.median(base["total_ms"]))
        rows[str(lim)] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per limit (at least 5 for the figures in DESIGN.md)")
    ap.add_argument("--limits", default="0,500,2000,8000")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    limits = [int(v) for v in a.limits.split(",")]
    if any(v < 0 for v in limits) or a.steps < 1 or a.batch < 1:
        ap.error("limits are 0 (no limit) or positive; steps and batch at least 1")
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "%d x %dx%d band-noise images, default parameters, hesaff_detect_batch_device, profiling level 1; "
                          "%d timed steps per limit, limits alternating within the run" % (a.batch, a.width, a.height, a.steps),
              "limits": limits, "families": {}}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        for family, bands in (("dense", synth.BANDS), ("natural", synth.BANDS_NATURAL)):
            imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=bands)
            torch.cuda.synchronize()
            report["families"][family] = summarise(measure(ctx, imgs, a.width, a.height, limits, a.steps), limits, a.batch)
            del imgs
    dense = report["families"]["dense"]
    if "0" in dense and "2000" in dense:
        report["condition_ok"] = bool(dense["2000"]["total_ms"] < dense["0"]["total_ms_min"])
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
