#!/usr/bin/env python3
"""What the dominant-orientation mode (hesaff_set_orientation) costs, on the bench's two image families.

One process, one context: device-resident hesaff_detect_batch_device on B images of 3840 x 2160 at profiling level 1, the dense
family (synth.BANDS) and the natural-density one (synth.BANDS_NATURAL).  Both modes are warmed up first; the timed steps then
ALTERNATE the modes within the same run (0, 1, 0, 1, ...), so that drift of the device hits both alike.

Prints one JSON line.  Per family and mode: the median total_ms with its spread (min, max), the medians of the stage times, Hessian
keypoints and descriptors per image, images/s (from the median total_ms); for mode 1 also, against mode 0 of the same run,
patch_ratio = patch_ms / patch_ms[0], step_ratio = total_ms / total_ms[0] and lost_in_pass_two: the share of mode 0's described
keypoints that normalizeAffine rejects for the turned frame.

    python tools/orientation_report.py [--batch 32] [--steps 5] [--out report.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("total_ms", "detect_ms", "affine_ms", "patch_ms", "sift_ms", "pyramid_ms", "pack_ms")
MODES = (0, 1)


def measure(ctx, imgs, width, height, steps):
    """-> {mode: {stage: [ms per timed step], "hessian": per image, "desc": per image}}"""
    n = imgs.shape[0]
    out = {}
    for mode in MODES:   # warm-up: buffers grown, every kernel loaded, in both modes
        ctx.set_orientation(mode)
        ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
        out[mode] = {s: [] for s in STAGES}
        out[mode]["hessian"] = float(ch.sum()) / n
        out[mode]["desc"] = float(cd.sum()) / n
    for _ in range(steps):
        for mode in MODES:
            ctx.set_orientation(mode)
            ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
            assert float(ch.sum()) / n == out[mode]["hessian"] and float(cd.sum()) / n == out[mode]["desc"], "counts changed between steps"
            t = ctx.timings()
            for s in STAGES:
                out[mode][s].append(float(getattr(t, s)))
    ctx.set_orientation(0)
    return out


def summarise(raw, batch):
    rows = {}
    base = raw[0]
    for mode in MODES:
        r = raw[mode]
        row = {"hessian_per_image": r["hessian"], "desc_per_image": r["desc"]}
        for s in STAGES:
            row[s] = float(np.median(r[s]))
        row["total_ms_min"] = float(min(r["total_ms"])); row["total_ms_max"] = float(max(r["total_ms"]))
        row["images_per_s"] = batch / (row["total_ms"] * 1e-3)
        if mode:
            row["patch_ratio"] = row["patch_ms"] / float(np.median(base["patch_ms"]))
            row["step_ratio"] = row["total_ms"] / float(np.median(base["total_ms"]))
            row["lost_in_pass_two"] = 1.0 - r["desc"] / base["desc"] if base["desc"] else 0.0
        rows[str(mode)] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per mode (at least 5 for the figures in DESIGN.md)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1 or a.batch < 1:
        ap.error("steps and batch at least 1")
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "%d x %dx%d band-noise images, default parameters, hesaff_detect_batch_device, profiling level 1; "
                          "%d timed steps per mode, modes 0 (up) and 1 (dominant) alternating within the run" % (a.batch, a.width, a.height, a.steps),
              "families": {}}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        for family, bands in (("dense", synth.BANDS), ("natural", synth.BANDS_NATURAL)):
            imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=bands)
            torch.cuda.synchronize()
            report["families"][family] = summarise(measure(ctx, imgs, a.width, a.height, a.steps), a.batch)
            del imgs
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
