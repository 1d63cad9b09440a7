#!/usr/bin/env python3
"""What the RootSIFT descriptor mode (hesaff_set_descriptor) costs, and what it does to the matching score.

One process, one context: device-resident hesaff_detect_batch_device on B dense images (synth.BANDS) of 3840 x 2160 at profiling
level 1.  Both modes are warmed up first; the timed steps then ALTERNATE the modes within the same run (0, 1, 0, 1, ...), so that
drift of the device hits both alike.

Prints one JSON line.  Per mode: the median total_ms with its spread (min, max), the medians of the stage times, Hessian keypoints
and descriptors per image, images/s (from the median total_ms); for mode 1 also, against mode 0 of the same run, sift_delta_ms,
step_delta_ms, sift_ratio and step_ratio.  "matching": tools/repeatability.py's synthetic sequence (a band-noise image and five
warped copies) detected in each mode and evaluated by its Mikolajczyk-protocol code - the regions are the same in both modes, the
matching scores are recorded as they come, with no bar.

    python tools/descriptor_mode_report.py [--batch 32] [--steps 5] [--no-matching] [--out report.json]
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
        ctx.set_descriptor(mode)
        ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
        out[mode] = {s: [] for s in STAGES}
        out[mode]["hessian"] = float(ch.sum()) / n
        out[mode]["desc"] = float(cd.sum()) / n
    for _ in range(steps):
        for mode in MODES:
            ctx.set_descriptor(mode)
            ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
            assert float(ch.sum()) / n == out[mode]["hessian"] and float(cd.sum()) / n == out[mode]["desc"], "counts changed between steps"
            t = ctx.timings()
            for s in STAGES:
                out[mode][s].append(float(getattr(t, s)))
    ctx.set_descriptor(0)
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
            assert r["hessian"] == base["hessian"] and r["desc"] == base["desc"], "the mode changed a count"
            row["sift_delta_ms"] = row["sift_ms"] - float(np.median(base["sift_ms"]))
            row["step_delta_ms"] = row["total_ms"] - float(np.median(base["total_ms"]))
            row["sift_ratio"] = row["sift_ms"] / float(np.median(base["sift_ms"]))
            row["step_ratio"] = row["total_ms"] / float(np.median(base["total_ms"]))
        rows[str(mode)] = row
    return rows


def matching(ctx, width, height, angles=(10, 20, 30, 40, 50), seed=1234):
    """tools/repeatability.py's synthetic sequence under both modes -> {mode: [evaluate() per pair]}"""
    import hesaff_amd
    from hesaff_amd.synth import band_noise_image
    from tools import repeatability as rp
    base = band_noise_image(height, width, seed)
    imgs = [base]; Hs = [np.eye(3)]
    for a in angles:
        H = rp.viewpoint_homography(width, height, a)
        imgs.append(rp.warp_image(base, H, (width, height))); Hs.append(H)
    out = {}
    for mode in MODES:
        ctx.set_descriptor(mode)
        res = ctx.detect_batch(imgs)
        regs = []
        for _, keys in res:
            e = hesaff_amd.ellipse(keys, ctx.params.mrSize).astype(np.float64)
            regs.append((np.c_[keys["x"].astype(np.float64), keys["y"].astype(np.float64), e], np.ascontiguousarray(keys["desc"])))
        pairs = []
        for a, H, (r, d) in zip(angles, Hs[1:], regs[1:]):
            ev = rp.evaluate(regs[0][0], regs[0][1], r, d, H, (width, height), (width, height))
            ev["viewpoint_deg"] = a
            pairs.append(ev)
        out[str(mode)] = {"pairs": pairs, "mean_matching_score": float(np.mean([p["matching_score"] for p in pairs])),
                          "mean_repeatability": float(np.mean([p["repeatability"] for p in pairs]))}
    ctx.set_descriptor(0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per mode (at least 5 for the figures in DESIGN.md)")
    ap.add_argument("--seq-width", type=int, default=800, help="size of the matching sequence's images")
    ap.add_argument("--seq-height", type=int, default=640)
    ap.add_argument("--no-matching", action="store_true", help="timings only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1 or a.batch < 1:
        ap.error("steps and batch at least 1")
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "%d x %dx%d dense band-noise images, default parameters, hesaff_detect_batch_device, profiling level 1; "
                          "%d timed steps per mode, modes 0 (SIFT) and 1 (RootSIFT) alternating within the run" % (a.batch, a.width, a.height, a.steps)}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
        torch.cuda.synchronize()
        report["modes"] = summarise(measure(ctx, imgs, a.width, a.height, a.steps), a.batch)
        del imgs
        ctx.set_profiling(0)
        if not a.no_matching:
            report["matching"] = matching(ctx, a.seq_width, a.seq_height)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
