#!/usr/bin/env python3
"""What per-image detection masks (hesaff_set_next_masks_device) cost and save, on the bench's two image families.

One process, one context: device-resident hesaff_detect_batch_device on B images of 3840 x 2160 at profiling level 1, the dense
family (synth.BANDS) and the natural-density one (synth.BANDS_NATURAL), with device masks.  Four cases: no mask, an all-255 mask
(every keypoint kept: what the selection itself costs), a left-half mask, and a mask covering one tenth of the area (the leftmost
tenth of the columns).  Every case is warmed up first; the timed steps then ALTERNATE the cases within the same run (none, all,
half, tenth, none, ...), so that drift of the device hits every case alike.

Prints one JSON line.  Per family and case: the median total_ms with its spread (min, max), the medians of the stages, kept Hessian
keypoints and descriptors per image, images/s (from the median total_ms), and against "none" of the same run:
mask_ms = detect_ms - detect_ms[none] (for "all": the cost of the selection kernels alone) and step_ratio = total_ms / total_ms[none].
Asserted, per family: the half mask's median total_ms is below the minimum total_ms without a mask, and the all-255 mask keeps
exactly the counts of the run without a mask.

    python tools/detection_mask_report.py [--batch 32] [--steps 5] [--out report.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("total_ms", "detect_ms", "affine_ms", "patch_ms", "sift_ms", "pyramid_ms", "pack_ms")
CASES = ("none", "all", "half", "tenth")


def make_masks(torch, batch, height, width):
    """-> {case: uint8 tensor [batch, height, width] on the device, or None}"""
    def columns(upto):
        m = torch.zeros((batch, height, width), dtype=torch.uint8, device="cuda")
        m[:, :, :upto] = 255
        return m
    return {"none": None, "all": columns(width), "half": columns(width // 2), "tenth": columns(width // 10)}


def measure(ctx, imgs, masks, width, height, steps):
    """-> {case: {stage: [ms per timed step], "hessian": per image, "desc": per image, "counts": per-image Hessian counts}}"""
    n = imgs.shape[0]

    def step(case):
        m = masks[case]
        return ctx.detect_batch_device(imgs.data_ptr(), n, width, height, masks_ptr=None if m is None else m.data_ptr())
    out = {}
    for case in CASES:   # warm-up: buffers grown, every kernel loaded, for every case
        ch, cd, _, _ = step(case)
        out[case] = {s: [] for s in STAGES}
        out[case]["hessian"] = float(ch.sum()) / n
        out[case]["desc"] = float(cd.sum()) / n
        out[case]["counts"] = ch.tolist() + cd.tolist()
    for _ in range(steps):
        for case in CASES:
            ch, cd, _, _ = step(case)
            assert ch.tolist() + cd.tolist() == out[case]["counts"], "counts changed between steps"
            t = ctx.timings()
            for s in STAGES:
                out[case][s].append(float(getattr(t, s)))
    return out


def summarise(raw, batch):
    rows = {}
    base = raw["none"]
    for case in CASES:
        r = raw[case]
        row = {"hessian_per_image": r["hessian"], "desc_per_image": r["desc"]}
        for s in STAGES:
            row[s] = float(np.median(r[s]))
        row["total_ms_min"] = float(min(r["total_ms"])); row["total_ms_max"] = float(max(r["total_ms"]))
        row["images_per_s"] = batch / (row["total_ms"] * 1e-3)
        row["mask_ms"] = row["detect_ms"] - float(np.median(base["detect_ms"]))
        row["step_ratio"] = row["total_ms"] / float(np.median(base["total_ms"]))
        rows[case] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per case (at least 5 for the figures in DESIGN.md)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1 or a.batch < 1 or a.width < 10 or a.height < 1:
        ap.error("steps and batch at least 1, width at least 10")
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "%d x %dx%d band-noise images, default parameters, hesaff_detect_batch_device with device masks, profiling "
                          "level 1; %d timed steps per case, cases alternating within the run" % (a.batch, a.width, a.height, a.steps),
              "cases": list(CASES), "families": {}}
    ok = True
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        masks = make_masks(torch, a.batch, a.height, a.width)
        for family, bands in (("dense", synth.BANDS), ("natural", synth.BANDS_NATURAL)):
            imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=bands)
            torch.cuda.synchronize()
            raw = measure(ctx, imgs, masks, a.width, a.height, a.steps)
            rows = summarise(raw, a.batch)
            rows["all_counts_equal_none"] = raw["all"]["counts"] == raw["none"]["counts"]
            rows["half_below_none_min"] = bool(rows["half"]["total_ms"] < rows["none"]["total_ms_min"])
            ok = ok and rows["all_counts_equal_none"] and rows["half_below_none_min"]
            report["families"][family] = rows
            del imgs
    report["condition_ok"] = bool(ok)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    assert ok, "the half mask is not faster than no mask, or the all-255 mask changed the counts: see the JSON line"


if __name__ == "__main__":
    main()
