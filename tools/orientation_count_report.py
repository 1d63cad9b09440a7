#!/usr/bin/env python3
"""What the orientation count (hesaff_set_orientation_count: secondary orientation peaks) costs, on the bench's dense image family.

One process, one context: device-resident hesaff_detect_batch_device on B images of 3840 x 2160 at profiling level 1.  Four settings -
ORI_UP, and ORI_DOMINANT with K = 1, 2 and 4 - are warmed up first; the timed steps then ALTERNATE the settings within the same run
(up, 1, 2, 4, up, 1, ...), so that drift of the device hits all alike.

Prints one JSON line.  Per setting: the median total_ms with its spread (min, max), the medians of the stage times, Hessian keypoints
and keys per image, images/s (from the median total_ms), step_ratio against ORI_UP of the same run; for K > 1 also the census of
keys per region (how many regions of the batch have 0, 1, 2, 3 and 4 keys, from one hesaff_detect_regions call on the first image).

    python tools/orientation_count_report.py [--batch 32] [--steps 5] [--out report.json]

--lib PATH loads another build of the library (the parent commit's, built beside this one) and measures ORI_UP and K = 1 only, in the
same alternating way: the two reports' "up" and "1" rows are what the parent comparison reads.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("total_ms", "detect_ms", "affine_ms", "patch_ms", "sift_ms", "pyramid_ms", "pack_ms")
SETTINGS = (("up", 0, 1), ("1", 1, 1), ("2", 1, 2), ("4", 1, 4))   # name, orientation mode, orientation count


def apply(ctx, mode, count, has_count):
    ctx.set_orientation(mode)
    if has_count:
        ctx.set_orientation_count(count)


def measure(ctx, imgs, width, height, steps, settings, has_count):
    n = imgs.shape[0]
    out = {}
    for name, mode, count in settings:   # warm-up: buffers grown, every kernel loaded, in every setting
        apply(ctx, mode, count, has_count)
        ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
        out[name] = {s: [] for s in STAGES}
        out[name]["hessian"] = float(ch.sum()) / n
        out[name]["keys"] = float(cd.sum()) / n
    for _ in range(steps):
        for name, mode, count in settings:
            apply(ctx, mode, count, has_count)
            ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
            assert float(ch.sum()) / n == out[name]["hessian"] and float(cd.sum()) / n == out[name]["keys"], "counts changed between steps"
            t = ctx.timings()
            for s in STAGES:
                out[name][s].append(float(getattr(t, s)))
    return out


def census(ctx, img, count):
    """keys per region of one image: [regions with 0, 1, 2, 3, 4 keys] among those findAffineShape converged on"""
    apply(ctx, 1, count, True)
    (regions, _), = ctx.detect_regions([img])
    conv = regions[regions["outcome"] >= 1]
    return np.bincount(conv["reserved"], minlength=5)[:5].tolist()


def summarise(raw, batch):
    rows = {}
    base = float(np.median(raw["up"]["total_ms"]))
    for name, r in raw.items():
        row = {"hessian_per_image": r["hessian"], "keys_per_image": r["keys"]}
        for s in STAGES:
            row[s] = float(np.median(r[s]))
        row["total_ms_min"] = float(min(r["total_ms"])); row["total_ms_max"] = float(max(r["total_ms"]))
        row["images_per_s"] = batch / (row["total_ms"] * 1e-3)
        row["step_ratio"] = row["total_ms"] / base
        rows[name] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per setting (at least 5 for the figures in DESIGN.md)")
    ap.add_argument("--lib", default=None, help="another build of libhesaff_amd.so (the parent commit's): ORI_UP and K = 1 only")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.steps < 1 or a.batch < 1:
        ap.error("steps and batch at least 1")
    if a.lib:
        os.environ["HESAFF_AMD_LIB"] = a.lib
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    has_count = hasattr(hesaff_amd.load_library(), "hesaff_set_orientation_count")
    settings = SETTINGS if has_count and not a.lib else SETTINGS[:2]
    report = {"workload": "%d x %dx%d dense band-noise images, default parameters, hesaff_detect_batch_device, profiling level 1; %d timed steps per "
                          "setting, settings %s alternating within the run" % (a.batch, a.width, a.height, a.steps, [s[0] for s in settings]),
              "library": hesaff_amd.lib_path()}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
        torch.cuda.synchronize()
        report["settings"] = summarise(measure(ctx, imgs, a.width, a.height, a.steps, settings, has_count), a.batch)
        if len(settings) == len(SETTINGS):
            first = imgs[0].cpu().numpy()
            for name, _, count in settings[2:]:
                report["settings"][name]["keys_per_region_census"] = census(ctx, first, count)
        del imgs
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
