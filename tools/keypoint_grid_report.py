#!/usr/bin/env python3
"""What a spatially uniform keypoint budget (hesaff_set_keypoint_grid) costs and what it buys, on the bench's two image families.

One process, one context: device-resident hesaff_detect_batch_device on B images of 3840 x 2160 at profiling level 1, the dense
family (synth.BANDS) and the natural-density one (synth.BANDS_NATURAL).  The cases are limit 0, and every limit N of --limits with
the grids of --grids (1x1 = the plain limit).  Every case is warmed up first; the timed steps then ALTERNATE the cases within the
same run, so that drift of the device hits every case alike.

Prints one JSON line.  Per family and case "N/RxC": the median total_ms with its spread (min, max), the medians of detect_ms,
affine_ms, patch_ms and sift_ms, kept Hessian keypoints and descriptors per image, images/s (from the median total_ms), and against
limit 0 of the same run: selection_ms = detect_ms - detect_ms[0] (the cost of the selection kernels) and step_ratio = total_ms /
total_ms[0].  Coverage: of a fixed 16 x 16 probe grid over the image, how many of the 256 cells hold at least one kept Hessian
keypoint ("probe_cells_hessian") and at least one described keypoint ("probe_cells_desc"), the mean over the first --coverage-images
images, taken once per case through hesaff_detect_regions outside the timed steps.
"condition_ok": in both families every gridded case's median total_ms is below the minimum total_ms at limit 0.

    python tools/keypoint_grid_report.py [--batch 32] [--steps 5] [--limits 500,2000,8000] [--grids 1x1,4x4,8x8] [--out report.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STAGES = ("total_ms", "detect_ms", "affine_ms", "patch_ms", "sift_ms", "pyramid_ms", "pack_ms")
PROBE = 16


def set_case(ctx, case):
    """(limit, rows, cols) on the context, through states both setters accept"""
    limit, rows, cols = case
    ctx.set_keypoint_grid(1, 1)
    ctx.set_keypoint_limit(limit)
    ctx.set_keypoint_grid(rows, cols)


def name_of(case):
    return "%d/%dx%d" % case


def probe_cells(x, y, width, height):
    """occupied cells of the PROBE x PROBE grid over the image (the library's pixel and cell rule)"""
    if len(x) == 0:
        return 0
    col = np.clip((np.asarray(x, np.float32) + np.float32(0.5)).astype(np.int64), 0, width - 1)
    row = np.clip((np.asarray(y, np.float32) + np.float32(0.5)).astype(np.int64), 0, height - 1)
    return len(np.unique(((row + 1) * PROBE - 1) // height * PROBE + ((col + 1) * PROBE - 1) // width))


def measure(ctx, imgs, host_imgs, width, height, cases, steps):
    """-> {case: {stage: [ms per timed step], "hessian": per image, "desc": per image, coverage}}"""
    n = imgs.shape[0]
    out = {}
    for case in cases:   # warm-up: buffers grown, every kernel loaded, for every case; coverage on the side
        set_case(ctx, case)
        ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
        out[case] = {s: [] for s in STAGES}
        out[case]["hessian"] = float(ch.sum()) / n
        out[case]["desc"] = float(cd.sum()) / n
        if host_imgs:
            res = ctx.detect_regions(host_imgs)
            out[case]["probe_cells_hessian"] = float(np.mean([probe_cells(r["x"], r["y"], width, height) for r, _ in res]))
            out[case]["probe_cells_desc"] = float(np.mean([probe_cells(k["x"], k["y"], width, height) for _, k in res]))
    for _ in range(steps):
        for case in cases:
            set_case(ctx, case)
            ch, cd, _, _ = ctx.detect_batch_device(imgs.data_ptr(), n, width, height)
            assert float(ch.sum()) / n == out[case]["hessian"] and float(cd.sum()) / n == out[case]["desc"], "counts changed between steps"
            t = ctx.timings()
            for s in STAGES:
                out[case][s].append(float(getattr(t, s)))
    set_case(ctx, (0, 1, 1))
    return out


def summarise(raw, cases, batch):
    rows = {}
    base = raw[(0, 1, 1)]
    for case in cases:
        r = raw[case]
        row = {"hessian_per_image": r["hessian"], "desc_per_image": r["desc"]}
        for k in ("probe_cells_hessian", "probe_cells_desc"):
            if k in r:
                row[k] = r[k]
        for s in STAGES:
            row[s] = float(np.median(r[s]))
        row["total_ms_min"] = float(min(r["total_ms"])); row["total_ms_max"] = float(max(r["total_ms"]))
        row["images_per_s"] = batch / (row["total_ms"] * 1e-3)
        row["selection_ms"] = row["detect_ms"] - float(np.median(base["detect_ms"]))
        row["step_ratio"] = row["total_ms"] / float(np.median(base["total_ms"]))
        rows[name_of(case)] = row
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per case (at least 5 for the figures in DESIGN.md)")
    ap.add_argument("--limits", default="500,2000,8000")
    ap.add_argument("--grids", default="1x1,4x4,8x8")
    ap.add_argument("--coverage-images", type=int, default=4, help="images of the batch whose kept keypoints are counted into the probe grid (0: none)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    limits = [int(v) for v in a.limits.split(",")]
    grids = [tuple(int(v) for v in g.split("x")) for g in a.grids.split(",")]
    if any(v < 1 for v in limits) or a.steps < 1 or a.batch < 1 or any(len(g) != 2 or min(g) < 1 or g[0] * g[1] > 64 for g in grids):
        ap.error("limits are positive; grids are RxC with R * C <= 64; steps and batch at least 1")
    cases = [(0, 1, 1)] + [(n, r, c) for n in limits for r, c in grids if r * c <= n]
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "%d x %dx%d band-noise images, default parameters, hesaff_detect_batch_device, profiling level 1; "
                          "%d timed steps per case, cases alternating within the run" % (a.batch, a.width, a.height, a.steps),
              "cases": [name_of(c) for c in cases], "probe_grid": "%dx%d" % (PROBE, PROBE), "families": {}}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        for family, bands in (("dense", synth.BANDS), ("natural", synth.BANDS_NATURAL)):
            imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=bands)
            torch.cuda.synchronize()
            host_imgs = [im for im in imgs[:min(a.coverage_images, a.batch)].cpu().numpy()]
            report["families"][family] = summarise(measure(ctx, imgs, host_imgs, a.width, a.height, cases, a.steps), cases, a.batch)
            del imgs
    report["condition_ok"] = all(row["total_ms"] < fam[name_of((0, 1, 1))]["total_ms_min"]
                                 for fam in report["families"].values() for name, row in fam.items() if not name.endswith("1x1"))
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
