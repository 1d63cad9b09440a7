#!/usr/bin/env python3
"""Float grey-plane input against 8-bit input, in one process, alternating the two forms over several rounds after a warm-up:

  * the device-resident step: hesaff_detect_batch_device (uint8 planes) against hesaff_detect_batch_device_f32 (the same planes as
    float32, check kernel included) on a batch of B x H x W images;
  * the host-to-host rate: hesaff_detect_batch against hesaff_detect_batch_f32 on N host images (staging copy + value check, H2D,
    kernels, D2H, all pipelined by the chunk engine).

The float planes are float32(u8), so both forms compute the same keypoints; the report checks that the counts agree.  One JSON line.

    python tools/float_input_report.py [--batch 256] [--host-images 128] [--width 3840 --height 2160] [--rounds 3] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def base_images(h, w, k):
    from hesaff_amd.synth import band_noise_image
    return [band_noise_image(h, w, 1000 + i) for i in range(k)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--host-images", type=int, default=128)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import hesaff_amd

    H, W, B, N = a.height, a.width, a.batch, a.host_images
    bases = base_images(H, W, 4)
    out = {"config": {"batch": B, "host_images": N, "height": H, "width": W, "rounds": a.rounds, "warmup": 1,
                      "device": torch.cuda.get_device_name(0)}}

    # ---- device-resident step ----
    shifts = [(i % 4, 37 * (i // 4), 53 * (i // 4)) for i in range(B)]
    u8 = torch.empty((B, H, W), dtype=torch.uint8, device="cuda")
    for i, (k, dy, dx) in enumerate(shifts):
        u8[i] = torch.from_numpy(np.roll(bases[k], (dy, dx), axis=(0, 1))).cuda()
    f32 = u8.float()
    torch.cuda.synchronize()
    p = hesaff_amd.default_params(); p.max_batch = B
    step = {"u8_ms": [], "f32_ms": []}
    with hesaff_amd.HesaffContext(p, device=0) as c:
        def run_u8():
            return c.detect_batch_device(u8.data_ptr(), B, W, H)

        def run_f32():
            return c.detect_batch_device_f32(f32)
        r8 = run_u8(); rf = run_f32()   # warm-up (plans, allocations)
        assert np.array_equal(r8[0], rf[0]) and np.array_equal(r8[1], rf[1]) and r8[3] == rf[3], "float32(u8) must give the u8 counts"
        for _ in range(a.rounds):
            for name, fn in (("u8_ms", run_u8), ("f32_ms", run_f32)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn()
                torch.cuda.synchronize()
                step[name].append((time.perf_counter() - t0) * 1e3)
        c.set_profiling(1)
        run_u8(); t8 = c.timings()
        run_f32(); tf = c.timings()
        c.set_profiling(0)
        step["pyramid_stage_ms"] = {"u8": round(t8.pyramid_ms, 3), "f32": round(tf.pyramid_ms, 3)}
        step["descriptors_per_step"] = int(r8[3])
    step["u8_median_ms"] = float(np.median(step["u8_ms"]))
    step["f32_median_ms"] = float(np.median(step["f32_ms"]))
    step["f32_over_u8"] = step["f32_median_ms"] / step["u8_median_ms"]
    step["u8_ms"] = [round(v, 2) for v in step["u8_ms"]]; step["f32_ms"] = [round(v, 2) for v in step["f32_ms"]]
    out["device_step"] = step
    del u8, f32
    torch.cuda.empty_cache()

    # ---- host to host ----
    imgs8 = [np.roll(bases[i % 4], (41 * (i // 4), 29 * (i // 4)), axis=(0, 1)) for i in range(N)]
    imgsf = [im.astype(np.float32) for im in imgs8]
    host = {"u8_s": [], "f32_s": []}
    with hesaff_amd.HesaffContext(device=0) as c:
        n8 = [len(k) for _, k in c.detect_batch(imgs8)]
        nf = [len(k) for _, k in c.detect_batch_f32(imgsf)]
        assert n8 == nf, "float32(u8) must give the u8 counts"
        for _ in range(a.rounds):
            for name, fn in (("u8_s", lambda: c.detect_batch(imgs8)), ("f32_s", lambda: c.detect_batch_f32(imgsf))):
                t0 = time.perf_counter()
                fn()
                host[name].append(time.perf_counter() - t0)
    for k in ("u8", "f32"):
        s = float(np.median(host[k + "_s"]))
        host[k + "_images_per_s"] = N / s
        host[k + "_s"] = [round(v, 3) for v in host[k + "_s"]]
    host["f32_over_u8_rate"] = host["f32_images_per_s"] / host["u8_images_per_s"]
    host["input_bytes"] = {"u8": int(sum(im.nbytes for im in imgs8)), "f32": int(sum(im.nbytes for im in imgsf))}
    out["host_to_host"] = host
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
