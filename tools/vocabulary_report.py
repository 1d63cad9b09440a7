#!/usr/bin/env python3
"""What visual-word assignment (hesaff_set_vocabulary, k_assign_words) costs, on the bench's dense image family, and how it compares
with the same search written in torch.

One process, one context: device-resident hesaff_detect_batch_device on B images of 3840 x 2160 at profiling level 1.  The keys of a
first run without a vocabulary are kept on the device; every vocabulary is random bytes with 1 % of its rows taken from those keys.
After a warm-up in every setting, the timed steps ALTERNATE the settings within the run (none, K1, K2, ..., none, K1, ...), so that drift
of the device hits all alike.

Per vocabulary size K the JSON line holds:
  assign_ms            hesaff_get_assign_ms of every timed step, and their median
  step_ms              wall time of hesaff_detect_batch_device of every timed step (the call returns with the words in place), beside
                       step_ms of the no-vocabulary setting of the same run
  evals_per_s          keys x K / median assign time: distance evaluations per second
  fraction_of_i8_peak  evals_per_s x 128 multiply-adds x 2 / 5e15 (the dense i8 rate of an MI355X: twice its ~2.5 PF dense BF16 peak)
  torch                the baseline on the same keys and vocabulary: keys.bfloat16() @ vocab.bfloat16().T in row blocks with f32 output,
                       plus the norms and argmin.  Bytes are exact in bf16 and the f32 sums stay below 2^24, so it is exact; it is first
                       checked against the kernel's rows (mismatches counted), then timed with HIP events.  kernel_ms beside it is the
                       stand-alone hesaff_assign_words_device on the same packed tensor.

    python tools/vocabulary_report.py [--batch 32] [--steps 5] [--sizes 4096,65536,1048576] [--out report.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

I8_DENSE_OPS = 5.0e15


def device_copy(torch, ptr, nbytes):
    """nbytes at a raw device pointer of the library -> a torch uint8 tensor of its own"""
    buf = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    rc = hip.hipMemcpy(ctypes.c_void_p(buf.data_ptr()), ctypes.c_void_p(ptr), ctypes.c_size_t(nbytes), 3)
    if rc != 0:
        raise RuntimeError("hipMemcpy failed: %d" % rc)
    return buf


def make_vocabulary(torch, desc, K, seed):
    """uint8 [K, 128] on the host: random bytes, 1 % of the rows (at least one) replaced by descriptors of the keys"""
    rng = np.random.RandomState(seed)
    vocab = rng.randint(0, 256, (K, 128), dtype=np.uint8)
    m = max(1, K // 100)
    rows = rng.permutation(K)[:m]
    pick = torch.from_numpy(rng.randint(0, desc.shape[0], m)).cuda()
    vocab[rows] = desc[pick].cpu().numpy()
    return vocab


def torch_route(torch, desc, vocab_dev, block):
    """(word, dist2) int32 [n, 2] of desc against vocab_dev, the matrix product in bf16 with f32 output.  -> rows, route name"""
    n, K = desc.shape[0], vocab_dev.shape[0]
    v16 = vocab_dev.to(torch.bfloat16)
    vnorm = (vocab_dev.to(torch.float32) ** 2).sum(dim=1)
    out = torch.empty((n, 2), dtype=torch.int32, device="cuda")
    route = "bf16 mm, out_dtype=float32"
    for i0 in range(0, n, block):
        d = desc[i0:i0 + block]
        d16 = d.to(torch.bfloat16)
        try:
            if route.startswith("bf16"):
                dot = torch.mm(d16, v16.T, out_dtype=torch.float32)
        except (TypeError, RuntimeError):
            route = "float32 mm (this torch has no f32 output for a bf16 product)"
        if not route.startswith("bf16"):
            dot = d.to(torch.float32) @ vocab_dev.to(torch.float32).T
        score = vnorm[None, :] - 2.0 * dot
        best, word = score.min(dim=1)
        out[i0:i0 + block, 0] = word.to(torch.int32)
        out[i0:i0 + block, 1] = (best + (d.to(torch.float32) ** 2).sum(dim=1)).to(torch.int32)
    return out, route


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--steps", type=int, default=5, help="timed steps per setting")
    ap.add_argument("--sizes", default="4096,65536,1048576")
    ap.add_argument("--torch-runs", type=int, default=1, help="timed runs of the torch route per vocabulary size")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [int(s) for s in a.sizes.split(",")]
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "%d x %dx%d dense band-noise images, default parameters, hesaff_detect_batch_device, profiling level 1; %d timed steps "
                          "per setting, settings none, %s alternating within the run" % (a.batch, a.width, a.height, a.steps, sizes),
              "library": hesaff_amd.lib_path(), "i8_dense_ops_per_s": I8_DENSE_OPS}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
        torch.cuda.synchronize()

        def step():
            t0 = time.perf_counter()
            ch, cd, dkeys, total = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
            return (time.perf_counter() - t0) * 1e3, dkeys, total

        _, dkeys, total = step()
        keys = device_copy(torch, dkeys, total * 164).view(total, 164)
        desc = keys[:, 36:].contiguous()
        del keys
        report["keys"] = total
        vocabs = {K: make_vocabulary(torch, desc, K, seed=K) for K in sizes}
        settings = [0] + sizes
        rows = {K: {"assign_ms_steps": [], "step_ms_steps": []} for K in settings}
        for K in settings:   # warm-up in every setting
            ctx.set_vocabulary(vocabs[K] if K else None)
            step()
        for _ in range(a.steps):
            for K in settings:
                ctx.set_vocabulary(vocabs[K] if K else None)
                ms, _, tot = step()
                assert tot == total, "counts changed between steps"
                rows[K]["step_ms_steps"].append(ms)
                rows[K]["assign_ms_steps"].append(ctx.assign_ms)
        base = float(np.median(rows[0]["step_ms_steps"]))
        for K in sizes:
            r = rows[K]
            r["assign_ms"] = float(np.median(r["assign_ms_steps"]))
            r["step_ms"] = float(np.median(r["step_ms_steps"]))
            r["step_ms_no_vocabulary"] = base
            r["evals_per_s"] = total * K / (r["assign_ms"] * 1e-3)
            r["fraction_of_i8_peak"] = r["evals_per_s"] * 128 * 2 / I8_DENSE_OPS
            # the baseline: the same keys (packed) and vocabulary; the kernel alone on the packed tensor beside it
            ctx.set_vocabulary(vocabs[K])
            got = torch.empty((total, 2), dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            ctx.assign_words_device(desc.data_ptr(), total, 128, 0, got.data_ptr())
            kernel_ms = ctx.assign_ms
            vdev = torch.from_numpy(vocabs[K]).cuda()
            block = max(256, min(total, (1 << 29) // K))
            check_n = min(total, 4 * block)
            ref, route = torch_route(torch, desc[:check_n], vdev, block)   # (also the warm-up of the torch route)
            mism = int((ref != got[:check_n]).any(dim=1).sum().item())
            times = []
            for _ in range(a.torch_runs):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                full, _ = torch_route(torch, desc, vdev, block)
                e1.record()
                torch.cuda.synchronize()
                times.append(e0.elapsed_time(e1))
            mism_full = int((full != got).any(dim=1).sum().item())
            r["torch"] = {"route": route, "row_block": block, "ms_runs": times, "ms": float(np.median(times)), "kernel_ms": kernel_ms,
                          "rows_checked_first": check_n, "mismatches_first": mism, "mismatches_all": mism_full,
                          "kernel_no_slower": kernel_ms <= float(np.median(times))}
            del vdev, ref, full, got
        report["no_vocabulary"] = {"step_ms_steps": rows[0]["step_ms_steps"], "step_ms": base}
        report["sizes"] = {str(K): rows[K] for K in sizes}
        ctx.set_vocabulary(None)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
