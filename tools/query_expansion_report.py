#!/usr/bin/env python3
"""What query expansion (hesaff_expand_query_device, kernels_expand.h) costs, and how it compares with the same computation written
in torch.

One process, one context at profiling level 1.  Per shape of `--shapes` (E selected candidates of n keys each; a query of
`--query-keys` keys): the rows are made on the device, every candidate is eligible with a map near the identity and its first row
for an anchor, the region is the middle of the candidates' spread (about a sixth of the keys fall into it), and max_rows is 2^18:
the larger shapes keep far more rows than that, so their scatter writes 2^18 rows and skips the tiles behind the cut, as every
call of that size does.  hesaff_get_expand_ms of `--rounds` calls - flags_ms (the flags pass and its scan) and scatter_ms -
alternated with the torch route.

The torch route does the same on the same rows on the same device, for all candidates at once in rank order: the back-projection
and both frames in float32 elementwise operations (no contraction: every operation is its own kernel), the kept mask, and `cat`
of the query with the masked rows, cut to max_rows.  Its output must equal the library's byte for byte: the tool exits with
status 1 where it does not.

bytes_read_per_second is the selected candidates' rows (24 bytes each) over flags_ms, set against read_only_GBs of bench.py's
hbm_probe, run in the same process.

    python tools/query_expansion_report.py [--shapes 10x3000,100x65536,1000x65536] [--rounds 3] [--out report.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_live(torch, x, y, a, b, c):
    r = torch.sqrt(c); q = b / r; t = a - q * q; p = torch.sqrt(t)
    lo, hi = 2.0 ** -20, 2.0 ** 20
    return (c > 0) & (t > 0) & (p >= lo) & (p <= hi) & (r >= lo) & (r <= hi) & (a <= 2.0 ** 40) & (x.abs() <= hi) & (y.abs() <= hi)


def torch_expand(torch, qrows, crows, anchors, roi, max_rows):
    """qrows int32 [nq, 6] and crows int32 [E, n, 6] (the bits of the rows, the candidates in rank order), anchors float32 [E, 7] =
    xq, yq, xd, yd, L11, L21, L22 -> the expanded rows int32 [n_out, 6]"""
    f = crows.view(torch.float32)
    x, y, a, b, c = (f[:, :, k] for k in range(5))
    xq, yq, xd, yd, L11, L21, L22 = (anchors[:, k:k + 1] for k in range(7))
    dx = x - xd; dy = y - yd
    u = dx / L11; t = L21 * u; s = dy - t; v = s / L22
    xn = xq + u; yn = yq + v
    e00 = a * L11 + b * L21; e10 = b * L11 + c * L21; e01 = b * L22; e11 = c * L22
    an = L11 * e00 + L21 * e10; bn = L11 * e01 + L21 * e11; cn = L22 * e11
    kept = torch_live(torch, x, y, a, b, c) & (xn >= roi[0]) & (xn <= roi[2]) & (yn >= roi[1]) & (yn <= roi[3]) & torch_live(torch, xn, yn, an, bn, cn)
    new = torch.stack([xn, yn, an, bn, cn], dim=2).view(torch.int32)
    new = torch.cat([new, crows[:, :, 5:6]], dim=2)
    return torch.cat([qrows, new[kept]])[:max_rows]


def spread(values):
    v = np.asarray(values, np.float64)
    return {"median": float(np.median(v)), "min": float(v.min()), "max": float(v.max())}


def device_rows(torch, gen, n, K, width, height):
    """n live rows on the device as int32 [n, 6]: ellipses with axes around 10 px and a little shear"""
    p = 0.05 + 0.1 * torch.rand(n, generator=gen, device="cuda"); r = 0.05 + 0.1 * torch.rand(n, generator=gen, device="cuda")
    q = 0.04 * (torch.rand(n, generator=gen, device="cuda") - 0.5)
    f = torch.stack([torch.rand(n, generator=gen, device="cuda") * width, torch.rand(n, generator=gen, device="cuda") * height, p * p + q * q, q * r, r * r], dim=1)
    w = torch.randint(0, K, (n, 1), generator=gen, device="cuda", dtype=torch.int32)
    return torch.cat([f.view(torch.int32), w], dim=1).contiguous()


def run(torch, ctx, E, n, nq, K, rounds, read_only_gbs):
    gen = torch.Generator(device="cuda"); gen.manual_seed(E * 131 + n)
    width, height = 3000.0, 2000.0
    roi = (1000.0, 600.0, 2000.0, 1400.0)
    max_rows = 1 << 18
    rng = np.random.RandomState(E)
    tq = device_rows(torch, gen, nq, K, width, height)
    tc = device_rows(torch, gen, E * n, K, width, height)
    out = np.zeros((E, 6), np.int32)
    out[:, 0] = 10 + rng.randint(0, 50, E); out[:, 1] = out[:, 2] = out[:, 0]; out[:, 3] = rng.randint(0, nq, E)
    hyp = np.stack([0.9 + 0.2 * rng.rand(E), 0.1 * (rng.rand(E) - 0.5), 0.9 + 0.2 * rng.rand(E)], axis=1).astype(np.float32)
    order = np.lexsort((np.arange(E), -out[:, 0].astype(np.int64)))
    counts = np.full(E, n, np.int32)
    cap = min(max_rows, nq + E * n)
    t_rows = torch.zeros((cap, 6), dtype=torch.int32, device="cuda"); t_words = torch.zeros(cap, dtype=torch.int32, device="cuda")
    # the torch route's inputs: the candidates in rank order and their anchors
    ranked = tc.view(E, n, 6)[torch.from_numpy(order).cuda()].contiguous()
    qf = tq.view(torch.float32)
    anchors = torch.cat([qf[torch.from_numpy(out[order, 3].astype(np.int64)).cuda(), 0:2], ranked.view(torch.float32)[:, 0, 0:2],
                         torch.from_numpy(hyp[order]).cuda()], dim=1).contiguous()
    torch.cuda.synchronize()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def library():
        return ctx.expand_query_device(tq.data_ptr(), nq, tc.data_ptr(), counts, out, hyp, K, 1, roi, t_rows.data_ptr(), t_words.data_ptr(), max_rows=max_rows)

    def torch_route():
        ev[0].record()
        res = torch_expand(torch, tq, ranked, anchors, roi, max_rows)
        ev[1].record()
        torch.cuda.synchronize()
        return res, ev[0].elapsed_time(ev[1])
    library(); torch_route()   # warm-up of both routes
    flags_ms, scatter_ms, torch_ms = [], [], []
    for _ in range(rounds):
        n_out, info = library()
        ms = ctx.expand_ms
        flags_ms.append(ms[0]); scatter_ms.append(ms[1])
        res, t = torch_route()
        torch_ms.append(t)
    torch.cuda.synchronize()
    equal = bool(n_out == len(res) and torch.equal(t_rows[:n_out], res) and torch.equal(t_words[:n_out], res[:, 5]))
    gbs = E * n * 24 / (np.median(flags_ms) * 1e-3) / 1e9
    return {"selected": E, "keys_per_candidate": n, "query_keys": nq, "kept_total": int(info[:, 2].sum()), "n_out": int(n_out),
            "flags_ms": spread(flags_ms), "scatter_ms": spread(scatter_ms), "torch_ms": spread(torch_ms), "torch_output_equal": equal,
            "flags_bytes_read_GBs": gbs, "read_only_GBs": read_only_gbs, "flags_frac_of_read_only": gbs / read_only_gbs if read_only_gbs else None}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="10x3000,100x65536,1000x65536")
    ap.add_argument("--query-keys", type=int, default=4096)
    ap.add_argument("--words", type=int, default=65536)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--no-probe", action="store_true", help="skip bench.py's hbm_probe")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import hesaff_amd
    probe = None
    if not a.no_probe:
        import bench
        probe = bench.hbm_probe(torch, "cuda:0")
    report = {"library": hesaff_amd.lib_path(), "hbm_probe": probe, "shapes": []}
    p = hesaff_amd.default_params()
    p.max_batch = 1
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        ctx.set_profiling(1)
        for shape in a.shapes.split(","):
            E, n = (int(v) for v in shape.split("x"))
            report["shapes"].append(run(torch, ctx, E, n, a.query_keys, a.words, a.rounds, probe["read_only_GBs"] if probe else None))
            torch.cuda.empty_cache()
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)
    sys.exit(0 if all(s["torch_output_equal"] for s in report["shapes"]) else 1)


if __name__ == "__main__":
    main()
