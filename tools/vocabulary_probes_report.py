#!/usr/bin/env python3
"""What probing P cells (hesaff_set_vocabulary_probes, kernels_cells.h) costs on the bench's dense image family, and what it buys:
per probe count the three parts of hesaff_get_assign_cells_ms, the share of keys that keep the word of the flat assignment of the same
rows, and the summed dist2 against the flat sum.

tools/vocabulary_cells_report.py's method on the same keys.  One process, one context at profiling level 1.  The keys of B dense
3840 x 2160 band-noise images (hesaff_detect_batch_device) are copied once into a packed [n, 128] tensor.  Per (K, C): C coarse rows
are trained on the keys (`--coarse-iterations` flat iterations), K rows are spread over the keys (row r = key r n // K), sorted into
cells (hesaff_build_vocabulary_cells) and moved by one training iteration inside the cells.  Those K rows are assigned flat once, then
through the layer with every probe count of `--probes`, the counts alternating `--rounds` times after a warm-up of each.  The summed
dist2 must not increase with P: the tool asserts it, and that no key is nearer through the cells than flat.

`--probes 1` runs on a library without the setter as well (HESAFF_AMD_LIB: another commit's build, for a comparison of the default).

    python tools/vocabulary_probes_report.py [--batch 32] [--rounds 3] [--probes 1,2,4,8] [--sizes 65536:256,1048576:1024] [--out report.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def median(v):
    return float(np.median(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--width", type=int, default=3840)
    ap.add_argument("--height", type=int, default=2160)
    ap.add_argument("--rounds", type=int, default=3, help="timed alternations per probe count")
    ap.add_argument("--probes", default="1,2,4,8")
    ap.add_argument("--sizes", default="65536:256,1048576:1024", help="K:C pairs")
    ap.add_argument("--coarse-iterations", type=int, default=2)
    ap.add_argument("--no-flat", action="store_true", help="skip the flat assignment and with it the agreement figures")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    sizes = [tuple(int(v) for v in s.split(":")) for s in a.sizes.split(",")]
    probes = [int(v) for v in a.probes.split(",")]
    import torch
    import hesaff_amd
    from hesaff_amd import synth
    from vocabulary_report import device_copy
    p = hesaff_amd.default_params()
    p.max_batch = a.batch
    report = {"workload": "the packed descriptors of %d x %dx%d dense band-noise images, default parameters; per (K, C) a warm-up of every probe "
                          "count, then %d alternations" % (a.batch, a.width, a.height, a.rounds), "library": hesaff_amd.lib_path(), "sizes": {}}
    with hesaff_amd.HesaffContext(p, device=0) as ctx:
        has_setter = hasattr(ctx.L, "hesaff_set_vocabulary_probes")
        assert has_setter or probes == [1], "this library has no hesaff_set_vocabulary_probes: --probes 1 only"
        imgs = synth.band_noise_batch_torch(a.batch, a.height, a.width, seed=1234, device="cuda", bands=synth.BANDS)
        torch.cuda.synchronize()
        ch, cd, dkeys, total = ctx.detect_batch_device(imgs.data_ptr(), a.batch, a.width, a.height)
        keys = device_copy(torch, dkeys, total * 164).view(total, 164)
        desc = keys[:, 36:].contiguous()
        del keys, imgs
        torch.cuda.synchronize()
        report["keys"] = total
        ctx.set_profiling(1)
        flat_out = torch.empty((total, 2), dtype=torch.int32, device="cuda")
        out = {P: torch.empty((total, 2), dtype=torch.int32, device="cuda") for P in probes}
        for K, C in sizes:
            coarse = ctx.train_vocabulary_device(desc.data_ptr(), total, 128, 0, C, a.coarse_iterations)[0]
            pick = torch.tensor([r * total // K for r in range(K)], device="cuda")
            v0, _, coarse, first = ctx.build_vocabulary_cells(desc[pick].cpu().numpy(), coarse)
            rows = ctx.train_vocabulary_cells_device(desc.data_ptr(), total, 128, 0, v0, coarse, first, 1)[0]
            r = {"cells_with_rows": len(coarse), "rows_per_cell_max": int(np.diff(first.astype(np.int64)).max()), "probes": {}}
            ctx.set_vocabulary(rows)
            if not a.no_flat:
                ctx.assign_words_device(desc.data_ptr(), total, 128, 0, flat_out.data_ptr())
                r["flat_ms"] = ctx.assign_ms
                flat_sum = flat_out[:, 1].double().sum().item()
            ctx.set_vocabulary_cells(coarse, first)

            def assign(P):
                if has_setter:
                    ctx.set_vocabulary_probes(P)
                ctx.assign_words_device(desc.data_ptr(), total, 128, 0, out[P].data_ptr())
                return ctx.assign_ms, ctx.assign_cells_ms
            for P in probes:
                assign(P)   # warm-up
            whole = {P: [] for P in probes}
            parts = {P: [] for P in probes}
            for _ in range(a.rounds):
                for P in probes:
                    ms, pp = assign(P)
                    whole[P].append(ms); parts[P].append(pp)
            sums = []
            for P in probes:
                q = {"assign_ms": median(whole[P]), "assign_ms_rounds": whole[P], "coarse_ms": median([x[0] for x in parts[P]]),
                     "group_ms": median([x[1] for x in parts[P]]), "fine_ms": median([x[2] for x in parts[P]])}
                sums.append(out[P][:, 1].double().sum().item())
                if not a.no_flat:
                    q["share_of_keys_with_the_flat_word"] = int((out[P][:, 0] == flat_out[:, 0]).sum().item()) / total
                    q["dist2_sum_ratio_over_flat"] = sums[-1] / flat_sum
                    assert bool((out[P][:, 1] >= flat_out[:, 1]).all().item()), "a key is nearer through %d probes than flat" % P
                r["probes"][str(P)] = q
            order = np.argsort(probes, kind="stable")
            assert all(sums[order[i + 1]] <= sums[order[i]] for i in range(len(order) - 1)), "the summed dist2 increases with P: %s" % sums
            if has_setter:
                ctx.set_vocabulary_probes(1)
            ctx.set_vocabulary(None)
            report["sizes"]["%d:%d" % (K, C)] = r
            print(json.dumps({"%d:%d" % (K, C): r}), flush=True)
    print(json.dumps(report))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(report, f, indent=1)


if __name__ == "__main__":
    main()
