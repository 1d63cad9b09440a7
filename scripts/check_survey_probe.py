#!/usr/bin/env python3
"""Check the CPU oracle against what SURVEY.md Appendix C recorded from the COMPILED reference.

The survey compiled the five reference sources unmodified against a throw-away OpenCV shim and
wrote down, for reproducible inputs (App. C.3), the md5 of every input PGM and the candidate /
Hessian-keypoint / descriptor counts of the reference's run (App. C.4, C.6, C.9).  Nothing of
that harness was kept; those recorded numbers are the survey's own trace of the reference's
behaviour.  (The reference is rebuilt against oracle/cvshim/ since, and tests/test_reference.py
compares the oracle with that build directly; this script stays as the check against the record.)
This script regenerates the inputs (the md5 prefixes must match App. C.3), runs
oracle/libhesaff_oracle.so on them and compares the counts.  FMA contraction alone moves these
counts (App. C.5: 4763 -> 4760 at VGA), so equal counts at three sizes are strong evidence that
the restatement follows the reference to the level of float operation order -- evidence against
survey-recorded outputs of a shimmed build, not a pin by reference-held vectors.

Usage: python scripts/check_survey_probe.py [--sizes vga fhd uhd small] [--hash-columns]
"""
import argparse
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

BANDS5 = ((1.5, 40.0), (3.0, 40.0), (6.0, 50.0), (12.0, 60.0), (24.0, 60.0))
BANDS3 = ((1.5, 40.0), (3.0, 40.0), (6.0, 50.0))

# name -> (height, width, seed, bands, PGM md5 prefix or None,
#                                  candidates (localizeKeypoint calls), Hessian keypoints, descriptors)
PROBE = {
    "vga": (480, 640, 1234, BANDS5, "74f828b5", 5281, 4763, 4183),
    "fhd": (1080, 1920, 1234, BANDS5, "6092dc4c", 31099, 26126, 24743),
    "uhd": (2160, 3840, 1234, BANDS5, "6c69f10c", 128471, 109187, 106302),
}
# App. C.9: fixture-sized runs, ONE default_rng(7) generating 131x77 and then 96x96: (height, width, Hessian, descriptors)
SMALL_PAIR = ((77, 131, 175, 88), (96, 96, 158, 73))
# md5 prefixes App. C.4 recorded for the reference's .hesaff.sift files (stock glibc 2.35)
SIFT_MD5 = {"vga": "e004ba88", "fhd": "d1e406df", "uhd": "f7893824"}


def probe_image(height, width, seed, bands):
    """App. C.3 recipe: default_rng(seed); sum of amp * gaussian_filter(standard_normal -> f32, sigma) / std,
    float32 accumulation, min-max stretch to 0..255, truncation to uint8."""
    return _probe_from_rng(np.random.default_rng(seed), height, width, bands)


def _probe_from_rng(rng, height, width, bands):
    from scipy.ndimage import gaussian_filter

    acc = np.zeros((height, width), np.float32)
    for sigma, amp in bands:
        n = rng.standard_normal((height, width)).astype(np.float32)
        g = gaussian_filter(n, sigma)
        acc = acc + amp * g / g.std()
    lo, hi = acc.min(), acc.max()
    return np.clip(np.floor((acc - lo) / (hi - lo) * 255.0), 0, 255).astype(np.uint8)


def small_pair():
    from tests import _oracle

    rng = np.random.default_rng(7)
    out = []
    for h, w, n_hess, n_desc in SMALL_PAIR:
        img = _probe_from_rng(rng, h, w, BANDS3)
        o = _oracle.OracleRun(_oracle.gray_from_u8(img))
        out.append({"name": "%dx%d" % (w, h), "hessian": int(o.n_hessian), "descriptors": int(o.n_keys), "expected": (n_hess, n_desc),
                    "ok": (o.n_hessian, o.n_keys) == (n_hess, n_desc)})
    return out


def pgm_bytes(img):
    return b"P5\n%d %d\n255\n" % (img.shape[1], img.shape[0]) + img.tobytes()


def run_one(name, hash_columns=False):
    from tests import _oracle

    h, w, seed, bands, md5, n_cand, n_hess, n_desc = PROBE[name]
    img = probe_image(h, w, seed, bands)
    got_md5 = hashlib.md5(pgm_bytes(img)).hexdigest()
    o = _oracle.OracleRun(_oracle.gray_from_u8(img))
    res = {"name": name, "pgm_md5": got_md5, "pgm_md5_expected": md5, "candidates": int(o.n_candidates), "hessian": int(o.n_hessian),
           "descriptors": int(o.n_keys), "expected": (n_cand, n_hess, n_desc)}
    res["pgm_md5_reproduced"] = got_md5.startswith(md5)
    res["ok"] = (o.n_candidates, o.n_hessian, o.n_keys) == (n_cand, n_hess, n_desc)
    if hash_columns:
        text = o.export_text()
        res["sift_md5"] = hashlib.md5(text).hexdigest()
        res["sift_md5_recorded"] = SIFT_MD5.get(name)
        res["sift_md5_reproduced"] = res["sift_md5"].startswith(SIFT_MD5.get(name, "-"))
        rows = text.split(b"\n")[2:-1]
        xy = b"\n".join(b" ".join(r.split(b" ")[:2]) for r in rows)
        abc = b"\n".join(b" ".join(r.split(b" ")[2:5]) for r in rows)
        desc = b"\n".join(b" ".join(r.split(b" ")[5:]) for r in rows)
        res["md5_xy_columns"] = hashlib.md5(xy).hexdigest()
        res["md5_abc_columns"] = hashlib.md5(abc).hexdigest()
        res["md5_descriptor_columns"] = hashlib.md5(desc).hexdigest()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", nargs="*", default=["small", "vga", "fhd", "uhd"])
    ap.add_argument("--hash-columns", action="store_true")
    a = ap.parse_args()
    bad = 0
    for n in a.sizes:
        for r in (small_pair() if n == "small" else [run_one(n, a.hash_columns)]):
            print(r)
            bad += 0 if r["ok"] else 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
