#!/usr/bin/env python3
"""Writes tests/golden/ref_*.npz and the "reference" block of manifest.json.  Run from the repo root, after
`make -C oracle ref`:  python tests/golden/make_ref_golden.py

WHAT THESE FIXTURES ARE: output of the COMPILED reference (oracle/_ref/ref_driver and oracle/_ref/hesaff_ref: the reference's
sources, unmodified, against the OpenCV stand-in oracle/cvshim/), on tests/golden/band_160x120.pgm.  The repo's own oracle is not
asked for a single number here; it only labels the captured planes with (octave, level), and that label is then asserted bit for
bit.  tests/test_reference.py checks that the oracle reproduces them (CPU) and that the HIP path does (GPU).

  ref_<set>.npz          records[RECORD] of one parameter set of tests/_reference.PARAM_SETS
  ref_float.npz          records of the float plane  grey * 1.37 - 300.75  (float32), default parameters
  ref_planes_o<k>.npz    the blur planes of octave k that the detector handed to its keypoint callback (default run)
  ref_foreign.npz        seeded points and shapes that no detector produced, and the reference's record for each
  manifest.json          "reference": counts and the md5 of the record bytes per fixture, and the md5 of hesaff_ref's
                         .hesaff.sift for the five golden PGMs (byte-identical to the committed *.hesaff.sift)
"""
import hashlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from tests import _reference as R  # noqa: E402

FOREIGN_SEED = 47
FOREIGN_PER_PLANE = 14
MIN_DESCRIBED = 30   # a parameter set that leaves fewer on band_160x120 is made on R.sparse_image() instead


def fate_counts(rec):
    n = np.bincount(rec["fate"], minlength=3)
    return {"records": int(len(rec)), "not_converged": int(n[0]), "rejected": int(n[1]), "described": int(n[2])}


def param_fixtures(driver):
    """-> {fixture name: (arrays, manifest entry)} for every parameter set"""
    out = {}
    grey = R.grey_of(R.fixture_image())
    for name, kw in R.PARAM_SETS.items():
        rec, image = R.run_driver(driver, grey, kw), "band_160x120"
        if (rec["fate"] == R.DESCRIBED).sum() < MIN_DESCRIBED:
            rec, image = R.run_driver(driver, R.grey_of(R.sparse_image()), kw), "sparse_200x260"
        assert (rec["fate"] == R.DESCRIBED).sum() >= MIN_DESCRIBED, name
        out[name] = ({"records": rec}, dict(fate_counts(rec), image=image, params=kw, records_md5=R.records_md5(rec)))
    return out


def float_fixture(driver):
    rec = R.run_driver(driver, R.float_fixture_plane())
    return {"records": rec}, dict(fate_counts(rec), image="band_160x120 * 1.37 - 300.75 (float32)", records_md5=R.records_md5(rec))


def labelled_planes(driver):
    """The default run's captured planes with the (octave, level) each is -> (records, [(octave, level, pd, plane)])"""
    from tests import _oracle
    grey = R.grey_of(R.fixture_image())
    rec, planes = R.run_driver(driver, grey, planes=True)
    o = _oracle.OracleRun(grey, keep_planes=True)
    _, labels = R.oracle_records(_oracle, grey, run=o)
    assert len(labels) == len(planes)
    out = []
    for (octave, level), (pd, plane) in zip(labels, planes):
        assert pd == 2.0 ** octave and plane.tobytes() == o.plane(octave, 0, level).tobytes(), (octave, level)
        out.append((octave, level, pd, plane))
    return rec, out


def plane_fixtures(planes):
    out = {}
    for octave in sorted({p[0] for p in planes}):
        mine = [p for p in planes if p[0] == octave]
        arrays = {"levels": np.array([p[1] for p in mine], np.int32), "pixelDistance": np.float32(mine[0][2])}
        for _, level, _, plane in mine:
            arrays["L%d" % level] = plane
        md5 = hashlib.md5(b"".join(p[3].tobytes() for p in mine)).hexdigest()
        out["planes_o%d" % octave] = (arrays, {"octave": octave, "levels": [int(p[1]) for p in mine], "rows": int(mine[0][3].shape[0]),
                                               "cols": int(mine[0][3].shape[1]), "planes_md5": md5})
    return out


def foreign_fixture(driver, planes):
    """Points and shapes built like tests/test_describe_regions.foreign_records, on the planes the default run captured."""
    from tests.test_describe_regions import foreign_records
    img = R.fixture_image()
    grey = R.grey_of(img)
    H, W = img.shape
    index = {(p[0], p[1]): k for k, p in enumerate(planes)}
    n_oct = 1 + max(o for o, _ in index)

    def build(shapes):
        reg = foreign_records(H, W, n_oct, 1.0, FOREIGN_SEED + int(shapes), per_plane=FOREIGN_PER_PLANE, shapes=shapes)
        return reg[[(o, l) in index for o, l in zip(reg["octave"].tolist(), reg["level"].tolist())]]

    reg = build(False)
    points = np.zeros(len(reg), np.dtype(R.POINT_IN.descr + [("octave", "<i4"), ("level", "<i4")]))
    for k in ("x", "y", "s", "octave", "level"):
        points[k] = reg[k]
    points["plane"] = [index[ol] for ol in zip(reg["octave"].tolist(), reg["level"].tolist())]
    pin = np.zeros(len(points), R.POINT_IN)
    for k in R.POINT_IN.names:
        pin[k] = points[k]
    point_records = R.run_driver(driver, grey, points=pin)

    reg = build(True)
    shapes = np.zeros(len(reg), R.SHAPE_IN)
    for k in ("x", "y", "s"):
        shapes[k] = reg[k]
    shapes["U"] = np.stack([reg[k] for k in ("a11", "a12", "a21", "a22")], 1)
    shape_records = R.run_driver(driver, grey, shapes=shapes)

    pc, sc = fate_counts(point_records), fate_counts(shape_records)
    assert min(pc["not_converged"], pc["rejected"], pc["described"]) >= 20, pc
    assert min(sc["rejected"], sc["described"]) >= 20 and sc["not_converged"] == 0, sc
    arrays = {"points": points, "point_records": point_records, "shapes": shapes, "shape_records": shape_records}
    return arrays, {"points": dict(pc, records_md5=R.records_md5(point_records)),
                    "shapes": dict(sc, records_md5=R.records_md5(shape_records))}


def sift_entries(hesaff_ref):
    out = {}
    for name in R.GOLDEN_PGMS:
        n_hess, n_desc, text = R.run_hesaff_ref(hesaff_ref, os.path.join(R.GOLD, name + ".pgm"))
        committed = open(os.path.join(R.GOLD, name + ".hesaff.sift"), "rb").read()
        assert text == committed, "%s: hesaff_ref's file differs from the committed %s.hesaff.sift" % (name, name)
        out[name] = {"hessian": n_hess, "descriptors": n_desc, "sift_md5": hashlib.md5(text).hexdigest(),
                     "same_bytes_as": name + ".hesaff.sift"}
    return out


def generate(driver, hesaff_ref):
    """-> ({fixture name: arrays}, the manifest's "reference" block); writes nothing"""
    fixtures = param_fixtures(driver)
    fixtures["float"] = float_fixture(driver)
    _, planes = labelled_planes(driver)
    fixtures.update(plane_fixtures(planes))
    fixtures["foreign"] = foreign_fixture(driver, planes)
    block = {"made_by": "oracle/_ref/ref_driver and oracle/_ref/hesaff_ref (tests/golden/make_ref_golden.py)",
             "fixtures": {"ref_%s.npz" % k: v[1] for k, v in fixtures.items()},
             "hesaff_ref_sift": sift_entries(hesaff_ref)}
    return {k: v[0] for k, v in fixtures.items()}, block


def main():
    driver, hesaff_ref = (os.path.join(R.REF_OUT, n) for n in ("ref_driver", "hesaff_ref"))
    arrays, block = generate(driver, hesaff_ref)
    largest = os.path.getsize(os.path.join(R.GOLD, "probe_vga.pgm"))
    for name, a in arrays.items():
        np.savez_compressed(R.fixture_path(name), **a)
        size = os.path.getsize(R.fixture_path(name))
        assert size < largest, (name, size)
        print("%-28s %7d bytes  %s" % (os.path.basename(R.fixture_path(name)), size, block["fixtures"]["ref_%s.npz" % name]))
    path = os.path.join(R.GOLD, "manifest.json")
    with open(path) as f:
        manifest = json.load(f)
    manifest["reference"] = block   # every other key stays as it is
    with open(path, "w") as f:
        json.dump(manifest, f, indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
