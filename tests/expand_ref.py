"""Query expansion of include/hesaff_amd.h (hesaff_expand_query) in numpy float32: the definition, not an implementation.
Elementwise + - * / on np.float32 arrays are the IEEE binary32 operations the definition names; comparisons with NaN are false."""
import numpy as np

from tests import verify_ref

F = np.float32


def select(out, min_inliers, max_images):
    """verify_out [R, 6] -> the selected candidates in rank order (inliers descending, r ascending)"""
    inl = np.asarray(out)[:, 0].astype(np.int64)
    eligible = np.nonzero(inl >= min_inliers)[0]
    return eligible[np.lexsort((eligible, -inl[eligible]))][:max_images]


def back_project(rows, anchor_q, anchor_d, L, roi):
    """rows of one candidate -> (the rows in the query's frame, live bool [n], kept bool [n])"""
    L11, L21, L22 = (F(v) for v in L)
    x, y, a, b, c = (rows[f].astype(F) for f in "xyabc")
    new = rows.copy()
    with np.errstate(all="ignore"):
        dx = x - F(anchor_d["x"]); dy = y - F(anchor_d["y"])
        u = dx / L11; t = L21 * u; s = dy - t; v = s / L22
        new["x"] = F(anchor_q["x"]) + u; new["y"] = F(anchor_q["y"]) + v
        e00 = a * L11 + b * L21; e10 = b * L11 + c * L21; e01 = b * L22; e11 = c * L22
        new["a"] = L11 * e00 + L21 * e10; new["b"] = L11 * e01 + L21 * e11; new["c"] = L22 * e11
        live = verify_ref.frames(rows)[1]
        inside = (new["x"] >= F(roi[0])) & (new["x"] <= F(roi[2])) & (new["y"] >= F(roi[1])) & (new["y"] <= F(roi[3]))
    return new, live, live & inside & verify_ref.frames(new)[1]


def expand(q, cands, out, hyp, min_inliers, max_images, roi, max_rows=2 ** 18, qsigs=None, csigs=None):
    """-> (rows, words int32, sigs or None, info int32 [R, 4]); the caller passes eligible candidates that are well-formed"""
    info = np.zeros((len(cands), 4), np.int32); info[:, 0] = -1
    parts, sparts, room = [q], [qsigs], max_rows - len(q)
    for s, r in enumerate(select(out, min_inliers, max_images)):
        new, live, kept = back_project(cands[r], q[out[r][3]], cands[r][out[r][4]], hyp[r], roi)
        take = np.nonzero(kept)[0][:max(room, 0)]
        info[r] = (s, live.sum(), kept.sum(), len(take)); room -= len(take)
        parts.append(new[take]); sparts.append(None if csigs is None else csigs[r][take])
    rows = np.concatenate(parts)
    return rows, rows["word"].astype(np.int32), (None if qsigs is None else np.concatenate(sparts)), info
