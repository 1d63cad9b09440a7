"""Spatial verification of include/hesaff_amd.h (hesaff_verify_matches) in numpy float32: the definition, not an implementation.
Elementwise + - * / sqrt on np.float32 arrays are the IEEE binary32 operations the definition names; comparisons with NaN are false."""
import numpy as np

F = np.float32
LO, HI = F(2.0 ** -20), F(2.0 ** 20)


def frames(rows):
    """rows (structured: x, y, a, b, c, word) -> (float32 [n, 5] = x, y, p, q, r; live bool [n])"""
    x, y, a, b, c = (rows[f].astype(F) for f in "xyabc")
    with np.errstate(all="ignore"):
        r = np.sqrt(c); q = b / r; t = a - q * q; p = np.sqrt(t)
        live = (c > 0) & (t > 0) & (p >= LO) & (p <= HI) & (r >= LO) & (r <= HI) & (a <= F(2.0 ** 40)) & (np.abs(x) <= HI) & (np.abs(y) <= HI)
    return np.stack([x, y, p, q, r], axis=1), live


def pairs(qrows, crows, P):
    """-> (found, used pairs int32 [M, 2] = (i, j) in the order (j, i), inert keys of the candidate)"""
    fq, lq = frames(qrows)
    fc, lc = frames(crows)
    wq, wc = qrows["word"].astype(np.int64), crows["word"].astype(np.int64)
    tfc = dict(zip(*(v.tolist() for v in np.unique(wc[lc], return_counts=True))))
    groups = {}   # word -> the live query keys with it, ascending
    for i in np.nonzero(lq)[0]:
        groups.setdefault(int(wq[i]), []).append(int(i))
    out = [(i, int(j)) for j in np.nonzero(lc)[0] if 0 < len(groups.get(int(wc[j]), ())) * tfc[int(wc[j])] <= P for i in groups[int(wc[j])]]
    return len(out), np.array(out[:4096], np.int32).reshape(-1, 2), int((~lc).sum())


def inliers(corr, tol):
    """corr float32 [M, 10] = xq, yq, pq, qq, rq, xd, yd, pd, qd, rd -> (inl int32 [M], best h or -1, L float32 [M, 3])"""
    corr = np.asarray(corr, F).reshape(-1, 10)
    xq, yq, pq, qq, rq, xd, yd, pd, qd, rd = (corr[:, k] for k in range(10))
    with np.errstate(all="ignore"):
        L11 = pq / pd; L22 = rq / rd; L21 = (qq - qd * L11) / rd
        dx = xq[None, :] - xq[:, None]; dy = yq[None, :] - yq[:, None]            # [h, k]
        u = L11[:, None] * dx; v = L21[:, None] * dx + L22[:, None] * dy
        ex = (xd[:, None] + u) - xd[None, :]; ey = (yd[:, None] + v) - yd[None, :]
        e2 = ex * ex + ey * ey
        inl = (e2 <= F(tol) * F(tol)).sum(axis=1).astype(np.int32)
    return inl, (int(np.argmax(inl)) if len(inl) else -1), np.stack([L11, L21, L22], axis=1)


def verify(qrows, cands, P, tol):
    """-> (out int32 [R, 6], hyp float32 [R, 3], order int32 [R], pair lists, query inert keys)"""
    fq, lq = frames(qrows)
    out, hyp, lists = np.zeros((len(cands), 6), np.int32), np.zeros((len(cands), 3), F), []
    for r, crows in enumerate(cands):
        found, pr, inert = pairs(qrows, crows, P)
        fc, _ = frames(crows)
        inl, h, L = inliers(np.concatenate([fq[pr[:, 0]], fc[pr[:, 1]]], axis=1), tol)
        out[r] = (inl[h], len(pr), found, pr[h, 0], pr[h, 1], inert) if h >= 0 else (0, 0, found, -1, -1, inert)
        hyp[r] = L[h] if h >= 0 else 0
        lists.append(pr)
    order = np.lexsort((np.arange(len(cands)), -out[:, 0].astype(np.int64))).astype(np.int32)
    return out, hyp, order, lists, int((~lq).sum())
