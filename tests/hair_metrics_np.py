"""The strand metrics of monohair_amd.hairmetrics restated in numpy from their definition (include/mh_pmvo.h, "Strand
metrics"): brute force over all pairs, float64 on the float32 coordinates, + - * / sqrt in the stated order.  Written from
the definition, not from the kernels; the GPU tests demand the same bits."""
import math

import numpy as np


def bounds(thresholds):
    """(r2, c): tau_d * tau_d and cos(tau_a * (pi / 180)) per (metres, degrees) pair"""
    return (np.array([np.float64(d) * np.float64(d) for d, _ in thresholds]),
            np.array([math.cos(np.float64(a) * (math.pi / 180.0)) for _, a in thresholds]))


def _strands(counts, points):
    pts = np.asarray(points, np.float32).reshape(-1, 3)
    off = 0
    for n in counts:
        yield pts[off:off + n]
        off += n
    assert off == pts.shape[0]


def _norm(d):
    return np.sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2])


def cumulative_length(p):
    """L_0 = 0, L_i = L_{i-1} + |p_i - p_{i-1}| (p float64 [n,3])"""
    L = np.zeros(p.shape[0], np.float64)
    for i in range(1, p.shape[0]):
        L[i] = L[i - 1] + _norm(p[i] - p[i - 1])
    return L


def resample(counts, points, step):
    """-> (counts int64 [S], points float32 [m,3])"""
    step = np.float64(step)
    out_counts, out = [], []
    for strand in _strands(counts, points):
        n = strand.shape[0]
        if n == 0:
            out_counts.append(0)
            continue
        p = strand.astype(np.float64)
        L = cumulative_length(p)
        if n < 2 or not L[-1] > 0.0:
            out_counts.append(1)
            out.append(strand[0])
            continue
        m = int(np.floor(L[-1] / step)) + 1
        out_counts.append(m)
        for j in range(m):
            s = np.float64(j) * step
            above = np.nonzero(L[1:] > s)[0]
            i = above[0] if above.size else np.nonzero(L[1:] > L[:-1])[0][-1]
            u = (s - L[i]) / (L[i + 1] - L[i])
            out.append((p[i] + u * (p[i + 1] - p[i])).astype(np.float32))
    return np.array(out_counts, np.int64), np.array(out, np.float32).reshape(-1, 3)


def tangents(counts, points):
    """-> (t float64 [n,3], valid uint8 [n])"""
    ts, vs = [], []
    for strand in _strands(counts, points):
        n = strand.shape[0]
        p = strand.astype(np.float64)
        for i in range(n):
            d = p[min(i + 1, n - 1)] - p[max(i - 1, 0)]
            ln = _norm(d)
            ok = n >= 2 and ln > 0.0
            ts.append(d / ln if ok else np.zeros(3))
            vs.append(1 if ok else 0)
    return np.array(ts, np.float64).reshape(-1, 3), np.array(vs, np.uint8)


def squared_distances(q, t):
    """[nq, nt] float64: (dx*dx + dy*dy) + dz*dz"""
    q, t = np.asarray(q, np.float32).astype(np.float64), np.asarray(t, np.float32).astype(np.float64)
    d2 = q[:, None, 0] - t[None, :, 0]
    d2 *= d2
    for c in (1, 2):          # d2 = dx*dx, then (d2 + dy*dy), then (that + dz*dz)
        d = q[:, None, c] - t[None, :, c]
        d *= d
        d2 += d
    return d2


def match_flags(q_pts, q_tan, q_valid, t_pts, t_tan, t_valid, r2, c, chunk=256):
    """uint8 [nq]: bit k iff the query is valid and some valid target has d2 <= r2[k] and |t . u| >= c[k].  All pairs; the
    blocks of queries go to a few threads (numpy releases the interpreter lock inside its loops)."""
    from concurrent.futures import ThreadPoolExecutor

    q_pts, t_pts = np.asarray(q_pts, np.float32).reshape(-1, 3), np.asarray(t_pts, np.float32).reshape(-1, 3)
    q_tan, t_tan = np.asarray(q_tan, np.float64).reshape(-1, 3), np.asarray(t_tan, np.float64).reshape(-1, 3)
    keep = np.asarray(t_valid) != 0
    t_pts, t_tan = t_pts[keep], t_tan[keep]
    flags = np.zeros(q_pts.shape[0], np.uint8)
    r2max = max(r2)

    def block(a):
        d2 = squared_distances(q_pts[a:a + chunk], t_pts)
        qi, ti = np.nonzero(d2 <= r2max)
        tq, tt = q_tan[a + qi], t_tan[ti]
        dot = np.abs((tq[:, 0] * tt[:, 0] + tq[:, 1] * tt[:, 1]) + tq[:, 2] * tt[:, 2])
        for k in range(len(r2)):
            hit = (d2[qi, ti] <= r2[k]) & (dot >= c[k])
            flags[a + np.unique(qi[hit])] |= np.uint8(1 << k)      # (a block writes its own queries only)

    starts = range(0, q_pts.shape[0], chunk)
    if len(starts) > 1:
        with ThreadPoolExecutor(8) as pool:
            list(pool.map(block, starts))
    else:
        for a in starts:
            block(a)
    flags[np.asarray(q_valid) == 0] = 0
    return flags


def counts_of(flags, valid, K):
    return {"matched": [int(((flags >> k) & 1).sum()) for k in range(K)], "valid": int((valid != 0).sum()),
            "invalid": int((valid == 0).sum())}


def score(pred, gt, thresholds, step=None):
    """-> (counts as monohair_amd.hairmetrics reports them, {"pred": flags, "gt": flags})"""
    r2, c = bounds(thresholds)
    side = {}
    for name, (cnt, pts) in (("pred", pred), ("gt", gt)):
        pts = np.asarray(pts, np.float32).reshape(-1, 3)
        if step is not None:
            cnt, pts = resample(cnt, pts, step)
        side[name] = (pts,) + tangents(cnt, pts)
    flags = {a: match_flags(*side[a], *side[b], r2, c) for a, b in (("pred", "gt"), ("gt", "pred"))}
    return {a: counts_of(flags[a], side[a][2], len(thresholds)) for a in flags}, flags
