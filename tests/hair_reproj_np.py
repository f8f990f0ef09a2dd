"""The capture-agreement rule of include/mh_pmvo.h ("Capture agreement") restated in numpy from the header text alone: what the
tests hold csrc/hairreproj.hip to, count for count.  Like tests/hair_capture_np.py it starts from the per-vertex (row, col,
z255, valid) of one view and does everything after it in float64 on those float32 values, one numpy operation per operation
of the rule.  The front plane is pass A of the capture rule, taken from that restatement."""
import numpy as np

import hair_capture_np as hc

MAX_N = 8192
MASK_MIN = 52
COLS = 4          # visible, on hair, confident, dropped segments; then one column per bound


def bounds_of(angles_deg):
    """what the Python side hands over: 4096 * cos(2 * angle), float64"""
    return np.array([4096.0 * np.cos(2.0 * (float(a) * (np.pi / 180.0))) for a in angles_deg], np.float64)


def conf_min_code(conf_threshold):
    """the smallest code whose decoded confidence (float32 of code / 255) is above float32(threshold); 256: none"""
    t = np.float32(conf_threshold)
    for c in range(256):
        if np.float32(np.uint8(c) / 255.0) > t:
            return c
    return 256


def segments(vert, valid, counts):
    """-> per kept segment the float64 arrays r0, c0, z0, dr, dc, dz, length, the int64 n, qc, qs and its strand; and the
    strand of every dropped segment"""
    vert = np.asarray(vert, np.float32).reshape(-1, 3)
    valid = np.asarray(valid).reshape(-1) != 0
    counts = np.asarray(counts, np.int64).reshape(-1)
    assert counts.sum() == vert.shape[0] == valid.shape[0]
    strand_of = np.repeat(np.arange(counts.shape[0], dtype=np.int64), counts)
    last = np.zeros(vert.shape[0], bool)
    last[np.cumsum(counts)[counts > 0] - 1] = True
    a = np.nonzero(~last)[0]
    a = a[valid[a] & valid[a + 1]]
    v = vert.astype(np.float64)
    r0, c0, z0 = v[a, 0], v[a, 1], v[a, 2]
    dr, dc, dz = v[a + 1, 0] - r0, v[a + 1, 1] - c0, v[a + 1, 2] - z0
    n = np.maximum(1.0, np.ceil(np.maximum(np.abs(dr), np.abs(dc))))
    keep = ~(n > MAX_N)
    dropped_strands = strand_of[a[~keep]]
    a, r0, c0, z0, dr, dc, dz, n = (x[keep] for x in (a, r0, c0, z0, dr, dc, dz, n))
    length = np.sqrt(dr * dr + dc * dc)
    with np.errstate(invalid="ignore", divide="ignore"):
        ur, uc = dr / length, dc / length
        c2 = uc * uc - ur * ur
        s2 = -2.0 * (uc * ur)
        qc = np.where(length > 0, np.rint(4096.0 * c2), 0.0)
        qs = np.where(length > 0, np.rint(4096.0 * s2), 0.0)
    return dict(r0=r0, c0=c0, z0=z0, dr=dr, dc=dc, dz=dz, length=length, n=n.astype(np.int64), qc=qc.astype(np.int64),
                qs=qs.astype(np.int64), strand=strand_of[a]), dropped_strands


def support(vert, valid, counts, H, W, ori_u8, conf_u8, mask_u8, conf_min, bounds, radius=1, tol=0.25, depth0=None,
            table=None, zmin=None):
    """One view -> dict(strand int64 [S, 4 + K], view int64 [4 + K], silhouette int64 [3], zmin float32 [H,W])"""
    counts = np.asarray(counts, np.int64).reshape(-1)
    bounds = np.asarray(bounds, np.float64).reshape(-1)
    K, S = bounds.shape[0], counts.shape[0]
    assert 1 <= K <= 8
    T = (hc.code_table() if table is None else np.asarray(table, np.float32)).astype(np.float64)
    ori, conf, mask = (np.asarray(x, np.uint8).reshape(-1) for x in (ori_u8, conf_u8, mask_u8))
    if zmin is None:
        zmin = hc.capture(vert, valid, counts, H, W, radius=radius, tol=tol, depth0=depth0)["zmin"]
    zmin = np.asarray(zmin, np.float32).reshape(-1)
    seg, dropped_strands = segments(vert, valid, counts)
    out = np.zeros((S, COLS + K), np.int64)
    np.add.at(out[:, 3], dropped_strands, 1)
    # the samples
    n = seg["n"]
    sidx = np.repeat(np.arange(n.shape[0], dtype=np.int64), n)
    j = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    t = (j.astype(np.float64) + 0.5) / n[sidx].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cr = np.rint(seg["r0"][sidx] + t * seg["dr"][sidx])
        cc = np.rint(seg["c0"][sidx] + t * seg["dc"][sidx])
        zf = (seg["z0"][sidx] + t * seg["dz"][sidx]).astype(np.float32)
    judged = np.isfinite(zf) & (cr >= 0) & (cr < H) & (cc >= 0) & (cc < W)
    cr, cc, zf, sidx = cr[judged].astype(np.int64), cc[judged].astype(np.int64), zf[judged], sidx[judged]
    p = cr * W + cc
    front = zmin[p] + np.float32(tol)
    assert front.dtype == np.float32
    visible = zf <= front
    if depth0 is not None:
        visible &= zf <= np.asarray(depth0, np.float32).reshape(-1)[p]
    on_hair = visible & (mask[p] >= MASK_MIN)
    code = ori[p].astype(np.int64)
    confident = on_hair & (conf[p].astype(np.int64) >= int(conf_min)) & (code < 180)
    tc = np.where(code < 180, code, 0)
    value = seg["qc"][sidx].astype(np.float64) * T[tc, 0] + seg["qs"][sidx].astype(np.float64) * T[tc, 1]
    has_dir = seg["length"][sidx] > 0
    st = seg["strand"][sidx]
    np.add.at(out[:, 0], st[visible], 1)
    np.add.at(out[:, 1], st[on_hair], 1)
    np.add.at(out[:, 2], st[confident], 1)
    for k in range(K):
        np.add.at(out[:, COLS + k], st[confident & has_dir & (value >= bounds[k])], 1)
    pred, obs = np.isfinite(zmin), mask >= MASK_MIN
    sil = np.array([(pred & obs).sum(), (pred & ~obs).sum(), (~pred & obs).sum()], np.int64)
    return dict(strand=out, view=out.sum(0), silhouette=sil, zmin=zmin.reshape(H, W))


def prune_mask(counts_rows, min_cover=0.5, min_agree=0.5, angle_index=-1, min_visible=1, drop_unseen=False):
    """the keep rule of prune_strands on counter rows [S, 4 + K], one strand at a time"""
    keep = []
    for row in np.asarray(counts_rows, np.int64).reshape(-1, np.shape(counts_rows)[-1]):
        vis, hair, confd = int(row[0]), int(row[1]), int(row[2])
        agrees = int(row[COLS:][angle_index])
        if vis < min_visible:
            keep.append(not drop_unseen)
        else:
            keep.append(float(hair) >= float(min_cover) * float(vis) and float(agrees) >= float(min_agree) * float(confd))
    return np.array(keep, bool)
