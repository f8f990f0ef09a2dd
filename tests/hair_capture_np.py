"""The hair-capture rule of include/mh_pmvo.h ("Hair capture") restated in numpy from the header text alone: what the tests
hold csrc/haircapture.hip to, bit for bit.  It starts from the per-vertex (row, col, z255, valid) of one view -- the
projection is PMVO's own and is held to mh_project_points separately -- and does everything after it in float64 on those
float32 values, one numpy operation per operation of the rule."""
import numpy as np

MAX_N = 8192


def code_table():
    """T[k] = float32 (cos 2 theta_k, sin 2 theta_k), theta_k = k degrees: the table the resolve step is handed"""
    th = np.arange(180, dtype=np.float64) * (np.pi / 180.0)
    return np.stack([np.cos(2.0 * th), np.sin(2.0 * th)], -1).astype(np.float32)


def segment_list(vert, valid, counts):
    """-> dict of per-segment float64 arrays (r0, c0, z0, dr, dc, dz), n, qc, qs (int64) of the kept segments, and `dropped`"""
    vert = np.asarray(vert, np.float32).reshape(-1, 3)
    valid = np.asarray(valid).reshape(-1) != 0
    counts = np.asarray(counts, np.int64).reshape(-1)
    assert counts.sum() == vert.shape[0] == valid.shape[0]
    last = np.zeros(vert.shape[0], bool)
    last[np.cumsum(counts)[counts > 0] - 1] = True
    a = np.nonzero(~last)[0]
    a = a[valid[a] & valid[a + 1]]
    v = vert.astype(np.float64)
    r0, c0, z0 = v[a, 0], v[a, 1], v[a, 2]
    dr, dc, dz = v[a + 1, 0] - r0, v[a + 1, 1] - c0, v[a + 1, 2] - z0
    n = np.maximum(1.0, np.ceil(np.maximum(np.abs(dr), np.abs(dc))))
    keep = ~(n > MAX_N)
    dropped = int((~keep).sum())
    r0, c0, z0, dr, dc, dz, n = (x[keep] for x in (r0, c0, z0, dr, dc, dz, n))
    length = np.sqrt(dr * dr + dc * dc)
    with np.errstate(invalid="ignore", divide="ignore"):
        ur, uc = dr / length, dc / length
        c2 = uc * uc - ur * ur
        s2 = -2.0 * (uc * ur)
        qc = np.where(length > 0, np.rint(4096.0 * c2), 0.0)
        qs = np.where(length > 0, np.rint(4096.0 * s2), 0.0)
    return dict(r0=r0, c0=c0, z0=z0, dr=dr, dc=dc, dz=dz, n=n.astype(np.int64), qc=qc.astype(np.int64),
                qs=qs.astype(np.int64), dropped=dropped)


def fragments(seg, H, W, radius, depth0=None):
    """-> (pixel index int64 [F], zf float32 [F], segment index int64 [F]) of every fragment that survives the image and the
    occluder"""
    n = seg["n"]
    m = n.shape[0]
    sidx = np.repeat(np.arange(m, dtype=np.int64), n)
    first = np.cumsum(n) - n
    j = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(first, n)
    t = (j.astype(np.float64) + 0.5) / n[sidx].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cr = np.rint(seg["r0"][sidx] + t * seg["dr"][sidx]).astype(np.int64)
        cc = np.rint(seg["c0"][sidx] + t * seg["dc"][sidx]).astype(np.int64)
        zf = (seg["z0"][sidx] + t * seg["dz"][sidx]).astype(np.float32)
    fin = np.isfinite(zf)
    cr, cc, zf, sidx = cr[fin], cc[fin], zf[fin], sidx[fin]
    off = np.arange(-radius, radius + 1, dtype=np.int64)
    dy, dx = [g.reshape(-1) for g in np.meshgrid(off, off, indexing="ij")]
    r = cr[:, None] + dy[None, :]
    c = cc[:, None] + dx[None, :]
    inside = (r >= 0) & (r < H) & (c >= 0) & (c < W)
    p = (r * W + c)[inside]
    z = np.broadcast_to(zf[:, None], r.shape)[inside]
    s = np.broadcast_to(sidx[:, None], r.shape)[inside]
    if depth0 is not None:
        d0 = np.asarray(depth0, np.float32).reshape(-1)
        keep = ~(z > d0[p])
        p, z, s = p[keep], z[keep], s[keep]
    return p, z, s


def capture(vert, valid, counts, H, W, radius=1, tol=0.25, depth0=None, table=None, n_full=None):
    """One view -> dict(depth float32, ori_u8, conf_u8, mask_u8, zmin float32, cnt int32, c2, s2 int64 -- all [H,W] -- and
    dropped)"""
    table = code_table() if table is None else np.asarray(table, np.float32)
    n_full = 2 * radius + 1 if n_full is None else int(n_full)
    seg = segment_list(vert, valid, counts)
    p, z, s = fragments(seg, H, W, radius, depth0)
    npix = H * W
    zmin = np.full(npix, np.inf, np.float32)
    np.minimum.at(zmin, p, z)                                   # pass A
    counted = z <= zmin[p] + np.float32(tol)                    # pass B (a float32 addition)
    assert (zmin[p] + np.float32(tol)).dtype == np.float32
    p, s = p[counted], s[counted]
    cnt = np.bincount(p, minlength=npix).astype(np.int32)
    c2 = np.zeros(npix, np.int64)
    s2 = np.zeros(npix, np.int64)
    np.add.at(c2, p, seg["qc"][s])
    np.add.at(s2, p, seg["qs"][s])
    # resolve
    T = table.astype(np.float64)
    C, S = c2.astype(np.float64), s2.astype(np.float64)
    score = C[:, None] * T[None, :, 0] + S[:, None] * T[None, :, 1]
    ori = np.argmax(score, axis=1)                              # the first maximum
    ori[(cnt == 0) | ((c2 == 0) & (s2 == 0))] = 0
    with np.errstate(invalid="ignore", divide="ignore"):
        coh = np.sqrt(C * C + S * S) / (4096.0 * cnt.astype(np.float64))
        dens = np.minimum(1.0, cnt.astype(np.float64) / float(n_full))
        conf = np.minimum(255.0, np.floor((255.0 * coh) * dens + 0.5))
    conf = np.where(cnt > 0, conf, 0.0)
    back = np.full(npix, 255.0, np.float32) if depth0 is None else np.asarray(depth0, np.float32).reshape(-1)
    depth = np.where(cnt > 0, zmin, back).astype(np.float32)
    sh = (H, W)
    return dict(depth=depth.reshape(sh), ori_u8=ori.astype(np.uint8).reshape(sh), conf_u8=conf.astype(np.uint8).reshape(sh),
                mask_u8=np.where(cnt > 0, 255, 0).astype(np.uint8).reshape(sh), zmin=zmin.reshape(sh), cnt=cnt.reshape(sh),
                c2=c2.reshape(sh), s2=s2.reshape(sh), dropped=seg["dropped"])
