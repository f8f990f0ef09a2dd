"""The strand-volume and volume-score rules of include/mh_pmvo.h ("Strand volume", "Volume scores") restated in numpy, brute
force: what the HIP kernels of csrc/hairvolume.hip must equal on every quantity.  float64 elementwise arithmetic in the order
the header writes it (numpy fuses nothing; + - * / sqrt are correctly rounded), np.rint rounds half to even, the per-voxel sums
are int64.  tests/test_hair_volume_host.py holds this file to hand-computed cases."""
import numpy as np

MAXN = 8192
MAX_COUNT = 1 << 29


def voxel_coords(points, bust_to_origin, voxel_min, voxel_size):
    """-> (w [n,3] world, g [n,3] unrounded voxel coordinates, valid [n]) float64"""
    p = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    b, m, vs = np.asarray(bust_to_origin, np.float64), np.asarray(voxel_min, np.float64), np.float64(voxel_size)
    with np.errstate(all="ignore"):
        w = p + b[None, :]
        g = np.empty_like(w)
        g[:, 0] = (w[:, 0] - m[0]) / vs
        g[:, 1] = ((-w[:, 1]) - m[1]) / vs
        g[:, 2] = ((-w[:, 2]) - m[2]) / vs
    return w, g, np.isfinite(g).all(1)


def accumulate(counts, points, bust_to_origin, voxel_min, voxel_size, dims, sub=2):
    """-> (acc int64 [X,Y,Z,7] = cnt, xx, yy, zz, xy, xz, yz; dropped_segments; outside_samples)"""
    X, Y, Z = (int(v) for v in dims)
    w, g, valid = voxel_coords(points, bust_to_origin, voxel_min, voxel_size)
    acc = np.zeros((X, Y, Z, 7), np.int64)
    dropped = outside = 0
    start = 0
    for c in (int(v) for v in counts):
        for a in range(start, start + c - 1):
            b = a + 1
            if not (valid[a] and valid[b]):
                continue
            d = g[b] - g[a]
            n = max(1.0, float(np.ceil(np.float64(sub) * max(abs(d[0]), abs(d[1]), abs(d[2])))))
            if not n <= MAXN:
                dropped += 1
                continue
            n = int(n)
            e = w[b] - w[a]
            ln = np.sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2])
            q = [0, 0, 0]
            if ln > 0.0 and np.isfinite(ln):
                q = [int(np.rint(4096.0 * (e[k] / ln))) for k in range(3)]
            prod = np.array([1, q[0] * q[0], q[1] * q[1], q[2] * q[2], q[0] * q[1], q[0] * q[2], q[1] * q[2]], np.int64)
            t = (np.arange(n, dtype=np.float64) + 0.5) / np.float64(n)
            v = [np.rint(g[a][k] + t * d[k]) for k in range(3)]
            inside = (v[0] >= 0) & (v[0] < X) & (v[1] >= 0) & (v[1] < Y) & (v[2] >= 0) & (v[2] < Z)
            outside += int((~inside).sum())
            ix = [v[k][inside].astype(np.int64) for k in range(3)]
            np.add.at(acc, (ix[0], ix[1], ix[2]), prod[None, :])
        start += c
    return acc, dropped, outside


def resolve(acc):
    """-> dict(voxels int64 [G,3] ascending by (x*Y + y)*Z + z, ori float32 [G,3], cnt int32 [G], coh float64 [G], sums [G,6])"""
    x, y, z = np.nonzero(acc[..., 0] > 0)          # C order of [X,Y,Z]: ascending key
    rows = acc[x, y, z]
    cnt = rows[:, 0]
    if (cnt > MAX_COUNT).any():
        raise ValueError("a voxel holds more than 2^29 samples")
    xx, yy, zz, xy, xz, yz = (rows[:, k].astype(np.float64) for k in range(1, 7))
    trace = (xx + yy) + zz
    has = trace > 0.0
    first = (xx >= yy) & (xx >= zz)
    second = ~first & (yy >= zz)
    vx = np.where(first, xx, np.where(second, xy, xz))
    vy = np.where(first, xy, np.where(second, yy, yz))
    vz = np.where(first, xz, np.where(second, yz, zz))

    def mul(vx, vy, vz):
        return (xx * vx + xy * vy) + xz * vz, (xy * vx + yy * vy) + yz * vz, (xz * vx + yz * vy) + zz * vz

    with np.errstate(all="ignore"):
        for _ in range(24):
            mx, my, mz = mul(vx, vy, vz)
            ln = np.sqrt((mx * mx + my * my) + mz * mz)
            vx, vy, vz = mx / ln, my / ln, mz / ln
        mx, my, mz = mul(vx, vy, vz)
        coh = ((vx * mx + vy * my) + vz * mz) / trace
    flip = vy > 0.0
    v = np.stack([np.where(flip, -vx, vx), np.where(flip, -vy, vy), np.where(flip, -vz, vz)], 1)
    ori = np.where(has[:, None], v, 0.0).astype(np.float32)
    return {"voxels": np.stack([x, y, z], 1).astype(np.int64).reshape(-1, 3), "ori": ori.reshape(-1, 3),
            "cnt": cnt.astype(np.int32), "coh": np.where(has, coh, 0.0), "sums": rows[:, 1:].reshape(-1, 6)}


def voxelize(counts, points, bust_to_origin, voxel_min, voxel_size, dims, sub=2):
    acc, dropped, outside = accumulate(counts, points, bust_to_origin, voxel_min, voxel_size, dims, sub)
    out = resolve(acc)
    out["dropped_segments"], out["outside_samples"] = dropped, outside
    return out


def check_unique(voxels, dims):
    v = np.asarray(voxels, np.int64).reshape(-1, 3)
    if ((v < 0) | (v >= np.asarray(dims, np.int64)[None, :])).any():
        raise ValueError("a voxel outside the grid")
    if len(np.unique(v, axis=0)) != len(v):
        raise ValueError("a voxel listed twice")
    return v


def match_flags(q_voxels, q_ori, t_voxels, t_ori, dims, reach, cos2):
    """uint8 [Gq]: every query against every target (the lists lie inside the grid: neighbours outside it do not exist)"""
    qv, tv = check_unique(q_voxels, dims), check_unique(t_voxels, dims)
    qo = np.asarray(q_ori, np.float32).reshape(-1, 3).astype(np.float64)
    to = np.asarray(t_ori, np.float32).reshape(-1, 3).astype(np.float64)
    out = np.zeros(len(qv), np.uint8)
    nb = (to[:, 0] * to[:, 0] + to[:, 1] * to[:, 1]) + to[:, 2] * to[:, 2]
    for i in range(len(qv)):
        cheb = np.abs(tv - qv[i][None, :]).max(1) if len(tv) else np.zeros(0, np.int64)
        a = qo[i]
        dot = (a[0] * to[:, 0] + a[1] * to[:, 1]) + a[2] * to[:, 2]
        na = (a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]
        for k, (r, c) in enumerate(zip(reach, cos2)):
            near = cheb <= int(r)
            ok = near if c < 0 else near & (na > 0.0) & (nb > 0.0) & (dot * dot >= np.float64(c) * (na * nb))
            if ok.any():
                out[i] |= 1 << k
    return out


def scores(pred, gt, dims, reach, cos2):
    """pred / gt = (voxels, ori) -> (flags_pred, flags_gt, counts dict as monohair_amd.hairvolume.score_volumes reports)"""
    fp = match_flags(pred[0], pred[1], gt[0], gt[1], dims, reach, cos2)
    fg = match_flags(gt[0], gt[1], pred[0], pred[1], dims, reach, cos2)
    K = len(reach)
    counts = {"pred": {"matched": [int(((fp >> k) & 1).sum()) for k in range(K)], "voxels": len(fp)},
              "gt": {"matched": [int(((fg >> k) & 1).sum()) for k in range(K)], "voxels": len(fg)}}
    return fp, fg, counts
