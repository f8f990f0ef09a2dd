"""The photograph rule of include/mh_pmvo.h ("Hair photograph") restated in numpy from the header text alone: what the tests
hold the photo kernels of csrc/haircapture.hip to, bit for bit.  It starts from the per-vertex (row, col, z255, valid) of one
view and the float32 world points, and does everything after the projection in float64 on those float32 values, one numpy
operation per operation of the rule."""
import numpy as np

MAX_N = 8192
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)


def _pairs(valid, counts):
    """indices a of the pairs (a, a+1) that are consecutive points of one strand, both valid"""
    valid = np.asarray(valid).reshape(-1) != 0
    counts = np.asarray(counts, np.int64).reshape(-1)
    assert counts.sum() == valid.shape[0]
    last = np.zeros(valid.shape[0], bool)
    last[np.cumsum(counts)[counts > 0] - 1] = True
    a = np.nonzero(~last)[0]
    return a[valid[a] & valid[a + 1]]


def segment_shades(points, valid, counts, albedo, light, ambient):
    """-> uint8 [n_points]: entry i is the shade q of segment (i, i+1), 0 where that pair makes no segment"""
    P = np.asarray(points, np.float32).reshape(-1, 3).astype(np.float64)
    counts = np.asarray(counts, np.int64).reshape(-1)
    albedo = np.asarray(albedo, np.float32).reshape(-1)
    L = np.asarray(light, np.float64).reshape(3)
    ambient = float(ambient)
    a = _pairs(valid, counts)
    strand = np.repeat(np.arange(len(counts)), counts)[a]
    T = P[a + 1] - P[a]
    tt = (T[:, 0] * T[:, 0] + T[:, 1] * T[:, 1]) + T[:, 2] * T[:, 2]
    tl = (T[:, 0] * L[0] + T[:, 1] * L[1]) + T[:, 2] * L[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        sin = np.where(tt > 0, np.sqrt(np.maximum(0.0, 1.0 - (tl * tl) / tt)), 0.0)
    v = (255.0 * albedo[strand].astype(np.float64)) * (ambient + (1.0 - ambient) * sin)
    q = np.where(v > 0, np.minimum(255.0, np.rint(v)), 0.0)
    shade = np.zeros(P.shape[0], np.uint8)
    shade[a] = q.astype(np.uint8)
    return shade


def fragments(vert, valid, counts, shade, H, W, S, w, depth0=None):
    """-> (sub-pixel index int64 [F], key uint64 [F], dropped) of every fragment that survives the grid and the occluder"""
    vert = np.asarray(vert, np.float32).reshape(-1, 3).astype(np.float64)
    shade = np.asarray(shade, np.uint8).reshape(-1)
    a = _pairs(valid, counts)
    k, h = float(S), float(S - 1) / 2.0
    r0, c0, z0 = k * vert[a, 0] + h, k * vert[a, 1] + h, vert[a, 2]
    dr, dc, dz = (k * vert[a + 1, 0] + h) - r0, (k * vert[a + 1, 1] + h) - c0, vert[a + 1, 2] - z0
    n = np.maximum(1.0, np.ceil(np.maximum(np.abs(dr), np.abs(dc))))
    keep = ~(n > MAX_N)
    dropped = int((~keep).sum())
    r0, c0, z0, dr, dc, dz, n, q = (x[keep] for x in (r0, c0, z0, dr, dc, dz, n, shade[a]))
    n = n.astype(np.int64)
    sidx = np.repeat(np.arange(n.shape[0], dtype=np.int64), n)
    j = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    t = (j.astype(np.float64) + 0.5) / n[sidx].astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        cr = np.rint(r0[sidx] + t * dr[sidx]).astype(np.int64)
        cc = np.rint(c0[sidx] + t * dc[sidx]).astype(np.int64)
        zf = (z0[sidx] + t * dz[sidx]).astype(np.float32)
    fin = np.isfinite(zf)
    cr, cc, zf, sidx = cr[fin], cc[fin], zf[fin], sidx[fin]
    off = np.arange(-w, w + 1, dtype=np.int64)
    dy, dx = [g.reshape(-1) for g in np.meshgrid(off, off, indexing="ij")]
    r = cr[:, None] + dy[None, :]
    c = cc[:, None] + dx[None, :]
    inside = (r >= 0) & (r < S * H) & (c >= 0) & (c < S * W)
    key = (zf.view(np.uint32).astype(np.uint64) << np.uint64(32)) | q[sidx].astype(np.uint64)
    z = np.broadcast_to(zf[:, None], r.shape)[inside]
    key = np.broadcast_to(key[:, None], r.shape)[inside]
    r, c = r[inside], c[inside]
    if depth0 is not None:
        d0 = np.asarray(depth0, np.float32).reshape(H, W)
        ok = ~(z > d0[r // S, c // S])
        r, c, key = r[ok], c[ok], key[ok]
    return r * (S * W) + c, key, dropped


def photo(vert, valid, counts, shade, H, W, S=4, w=1, depth0=None, bust_code=64, background_code=32):
    """One view -> dict(keys uint64 [S H, S W], gray uint8 [H,W], cover int32 [H,W], dropped)"""
    p, key, dropped = fragments(vert, valid, counts, shade, H, W, S, w, depth0)
    keys = np.full(S * H * S * W, EMPTY, np.uint64)
    np.minimum.at(keys, p, key)                                  # nearest first, then the darker shade
    keys = keys.reshape(S * H, S * W)
    hit = keys != EMPTY
    empty = np.full((H, W), background_code, np.int64)
    if depth0 is not None:
        empty[np.asarray(depth0, np.float32).reshape(H, W) < 255] = bust_code
    value = np.where(hit, (keys & np.uint64(0xFF)).astype(np.int64), np.repeat(np.repeat(empty, S, 0), S, 1))
    total = value.reshape(H, S, W, S).sum((1, 3))
    gray = (2 * total + S * S) // (2 * S * S)
    cover = hit.reshape(H, S, W, S).sum((1, 3))
    return dict(keys=keys, gray=gray.astype(np.uint8), cover=cover.astype(np.int32), dropped=dropped)
