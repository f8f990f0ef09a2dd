"""The reference's diffusion_scalp (Utils/PMVO_utils.py:467-593) restated in plain numpy, operation by operation: float32
where torch computes in float32 (the walk), float64 for the Hermite arc, the tangents and their normalisation.  Two facts
about the libraries are part of it (probed against CPU torch 2.10 and scipy 1.15, and held by the golden):
  * torch.linalg.norm(x, 2, dim=-1) of three elements is sqrt(fma(x2, x2, fma(x1, x1, x0*x0))), in float32 and float64;
  * scipy's PPoly evaluates c0 s^3 + c1 s^2 + c2 s + c3 in power form: res = 0; z = 1; for c in (c3, c2, c1, c0):
    res += c*z; z *= s.
tests/test_scalp_diffusion_host.py holds it to the reference's run (tests/golden/scalp_diffusion.npz);
tests/test_scalp_diffusion_gpu.py uses it as the comparator of the kernels."""
import collections
from fractions import Fraction

import numpy as np

F32 = np.float32
VMIN = np.array([-0.32, -0.32, -0.24], F32)          # points_to_voxel's float32 voxel_min
VS = 0.005 / 2
VS32 = F32(VS)                                        # what a float32 tensor is multiplied with / divided by
ACCEPTED, INSIDE, STEPS, RESTARTS, LEFT = range(5)
TRACE_STEP, MAX_FAIL, THRESHOLD = 10, 8, F32(0.5)


def to_world(v):
    """voxel coordinates (x, y, z) -> float32 world points (voxel_to_points: v * 0.0025 + voxel_min, y and z negated)"""
    p = (np.asarray(v, F32) * VS32 + VMIN).astype(F32)
    p[..., 1:] *= F32(-1)
    return p


def _round(fr, dtype):
    """a Fraction rounded to nearest-even in dtype"""
    d = float(fr)                                     # correctly rounded to float64
    if dtype is np.float64:
        return np.float64(d)
    best = F32(d)
    for c in (np.nextafter(best, F32(np.inf)), np.nextafter(best, F32(-np.inf))):
        if np.isfinite(c) and abs(Fraction(float(c)) - fr) < abs(Fraction(float(best)) - fr):
            best = c
    return best


def fma(a, b, c, dtype):
    """round(a*b + c) with ONE rounding"""
    if not (np.isfinite(a) and np.isfinite(b) and np.isfinite(c)):
        return dtype(a) * dtype(b) + dtype(c)
    return _round(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)), dtype)


def norm3(v, dtype):
    """torch.linalg.norm(v, 2, dim=-1) of three elements"""
    return np.sqrt(fma(v[2], v[2], fma(v[1], v[1], dtype(v[0] * v[0]), dtype), dtype))


def voxel32(p):
    """points_to_voxel(p).type(torch.long) of a float32 point: truncation toward zero"""
    q = p.copy()
    q[1:] *= F32(-1)
    f = (q - VMIN) / VS32
    return np.trunc(f).astype(np.int64) if np.isfinite(f).all() else None


def cosine32(a, b):
    """torch.cosine_similarity of two float32 3-vectors (decisions only: the goldens keep 1e-4 away from its thresholds)"""
    na, nb = np.maximum(norm3(a, F32), F32(1e-8)), np.maximum(norm3(b, F32), F32(1e-8))
    x, y = a / na, b / nb
    return F32(F32(x[0] * y[0] + x[1] * y[1]) + x[2] * y[2])


def walk(point, normal, occ, ori, stats=None):
    """:494-536 for one sample -> (status, step, end point, normal_set[0], normal_set[-1], restarts).  occ [Z,Y,X],
    ori [3,Z,Y,X] float32.  A voxel index outside the volume ends the walk with LEFT (the reference raises or wraps)."""
    Z, Y, X = occ.shape
    pc, nc = point.copy(), normal.copy()
    bias = np.zeros(3, F32)
    first = last = np.zeros(3, F32)
    step = fail = 0
    while True:
        if fail > MAX_FAIL:
            return RESTARTS, step, pc, first, last, fail
        idx = voxel32(pc)
        if idx is None or (idx < 0).any() or idx[0] >= X or idx[1] >= Y or idx[2] >= Z:
            return LEFT, step, pc, first, last, fail
        if stats is not None:
            f = (pc * np.array([1, -1, -1], F32) - VMIN) / VS32
            stats["trunc_negative"] += int(((f > -1) & (f < 0)).any())
        conf = occ[idx[2], idx[1], idx[0]]
        if conf == 0 and step < TRACE_STEP:
            t = (F32(0.8) * nc + F32(0.2) * bias).astype(F32)
            nc = (t / norm3(t, F32)).astype(F32)
            if step == 0:
                first = nc
            pc = (pc + nc * VS32).astype(F32)
            step += 1
            continue
        if step == 0:
            return INSIDE, step, pc, first, last, fail
        if step >= TRACE_STEP:
            return STEPS, step, pc, first, last, fail
        g = ori[:, idx[2], idx[1], idx[0]].astype(F32)
        c = cosine32(g, nc)
        if stats is not None:
            stats["cos_near"] += int(abs(abs(float(c)) - 0.5) < 1e-4 or abs(float(c)) < 1e-4 and g.any())
            stats["zero_ori"] += int(not g.any())
        if c > THRESHOLD or -c > THRESHOLD:
            if stats is not None:
                stats["accept_%s_%s" % ("pos" if c > 0 else "neg", "first" if fail == 0 else "restarted")] += 1
            return ACCEPTED, step, pc, first, (g if c > 0 else -g), fail
        pc = point.copy()
        bias = -g if c < 0 else g
        step = 0
        fail += 1


def arc(p0, p1, n0, n1, step):
    """:545-548 -> (sample [step+1,3], tangent [step+1,3]) float64"""
    y0, y1 = p0.astype(np.float64), p1.astype(np.float64)
    d0 = ((n0 * VS32).astype(F32) * F32(step)).astype(np.float64)
    d1 = ((n1 * VS32).astype(F32) * F32(step)).astype(np.float64)
    slope = (y1 - y0) / 1.0
    t = ((d0 + d1) - 2 * slope) / 1.0
    c0, c1, c2, c3 = t / 1.0, (slope - d0) / 1.0 - t, d0, y0
    u = np.arange(step + 1) * (1.0 / step)
    u[-1] = 1.0
    s = np.empty((step + 1, 3))
    for k, x in enumerate(u):
        res, z = np.zeros(3), 1.0
        for c in (c3, c2, c1, c0):
            res = res + c * z
            z = z * x
        s[k] = res
    return s, np.concatenate([s[1:] - s[:-1], s[-1:] - s[-2:-1]], 0)


def voxel64(sample):
    """:561 on float64 rows -> (float voxel coordinates [R,3], truncated int64 [R,3])"""
    f = (sample * np.array([1.0, -1.0, -1.0]) - VMIN.astype(np.float64)) / VS
    return f, np.trunc(f).astype(np.int64)


def diffusion_scalp(points, normals, ori, occ, stats=None):
    """-> (ori [3,Z,Y,X], occ [1,Z,Y,X], details).  details: status / step / restarts [n], end_point / first_normal /
    last_normal [n,3] float32, total_sample / total_normal (as the reference saves them) / total_normal_unit [R,3]
    float64, voxel [R,3] int64 (x, y, z).  No accepted sample: the volumes come back unchanged."""
    stats = collections.defaultdict(int) if stats is None else stats
    points, normals = np.ascontiguousarray(points, F32).reshape(-1, 3), np.ascontiguousarray(normals, F32).reshape(-1, 3)
    ori, occ = np.asarray(ori, F32), np.asarray(occ, F32)
    Z, Y, X = occ.shape[1:]
    n = points.shape[0]
    det = dict(status=np.zeros(n, np.int32), step=np.zeros(n, np.int32), restarts=np.zeros(n, np.int32),
               end_point=np.zeros((n, 3), F32), first_normal=np.zeros((n, 3), F32), last_normal=np.zeros((n, 3), F32))
    samples, tangents = [], []
    for i in range(n):
        st, step, pe, nf, nl, fail = walk(points[i], normals[i], occ[0], ori, stats)
        det["status"][i], det["step"][i], det["restarts"][i] = st, step, fail
        det["end_point"][i], det["first_normal"][i], det["last_normal"][i] = pe, nf, nl
        if st == ACCEPTED:
            s, t = arc(points[i], pe, nf, nl, step)
            samples.append(s)
            tangents.append(t)
    R = sum(len(s) for s in samples)
    det["total_sample"] = np.concatenate(samples, 0) if R else np.zeros((0, 3))
    det["total_normal"] = np.concatenate(tangents, 0) if R else np.zeros((0, 3))
    unit = np.zeros((R, 3))
    for r in range(R):
        t = det["total_normal"][r]
        with np.errstate(divide="ignore", invalid="ignore"):
            unit[r] = t / norm3(t, np.float64)
    det["total_normal_unit"] = unit
    f, vox = voxel64(det["total_sample"])
    inside = ((f > -1) & (f < np.array([X, Y, Z]))).all(1)
    det["voxel"] = np.where(inside[:, None], vox, -1)
    stats["boundary_near"] += int((np.abs(f - np.rint(f)) < 1e-6).any()) if R else 0
    stats["zero_tangent"] += int((~det["total_normal"].any(1)).sum())
    stats["rows_outside"] += int((~inside).sum())
    ori_out, occ_out = ori.copy(), occ.copy()
    acc = collections.OrderedDict()
    for r in np.flatnonzero(inside):
        key = tuple(vox[r])
        a, c = acc.get(key, (np.zeros(3, F32), F32(0)))
        acc[key] = ((a.astype(np.float64) + unit[r]).astype(F32), F32(c + F32(1)))
    for (x, y, z), (a, c) in acc.items():
        d = (a / np.maximum(c, F32(1e-6))).astype(F32)
        o = occ[0, z, y, x]
        ori_out[:, z, y, x] = ori[:, z, y, x] + F32(F32(1) - o) * d
        occ_out[0, z, y, x] = o + F32(F32(1) - o) * F32(1)
    det["rows_per_voxel"] = {k: int(v[1]) for k, v in acc.items()}
    return ori_out, occ_out, det
