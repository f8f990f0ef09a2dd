"""The reference's diffusion_scalp (Utils/PMVO_utils.py:467-593) restated in plain numpy, operation by operation: float32
where torch computes in float32 (the walk), float64 for the Hermite arc, the tangents and their normalisation.  Two facts
about the libraries are part of it (probed against CPU torch 2.10 and scipy 1.15, and held by the golden):
  * torch.linalg.norm(x, 2, dim=-1) of three elements is sqrt(fma(x2, x2, fma(x1, x1, x0*x0))), in float32 and float64;
  * scipy's PPoly evaluates c0 s^3 + c1 s^2 + c2 s + c3 in power form: res = 0; z = 1; for c in (c3, c2, c1, c0):
    res += c*z; z *= s.
tests/test_scalp_diffusion_host.py holds it to the reference's run (tests/golden/scalp_diffusion.npz);
tests/test_scalp_diffusion_gpu.py uses it as the comparator of the kernels.

Every decision is switchable (RULES below; `rules=dict(name=value)` on walk / arc / diffusion_scalp): the defaults are the
reference's, every other value is a form a kernel could take by mistake.  tests/test_scalp_diffusion_bounds_host.py holds
the defaults to the reference's run on the bounds (tests/golden/scalp_diffusion_bounds.npz) and shows that each other value
changes recorded rows."""
import collections
from fractions import Fraction

import numpy as np

F32 = np.float32
VMIN = np.array([-0.32, -0.32, -0.24], F32)          # points_to_voxel's float32 voxel_min
VS = 0.005 / 2
VS32 = F32(VS)                                        # what a float32 tensor is multiplied with / divided by
ACCEPTED, INSIDE, STEPS, RESTARTS, LEFT = range(5)
TRACE_STEP, MAX_FAIL, THRESHOLD = 10, 8, F32(0.5)
EPS = F32(1e-8)                                       # torch.cosine_similarity's eps
COS_FORMS = ("torch", "dot_over_norms", "dot_over_max", "plain_norms", "dot_rtl")
RULES = dict(
    accept_pos="gt",        # cos(g) > 0.5                         | "ge"
    accept_neg="gt",        # cos(-g) > 0.5                        | "ge"
    bias_sign="lt",         # cos(g) < 0 takes -g as the bias      | "le"
    max_fail=MAX_FAIL,      # fail_count > 8                       | 7, 9
    trace_step=TRACE_STEP,  # step < 10, step >= 10                | 9, 11
    cos_first=False,        # the ten-step rule before the cosine  | True: the cosine first
    cos_form="torch",       # one of COS_FORMS
    unit_bias=False,        # the bias is the raw orientation      | True: its unit vector
    occ_test="eq0",         # conf == 0                            | "le0", "flush" (|conf| below the smallest normal)
    index="trunc",          # .type(torch.long)                    | "floor"
    row_vs="f64",           # rows: / 0.0025 in float64            | "f32": / float64(float32(0.0025))
    param="mul",            # np.linspace: k * (1 / step)          | "div": k / step
    force_last=True,        # np.linspace sets the last one to 1   | False
    acc="f32",              # float32 accumulator, float64 sums    | "f64": a float64 accumulator, rounded once
    row_order="forward",    # rows of a voxel in row order         | "reverse"
    occ_rule="blend",       # occ + (1 - occ) * 1                  | "one"
    weight="blend",         # ori + (1 - occ) * d                  | "one": ori + d
)


def _rules(rules):
    r = dict(RULES)
    if rules:
        assert set(rules) <= set(RULES), sorted(set(rules) - set(RULES))
        r.update(rules)
    return r


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


def voxel32(p, index="trunc"):
    """points_to_voxel(p).type(torch.long) of a float32 point: truncation toward zero"""
    q = p.copy()
    q[1:] *= F32(-1)
    f = (q - VMIN) / VS32
    return (np.trunc(f) if index == "trunc" else np.floor(f)).astype(np.int64) if np.isfinite(f).all() else None


def fma32_rows(a, b, c):
    """round(a*b + c) with ONE rounding, elementwise on float32 arrays: the product is exact in float64, the sum is
    rounded to odd there (two-sum tells whether it was exact), and 53 bits rounded to odd round to 24 as the exact value"""
    with np.errstate(over="ignore", invalid="ignore"):
        p, c = np.asarray(a, F32).astype(np.float64) * np.asarray(b, F32).astype(np.float64), np.asarray(c, F32).astype(np.float64)
        s = p + c
        bp = s - p
        err = (p - (s - bp)) + (c - bp)
        bits = s.view(np.int64).copy() if s.ndim else np.array(s).view(np.int64).copy()
        odd = np.isfinite(s) & (err != 0) & ((bits & 1) == 0)
        away = (err > 0) == (s > 0)                   # the exact sum lies further from zero than s
        bits = np.where(odd, np.where(away | (s == 0), bits + 1, bits - 1), bits)
        s2 = bits.view(np.float64)
        s2 = np.where(odd & (s == 0), np.where(err > 0, 1.0, -1.0) * 5e-324, s2)
        return s2.astype(F32)


def norm32_rows(v, plain=False):
    """torch.linalg.norm(v, 2, dim=-1) of [...,3] float32 rows (plain: the squares added left to right, no fma)"""
    v = np.asarray(v, F32)
    with np.errstate(over="ignore", invalid="ignore"):
        if plain:
            return np.sqrt((v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2])
        return np.sqrt(fma32_rows(v[..., 2], v[..., 2], fma32_rows(v[..., 1], v[..., 1], v[..., 0] * v[..., 0])))


def cosine32_rows(a, b, form="torch"):
    """torch.cosine_similarity(a, b, dim=-1) of [...,3] float32 rows, bit for bit (held to the installed torch by
    tests/test_scalp_diffusion_bounds_host.py, and to the reference's own calls on the bound by the golden): each operand
    divided by max(its norm, 1e-8), the three products added left to right to a sum that starts at +0.0 (three products
    of -0.0 give +0.0: the reference's run records it).  The other COS_FORMS are what it is not."""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    with np.errstate(over="ignore", invalid="ignore", divide="ignore", under="ignore"):
        na, nb = norm32_rows(a, form == "plain_norms"), norm32_rows(b, form == "plain_norms")
        if form in ("dot_over_norms", "dot_over_max"):
            dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
            den = na * nb
            return (dot / (np.maximum(den, EPS) if form == "dot_over_max" else den)).astype(F32)
        x, y = a / np.maximum(na, EPS)[..., None], b / np.maximum(nb, EPS)[..., None]
        if form == "dot_rtl":
            return (((F32(0) + x[..., 2] * y[..., 2]) + x[..., 1] * y[..., 1]) + x[..., 0] * y[..., 0]).astype(F32)
        assert form in ("torch", "plain_norms"), form
        return (((F32(0) + x[..., 0] * y[..., 0]) + x[..., 1] * y[..., 1]) + x[..., 2] * y[..., 2]).astype(F32)


def cosine32(a, b, form="torch"):
    """torch.cosine_similarity of two float32 3-vectors"""
    return F32(cosine32_rows(a, b, form))


def _ge_gt(x, bound, op):
    return x >= bound if op == "ge" else x > bound


def walk(point, normal, occ, ori, stats=None, rules=None, cosines=None):
    """:494-536 for one sample -> (status, step, end point, normal_set[0], normal_set[-1], restarts).  occ [Z,Y,X],
    ori [3,Z,Y,X] float32.  A voxel index outside the volume ends the walk with LEFT (the reference raises or wraps).
    cosines: a list that receives cos(grow_dir, normal) of every turn that asks for it."""
    r = _rules(rules)
    TRACE_STEP, MAX_FAIL = r["trace_step"], r["max_fail"]
    Z, Y, X = occ.shape
    pc, nc = point.copy(), normal.copy()
    bias = np.zeros(3, F32)
    first = last = np.zeros(3, F32)
    step = fail = 0
    while True:
        if fail > MAX_FAIL:
            return RESTARTS, step, pc, first, last, fail
        idx = voxel32(pc, r["index"])
        if idx is None or (idx < 0).any() or idx[0] >= X or idx[1] >= Y or idx[2] >= Z:
            return LEFT, step, pc, first, last, fail
        if stats is not None:
            f = (pc * np.array([1, -1, -1], F32) - VMIN) / VS32
            stats["trunc_negative"] += int(((f > -1) & (f < 0)).any())
        conf = occ[idx[2], idx[1], idx[0]]
        with np.errstate(invalid="ignore"):
            empty = conf == 0 if r["occ_test"] == "eq0" else (conf <= 0 if r["occ_test"] == "le0"
                                                              else np.abs(conf) < np.finfo(F32).tiny)
        if empty and step < TRACE_STEP:
            t = (F32(0.8) * nc + F32(0.2) * bias).astype(F32)
            nc = (t / norm3(t, F32)).astype(F32)
            if step == 0:
                first = nc
            pc = (pc + nc * VS32).astype(F32)
            step += 1
            continue
        if step == 0:
            return INSIDE, step, pc, first, last, fail
        if step >= TRACE_STEP and not r["cos_first"]:
            return STEPS, step, pc, first, last, fail
        g = ori[:, idx[2], idx[1], idx[0]].astype(F32)
        c = cosine32(g, nc, r["cos_form"])
        if cosines is not None:
            cosines.append(c)
        if stats is not None:
            stats["cos_near"] += int(abs(abs(float(c)) - 0.5) < 1e-4 or abs(float(c)) < 1e-4 and g.any())
            stats["zero_ori"] += int(not g.any())
        pos = _ge_gt(c, THRESHOLD, r["accept_pos"])
        if pos or _ge_gt(-c, THRESHOLD, r["accept_neg"]):
            if stats is not None:
                stats["accept_%s_%s" % ("pos" if pos else "neg", "first" if fail == 0 else "restarted")] += 1
            return ACCEPTED, step, pc, first, (g if pos else -g), fail
        if step >= TRACE_STEP:                        # cos_first alone comes here
            return STEPS, step, pc, first, last, fail
        pc = point.copy()
        bias = -g if (c <= 0 if r["bias_sign"] == "le" else c < 0) else g
        if r["unit_bias"]:
            with np.errstate(invalid="ignore", divide="ignore"):
                bias = (bias / norm3(bias, F32)).astype(F32)
        step = 0
        fail += 1


def arc(p0, p1, n0, n1, step, rules=None):
    """:545-548 -> (sample [step+1,3], tangent [step+1,3]) float64"""
    r = _rules(rules)
    y0, y1 = p0.astype(np.float64), p1.astype(np.float64)
    d0 = ((n0 * VS32).astype(F32) * F32(step)).astype(np.float64)
    d1 = ((n1 * VS32).astype(F32) * F32(step)).astype(np.float64)
    slope = (y1 - y0) / 1.0
    t = ((d0 + d1) - 2 * slope) / 1.0
    c0, c1, c2, c3 = t / 1.0, (slope - d0) / 1.0 - t, d0, y0
    u = np.arange(step + 1) * (1.0 / step) if r["param"] == "mul" else np.arange(step + 1) / float(step)
    if r["force_last"]:
        u[-1] = 1.0
    s = np.empty((step + 1, 3))
    for k, x in enumerate(u):
        res, z = np.zeros(3), 1.0
        for c in (c3, c2, c1, c0):
            res = res + c * z
            z = z * x
        s[k] = res
    return s, np.concatenate([s[1:] - s[:-1], s[-1:] - s[-2:-1]], 0)


def voxel64(sample, row_vs="f64", index="trunc"):
    """:561 on float64 rows -> (float voxel coordinates [R,3], truncated int64 [R,3])"""
    f = (sample * np.array([1.0, -1.0, -1.0]) - VMIN.astype(np.float64)) / (VS if row_vs == "f64" else np.float64(VS32))
    return f, (np.trunc(f) if index == "trunc" else np.floor(f)).astype(np.int64)


def diffusion_scalp(points, normals, ori, occ, stats=None, rules=None):
    """-> (ori [3,Z,Y,X], occ [1,Z,Y,X], details).  details: status / step / restarts [n], end_point / first_normal /
    last_normal [n,3] float32, total_sample / total_normal (as the reference saves them) / total_normal_unit [R,3]
    float64, voxel [R,3] int64 (x, y, z), cosines: per sample the list of cos(grow_dir, normal) it asked for.  No accepted
    sample: the volumes come back unchanged."""
    r = _rules(rules)
    stats = collections.defaultdict(int) if stats is None else stats
    points, normals = np.ascontiguousarray(points, F32).reshape(-1, 3), np.ascontiguousarray(normals, F32).reshape(-1, 3)
    ori, occ = np.asarray(ori, F32), np.asarray(occ, F32)
    Z, Y, X = occ.shape[1:]
    n = points.shape[0]
    det = dict(status=np.zeros(n, np.int32), step=np.zeros(n, np.int32), restarts=np.zeros(n, np.int32),
               end_point=np.zeros((n, 3), F32), first_normal=np.zeros((n, 3), F32), last_normal=np.zeros((n, 3), F32))
    samples, tangents = [], []
    det["cosines"] = [[] for _ in range(n)]
    for i in range(n):
        st, step, pe, nf, nl, fail = walk(points[i], normals[i], occ[0], ori, stats, r, det["cosines"][i])
        det["status"][i], det["step"][i], det["restarts"][i] = st, step, fail
        det["end_point"][i], det["first_normal"][i], det["last_normal"][i] = pe, nf, nl
        if st == ACCEPTED:
            s, t = arc(points[i], pe, nf, nl, step, r)
            samples.append(s)
            tangents.append(t)
    R = sum(len(s) for s in samples)
    det["total_sample"] = np.concatenate(samples, 0) if R else np.zeros((0, 3))
    det["total_normal"] = np.concatenate(tangents, 0) if R else np.zeros((0, 3))
    unit = np.zeros((R, 3))
    for k in range(R):
        t = det["total_normal"][k]
        with np.errstate(divide="ignore", invalid="ignore"):
            unit[k] = t / norm3(t, np.float64)
    det["total_normal_unit"] = unit
    f, vox = voxel64(det["total_sample"], r["row_vs"], r["index"])
    inside = ((f > -1) & (f < np.array([X, Y, Z]))).all(1) & (vox >= 0).all(1)
    det["voxel"] = np.where(inside[:, None], vox, -1)
    stats["boundary_near"] += int((np.abs(f - np.rint(f)) < 1e-6).any()) if R else 0
    stats["zero_tangent"] += int((~det["total_normal"].any(1)).sum())
    stats["rows_outside"] += int((~inside).sum())
    ori_out, occ_out = ori.copy(), occ.copy()
    acc = collections.OrderedDict()
    rows = np.flatnonzero(inside)
    first_seen = list(collections.OrderedDict((tuple(vox[k]), None) for k in rows))
    for k in (rows if r["row_order"] == "forward" else rows[::-1]):
        key = tuple(vox[k])
        a, c = acc.get(key, (np.zeros(3, F32 if r["acc"] == "f32" else np.float64), F32(0)))
        acc[key] = ((a.astype(np.float64) + unit[k]).astype(a.dtype), F32(c + F32(1)))
    acc = collections.OrderedDict((key, acc[key]) for key in first_seen)
    with np.errstate(invalid="ignore"):
        for (x, y, z), (a, c) in acc.items():
            d = (a.astype(F32) / np.maximum(c, F32(1e-6))).astype(F32)
            o = occ[0, z, y, x]
            w = F32(F32(1) - o) if r["weight"] == "blend" else F32(1)
            ori_out[:, z, y, x] = ori[:, z, y, x] + w * d
            occ_out[0, z, y, x] = o + F32(F32(1) - o) * F32(1) if r["occ_rule"] == "blend" else F32(1)
    det["rows_per_voxel"] = {k: int(v[1]) for k, v in acc.items()}
    return ori_out, occ_out, det
