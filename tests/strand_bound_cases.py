"""Cases that put every comparison of the strand tracer on its bound, and a plain numpy restatement of the walks and of
the gate with every comparison, the dot order and the norm form switchable.  Shared by tools/gen_golden_strand_bounds.py
(which records what the reference does on them: tests/golden/strand_bounds.npz) and by tests/test_strand_bounds_*.py.
Needs no reference.

Reference: HairGrow.py -- trace :59-149, traceFromScalp :154-223, the drivers :226-299, the occupancy test :517-528.

The volume is 64 x 32 x 24 (W, H, Z).  Every case owns one row of voxels along x at its own (y, z); a per-seed walk never
leaves its row (the generator asserts it).  Every value is written by hand.  `e` below is the field a walk follows; the
reference negates y and z of what is stored, so (e_x, -e_y, -e_z) is stored (volume_arrays).

A trace case is laid out so that the decision on the bound changes the NUMBER of points of a strand of six or more
points (five lead steps on the other side of the seed), because trace returns False below five points; the five-point
cases alone have 4 and 5 points.  A scalp case returns whatever it walked once it has met an oriented voxel."""
import numpy as np

F = np.float32
W, H, Z = 64, 32, 24
DIMS = (W, H, Z)
THR8, THR7, THR_SMALL = 0.8, 0.7, 0.05          # Python floats, as the reference's thrDot
K = 8                                          # seed voxel of most cases
E = (1.0, 0.0, 0.0)
OCC_VALUES = (1.0, 0.5, -1.0, float("nan"), 1e-45, 1e-39, -0.0, 0.0)
TINY = float(np.finfo(np.float32).tiny)


def nxt(v, up=True):
    return F(np.nextafter(F(v), F(np.inf) if up else F(-np.inf)))


def around(v):
    """the float32 below v, v, the float32 above v"""
    return (nxt(v, False), F(v), nxt(v, True))


# ---------------------------------------------------------------------------------------------- arithmetic forms
def fma32(a, b, c):
    """fmaf on float32 scalars or arrays: the product of two float32 is exact in float64; the one float64 rounding of the
    sum is harmless unless it lands exactly half-way between two float32 (fma_tie), which the searches below exclude"""
    return (np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)).astype(F)


def fma_tie(a, b, c):
    d = np.asarray(a, np.float64) * np.asarray(b, np.float64) + np.asarray(c, np.float64)
    return (np.atleast_1d(d).view(np.uint64) & np.uint64(0x1FFFFFFF)) == np.uint64(0x10000000)


def dot3(a, b, order="ltr"):
    """torch.dot of three float32: separately rounded products added left to right ("ltr"); "rtl": the same products
    added from the last; "fma": a chain of fused multiply-adds from the first product.  a, b: [..., 3] float32"""
    a, b = np.asarray(a, F), np.asarray(b, F)
    if order == "ltr":
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
    if order == "rtl":
        return (a[..., 2] * b[..., 2] + a[..., 1] * b[..., 1]) + a[..., 0] * b[..., 0]
    return fma32(a[..., 2], b[..., 2], fma32(a[..., 1], b[..., 1], a[..., 0] * b[..., 0]))


def norm3(a, form="fma"):
    """torch.linalg.norm of three float32: the square root of an fma chain ("fma"); "plain": of the plain sum of
    separately rounded squares"""
    a = np.asarray(a, F)
    if form == "fma":
        s = fma32(a[..., 2], a[..., 2], fma32(a[..., 1], a[..., 1], a[..., 0] * a[..., 0]))
    else:
        s = (a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1]) + a[..., 2] * a[..., 2]
    return np.sqrt(s, dtype=F)


DEFAULT_FORMS = dict(
    dot="ltr", norm="fma", thr64=False, index="trunc",
    trace_dot="<",              # :88 / :127
    scalp_dot="<",              # :194
    scalp_neg="<",              # :196
    scalp_zero="<",             # :200
    scalp_norm="<",             # :184
    scalp_085="<",              # :187
    occ_zero="eq",              # :79 / :117 / :176   "eq": occ == 0, "le": occ <= 0, "tiny": fabs(occ) < smallest normal
    min_points=5,               # :144
    rule25_before_turn=False,   # :216 asked with Grow_Inner as it was before this step's turn
    flag_ge=">=",               # :70
    flag_per_point=False,       # :260 / :293   True: += 1 for every point, not once per distinct voxel
)
# every opposite form of a comparison: name -> the switches it changes
OPPOSITE_FORMS = {
    "trace_dot_le": dict(trace_dot="<="), "scalp_dot_le": dict(scalp_dot="<="), "scalp_neg_le": dict(scalp_neg="<="),
    "scalp_zero_le": dict(scalp_zero="<="), "scalp_norm_le": dict(scalp_norm="<="), "scalp_085_le": dict(scalp_085="<="),
    "occ_le": dict(occ_zero="le"), "occ_tiny": dict(occ_zero="tiny"),
    "min_points_4": dict(min_points=4), "min_points_6": dict(min_points=6),
    "index_floor": dict(index="floor"),
    "dot_rtl": dict(dot="rtl"), "dot_fma": dict(dot="fma"), "norm_plain": dict(norm="plain"),
    "thr64": dict(thr64=True), "rule25_before_turn": dict(rule25_before_turn=True),
    "flag_gt": dict(flag_ge=">"), "flag_per_point": dict(flag_per_point=True),
}
# the groups of cases each form may change (a form changes at least one strand, and strands of these groups only).
# index_floor changes nothing and cannot: trunc and floor differ on (-1, 0) alone, where trunc gives 0 and floor -1,
# and the clamp to [0, dim-1] that follows every conversion (:67-69 ...) makes both 0.
FORM_GROUPS = {
    "trace_dot_le": {"t_dot", "t_round_eq", "t_round_hi"},      # (a "hi" pair may have its left-to-right dot on the bound)
    "scalp_dot_le": {"s_dot"}, "scalp_neg_le": {"s_neg"},
    "scalp_zero_le": {"s_zero"}, "scalp_norm_le": {"s_norm1", "s_norm3"}, "scalp_085_le": {"s_085"},
    "occ_le": {"t_occ", "s_occ"}, "occ_tiny": {"t_occ", "s_occ"},
    "min_points_4": {"t_five"}, "min_points_6": {"t_five"},
    "index_floor": set(),
    "dot_rtl": {"t_round_hi", "t_round_lo", "t_round_eq"}, "dot_fma": {"t_round_hi", "t_round_lo", "t_round_eq"},
    "norm_plain": {"s_norm3", "s_lift", "s_085"},      # every normalisation goes through the same norm
    "thr64": {"t_dot", "s_dot", "s_neg"}, "rule25_before_turn": {"s_25"},
    "flag_gt": {"gate"}, "flag_per_point": {"driver"},
}


def forms(**kw):
    f = dict(DEFAULT_FORMS)
    for k in kw:
        assert k in f, k
    f.update(kw)
    return f


def _less(x, bound, op, f):
    """x < bound as the reference evaluates it: a 0-dim float32 tensor against a Python float compares in float32"""
    if f["thr64"]:
        x, bound = float(x), float(bound)
    else:
        x, bound = F(x), F(bound)
    return bool(x <= bound) if op == "<=" else bool(x < bound)


def _occ_is_zero(v, f):
    if f["occ_zero"] == "eq":
        return bool(v == 0)
    if f["occ_zero"] == "le":
        return bool(v <= 0)
    return bool(abs(v) < F(TINY))


def voxel_of(p, f=DEFAULT_FORMS, dims=DIMS):
    """.type(torch.long) and the clamps that follow: (x, y, z)"""
    q = np.floor(p) if f["index"] == "floor" else np.trunc(p)
    return tuple(int(min(max(int(q[a]), 0), dims[a] - 1)) for a in range(3))


# ---------------------------------------------------------------------------------------------- the walks, restated
def trace_np(vox, seed, thr, f=DEFAULT_FORMS):
    """HairGrowing.trace (:59-149) from an already shifted seed, without the flag test and the five-point rule
    -> (first, len, points [len, 3]) in the layout of mh_trace_seeds (centre slot 256).  vox: [Z, H, W, 4] float32"""
    dims = (vox.shape[2], vox.shape[1], vox.shape[0])
    seed = np.asarray(seed, F)
    sides = []
    for sgn in (1, -1):
        pos = seed.copy()
        x, y, z = voxel_of(pos, f, dims)
        tan = vox[z, y, x, :3].copy()
        pts, count = [], 0
        while True:
            if _occ_is_zero(vox[z, y, x, 3], f):
                break
            nx = (pos + tan) if sgn > 0 else (pos - tan)
            a, b, c = voxel_of(nx, f, dims)
            ntan = vox[c, b, a, :3].copy()
            if _less(dot3(ntan, tan, f["dot"]), thr, f["trace_dot"], f):
                break
            pos, tan, (x, y, z) = nx.astype(F), ntan, (a, b, c)
            pts.append(pos.copy())
            count += 1
            if count >= 256:
                break
        sides.append(pts)
    fw, bw = sides
    pts = np.array(bw[::-1] + [seed] + fw, F).reshape(-1, 3)
    return 256 - len(bw), len(pts), pts


def trace_gated_np(vox, flag, seed, thr, f=DEFAULT_FORMS):
    """trace as the reference returns it: the strand, or None for its False (flag at the seed voxel, fewer points)"""
    dims = (vox.shape[2], vox.shape[1], vox.shape[0])
    x, y, z = voxel_of(np.asarray(seed, F), f, dims)
    if (flag[z, y, x] > 3) if f["flag_ge"] == ">" else (flag[z, y, x] >= 3):
        return None
    _, n, pts = trace_np(vox, seed, thr, f)
    return pts if n >= f["min_points"] else None


def scalp_np(vox, seed, normal, thr, f=DEFAULT_FORMS):
    """HairGrowing.traceFromScalp (:154-223) -> points [len, 3], or None"""
    dims = (vox.shape[2], vox.shape[1], vox.shape[0])
    pos, nrm = np.asarray(seed, F).copy(), np.asarray(normal, F)
    d = np.array([0, 1, 0], F)
    lift = dot3(nrm, d, f["dot"]) + F(1)
    if F(1) < lift:                 # Python's min(lift, 1): 1 only where 1 < lift
        lift = F(1)
    t = nrm + d * lift
    tan = (t / norm3(t, f["norm"])).astype(F)
    x, y, z = voxel_of(pos, f, dims)
    pts, count, inner = [pos.copy()], 0, True
    while True:
        was_inner = inner
        if _occ_is_zero(vox[z, y, x, 3], f) and not inner:
            break
        nx = (pos + tan).astype(F)
        a, b, c = voxel_of(nx, f, dims)
        ntan = vox[c, b, a, :3].copy()
        if _less(norm3(ntan, f["norm"]), 0.1, f["scalp_norm"], f) and inner:
            if _less(dot3(tan, nrm, f["dot"]), 0.85, f["scalp_085"], f):
                ntan = tan
            else:
                t = tan + d * lift
                ntan = (t / norm3(t, f["norm"])).astype(F)
        else:
            if _less(dot3(ntan, tan, f["dot"]), thr, f["scalp_dot"], f) and not inner:
                if _less(dot3(-ntan, tan, f["dot"]), thr, f["scalp_neg"], f):
                    break
                ntan = -ntan
            if _less(dot3(ntan, tan, f["dot"]), 0, f["scalp_zero"], f) and inner:
                ntan = -ntan
            inner = False
        pos, tan, (x, y, z) = nx, ntan, (a, b, c)
        pts.append(pos.copy())
        count += 1
        if count >= 256:
            break
        if count >= 25 and (was_inner if f["rule25_before_turn"] else inner):
            break
    return None if inner else np.array(pts, F)


def _mark(flag, strand, mode, f, dims):
    seen = set()
    for p in strand:
        x, y, z = voxel_of(p, f, dims)
        if mode == 1:
            flag[z, y, x] = 1
        elif f["flag_per_point"] or (x, y, z) not in seen:
            seen.add((x, y, z))
            flag[z, y, x] += 1


def voxel_rounds_np(vox, flag, thr, jitter, rounds, f=DEFAULT_FORMS):
    """`rounds` passes of trace() over the occupied voxels (:250-260 / :283-293): the seed tensor is shifted in place by
    every call, so the shifts add up from round to round.  jitter: [rounds * n, 3] float32 draws in the reference's
    order.  Mutates flag -> the accepted strands"""
    dims = (vox.shape[2], vox.shape[1], vox.shape[0])
    pos = np.argwhere(vox[..., 3] != 0)[:, ::-1].astype(F)
    n, out = len(pos), []
    for r in range(rounds):
        for i in range(n):
            pos[i] = pos[i] + F(0.5)
            pos[i] = pos[i] + np.asarray(jitter[r * n + i], F) * F(0.5)
            s = trace_gated_np(vox, flag, pos[i], thr, f)
            if s is not None:
                out.append(s)
                _mark(flag, s, 0, f, dims)
    return out


def guide_np(vox, sp, sn, thr, jitter, f=DEFAULT_FORMS):
    """GenerateGuideStrandFromScalp (:226-265) -> (strands, num_root)"""
    dims = (vox.shape[2], vox.shape[1], vox.shape[0])
    flag = np.zeros(vox.shape[:3], F)
    out = []
    for p, m in zip(sp, sn):
        s = scalp_np(vox, p, m, thr, f)
        if s is not None:
            out.append(s)
            _mark(flag, s, 1, f, dims)
    num_root = len(out)
    return out + voxel_rounds_np(vox, flag, thr, jitter, 2, f), num_root


def random_np(vox, thr, jitter, f=DEFAULT_FORMS):
    """randomlyGenerateSegments (:269-299)"""
    return voxel_rounds_np(vox, np.zeros(vox.shape[:3], F), thr, jitter, 3, f)


# ---------------------------------------------------------------------------------------------- seeded searches
def search_dot_pairs(thr=THR8, want=8, seed=5):
    """(Tan, nextTan) pairs with three non-zero components whose dot product is about float32(thr):
    "hi": left to right >= float32(thr) while right to left or the fma chain is below it; "lo": the other way round
    (left to right below, another order not below); "eq": left to right exactly float32(thr).
    Tan = (0.9 .. 1, +-0.05 .. 0.25, +-0.05 .. 0.25): a step of Tan from a voxel centre lands in the next voxel of the row."""
    rng = np.random.default_rng(seed)
    n = 200000
    sg = lambda: rng.choice(np.array([-1.0, 1.0]), n)      # noqa: E731
    T = np.stack([0.9 + 0.1 * rng.random(n), sg() * (0.05 + 0.2 * rng.random(n)), sg() * (0.05 + 0.2 * rng.random(n))], 1).astype(F)
    M = np.stack([0.7 + 0.3 * rng.random(n), sg() * (0.05 + 0.4 * rng.random(n)), sg() * (0.05 + 0.4 * rng.random(n))], 1).astype(F)
    N = (M * (F(thr) / dot3(M, T))[:, None]).astype(F)
    ltr, rtl, fm = dot3(N, T, "ltr"), dot3(N, T, "rtl"), dot3(N, T, "fma")
    p0 = N[:, 0] * T[:, 0]
    safe = ~(fma_tie(N[:, 1], T[:, 1], p0) | fma_tie(N[:, 2], T[:, 2], fma32(N[:, 1], T[:, 1], p0)))
    t = F(thr)
    hi = safe & (ltr >= t) & ((rtl < t) | (fm < t))
    lo = safe & (ltr < t) & ((rtl >= t) | (fm >= t))
    eq = safe & (ltr == t)
    out = {}
    for name, m in (("hi", hi), ("lo", lo), ("eq", eq)):
        k = np.flatnonzero(m)
        # half of them picked where the right-to-left order decides, half where the fma chain does
        a = [i for i in k if (rtl[i] < t) != (ltr[i] < t)][:want // 2] if name != "eq" else []
        b = [i for i in k if (fm[i] < t) != (ltr[i] < t) and i not in a][:want - len(a)] if name != "eq" else list(k[:want])
        sel = np.array(a + b)
        assert len(sel) >= want, (name, len(sel))
        out[name] = (T[sel], N[sel])
    return out


def search_norm_rows(want=8, seed=6):
    """three-component rows whose fma-chain norm and plain-sum norm fall on different sides of float32(0.1); x > 0"""
    rng = np.random.default_rng(seed)
    n = 400000
    v = rng.normal(size=(n, 3))
    v[:, 0] = np.abs(v[:, 0]) + 0.2
    v = (v / np.linalg.norm(v, axis=1, keepdims=True) * 0.1).astype(F)
    a, b = norm3(v, "fma"), norm3(v, "plain")
    p0 = v[:, 0] * v[:, 0]
    safe = ~(fma_tie(v[:, 1], v[:, 1], p0) | fma_tie(v[:, 2], v[:, 2], fma32(v[:, 1], v[:, 1], p0)))
    t = F(0.1)
    k1 = np.flatnonzero(safe & (a < t) & (b >= t))[:want // 2]
    k2 = np.flatnonzero(safe & (a >= t) & (b < t))[:want - want // 2]
    assert len(k1) + len(k2) >= want
    return v[np.concatenate([k1, k2])]


def search_norm_axis():
    """c > 0 with norm((c, 0, 0)) = sqrt(c * c) equal to the float32 below 0.1, float32(0.1) and the float32 above"""
    out = []
    for target in around(0.1):
        c = F(target)
        for _ in range(8):
            c = nxt(c, False)
        found = None
        for _ in range(17):
            if norm3(np.array([c, 0, 0], F)) == target:
                found = c
                break
            c = nxt(c)
        assert found is not None, target
        out.append(found)
    return out


# ---------------------------------------------------------------------------------------------- the cases
class Cases:
    """vol_e [W, H, Z, 3] the field a walk follows, vol_occ [W, H, Z]; trace: list of dicts (group, name, seed, thr,
    row); scalp: likewise with `normal`; gate: (trace case index, flag value)"""

    def __init__(self):
        self.e = np.zeros(DIMS + (3,), F)
        self.occ = np.zeros(DIMS, F)
        self.trace, self.scalp, self.gate = [], [], []
        self._used = set()
        self._next = 0

    def row(self, y=None, z=None, guard=False):
        if y is None:
            while True:
                y, z = 1 + self._next % (H - 2), 1 + self._next // (H - 2)
                self._next += 1
                need = [(y, z)] + ([(y, z - 1), (y, z + 1)] if guard else [])
                if not any(r in self._used for r in need):
                    break
        assert (y, z) not in self._used and 0 <= y < H and 0 <= z < Z
        self._used.add((y, z))
        if guard:
            self._used.update([(y, z - 1), (y, z + 1)])
        return y, z

    def put(self, x, row, e, occ):
        assert np.all(self.e[x, row[0], row[1]] == 0) and self.occ[x, row[0], row[1]] == 0
        self.e[x, row[0], row[1]] = np.asarray(e, F)
        self.occ[x, row[0], row[1]] = F(occ)

    def add_trace(self, group, name, row, seed, thr):
        self.trace.append(dict(group=group, name=name, row=row, seed=np.asarray(seed, F), thr=thr))

    def add_scalp(self, group, name, row, seed, normal, thr):
        self.scalp.append(dict(group=group, name=name, row=row, seed=np.asarray(seed, F), normal=np.asarray(normal, F), thr=thr))

    # a trace cell: the seed voxel K holds T, `lead` voxels of (1,0,0) on the other side of the decision, then an empty
    # voxel (its dot of 0 stops the walk); the voxel on the decision's side holds N with occupancy 0, so the walk ends
    # there when it gets there
    def trace_cell(self, group, name, T, N, thr, back=False, lead=5, occ_seed=1.0, seed=None):
        row = self.row()
        s = -1 if back else 1
        for j in range(1, lead + 1):
            self.put(K - s * j, row, E, 1.0)
        self.put(K, row, T, occ_seed)
        if N is not None:
            self.put(K + s, row, N, 0.0)
        self.add_trace(group, name, row, (K + 0.5, row[0] + 0.5, row[1] + 0.5) if seed is None else seed, thr)
        return row


def build_cases():
    c = Cases()
    # ------------------------------------------------------------------ trace
    for thr in (THR8, THR7):                    # the dot on the bound, forward and backward
        for v in around(thr):
            for back in (False, True):
                c.trace_cell("t_dot", "thr%g_%r_%s" % (thr, float(v), "b" if back else "f"), E, (v, 0, 0), thr, back)
    pairs = search_dot_pairs()
    for kind in ("hi", "lo", "eq"):             # the rounding order
        for i, (T, N) in enumerate(zip(*pairs[kind])):
            c.trace_cell("t_round_" + kind, "%s%d" % (kind, i), T, N, THR8, back=bool(i % 2))
    for v in OCC_VALUES:                        # occ of the current voxel
        c.trace_cell("t_occ", "occ_%r" % v, E, E, THR8, occ_seed=v)
    # the five-point rule: f forward and b backward steps
    for fsteps, bsteps in ((4, 0), (0, 4), (2, 2), (2, 1), (3, 0), (0, 3), (5, 0), (3, 2)):
        row = c.row()
        for j in range(-bsteps, fsteps + 1):
            # the last forward voxel has occupancy 0; with no forward step the empty next voxel (a dot of 0) ends the walk
            c.put(K + j, row, E, 1.0 if (j != fsteps or fsteps == 0) else 0.0)
        c.add_trace("t_five", "five_%d+%d" % (fsteps, bsteps), row, (K + 0.5, row[0] + 0.5, row[1] + 0.5), THR8)
    # truncation.  at_k: a seed at exactly K.0 starts in voxel K.  below_k: the float32 below K.0 starts in K-1, whose
    # field (0.75,0,0) ends the walk at once (dot 0.75 with its neighbours).  step_on_int: (1.5,0,0) in voxel K takes
    # the seed K+0.5 to exactly K+2.0 and K-1.0: voxels K+2 (occupancy 0: the end) and K-1
    for name, sx in (("at_k", F(K)), ("below_k", nxt(K, False)), ("step_on_int", F(K + 0.5))):
        row = c.row()
        for j in range(-5, 3):
            e = (0.75, 0, 0) if (name == "below_k" and j == -1) else ((1.5, 0, 0) if (name == "step_on_int" and j == 0) else E)
            c.put(K + j, row, e, 1.0 if j < 2 else 0.0)
        c.add_trace("t_trunc", name, row, (sx, row[0] + 0.5, row[1] + 0.5), THR8)
    for axis in range(3):                       # seeds in (-1, 0) on each axis: voxel 0, as for 0.25
        for val in (-0.25, -0.875, 0.25):
            row = c.row(y=0 if axis == 1 else None, z=2 + len(c.trace) % 16 if axis == 1 else None) if axis != 2 else \
                c.row(y=2 + len(c.trace) % 24, z=0)
            x0 = 0 if axis == 0 else K
            for j in range(0, 7):
                c.put(x0 + j, row, E, 1.0 if j < 6 else 0.0)
            seed = [x0 + 0.5, row[0] + 0.5, row[1] + 0.5]
            seed[axis] = val
            c.add_trace("t_trunc", "axis%d_%g" % (axis, val), row, seed, THR8)
    for name, sx in (("w_minus", nxt(W, False)), ("w_exact", F(W)), ("w_999", F(W - 1 + 0.999))):
        row = c.row()
        for j in range(1, 8):                   # the last voxels of the row, pointing back into the volume
            c.put(W - j, row, (-1.0, 0, 0), 1.0 if j < 7 else 0.0)
        c.add_trace("t_trunc", name, row, (sx, row[0] + 0.5, row[1] + 0.5), THR8)
    # an orientation of length 0.5: two consecutive points share a voxel
    row = c.row()
    for j in range(-3, 4):
        c.put(K + j, row, (0.5, 0, 0), 1.0)
    c.add_trace("t_repeat", "half_steps", row, (K + 0.25, row[0] + 0.5, row[1] + 0.5), THR_SMALL)
    # the gate: flag values at the seed voxel of a strand that is otherwise returned
    gate_case = next(i for i, t in enumerate(c.trace) if t["name"] == "five_4+0")
    c.gate = [(gate_case, v) for v in (0.0, 2.0, 2.5, 3.0, 4.0)]

    # ------------------------------------------------------------------ traceFromScalp
    STRAIGHT = (0.5, -0.5, 0.0)       # Normal = (0.5, 0, 0) / 0.5 = (1, 0, 0); dot(Tan, seedNormal) = 0.5 < 0.85: keeps Tan

    def scalp_row(group, name, cells, thr, normal=STRAIGHT, guard=False, yoff=0.5):
        row = c.row(guard=guard)
        for j, (e, occ) in cells.items():
            c.put(K + j, row, e, occ)
        c.add_scalp(group, name, row, (K + 0.5, row[0] + yoff, row[1] + 0.5), normal, thr)

    for cc, tg in zip(search_norm_axis(), ("below", "at", "above")):       # norm on the bound, one axis
        scalp_row("s_norm1", "norm_" + tg, {1: ((cc, 0, 0), 1.0), 2: (E, 0.0)}, THR8)
    for i, v in enumerate(search_norm_rows()):                              # the norm's form
        scalp_row("s_norm3", "norm3_%d" % i, {1: (v, 1.0), 2: (E, 0.0)}, THR8)
    for v, tg in zip(around(0.85), ("below", "at", "above")):                # dot(Tan, seedNormal) on 0.85, inside
        scalp_row("s_085", "d085_" + tg, {2: (E, 1.0)}, THR8, normal=(v, -0.5, 0.0), yoff=0.25)
    for y in (0.0, -0.0, 1e-10, -1e-10, 0.5, -0.5, -1.0, -2.0):              # the lift
        scalp_row("s_lift", "lift_%r" % y, {1: (E, 0.0)}, THR8, normal=(8.0, y, 0.0))
    for s in (24, 25, 26):                                                   # the 25-step rule
        scalp_row("s_25", "first_at_%d" % s, {s: (E, 1.0), s + 1: (E, 0.0)}, THR8)
    for thr in (THR8, THR7):
        for v in around(thr):                                                # outside the head: the dot on the bound
            scalp_row("s_dot", "out_thr%g_%r" % (thr, float(v)), {1: (E, 1.0), 2: ((v, 0, 0), 0.0)}, thr)
            # the negated field on the bound: turned round when -dot >= thr; (2,0,0) behind it shows the turned step
            scalp_row("s_neg", "neg_thr%g_%r" % (thr, float(v)), {1: (E, 1.0), 2: ((-v, 0, 0), 1.0), 3: ((2.0, 0, 0), 0.0)}, thr)
    for v in (0.0, -0.0, TINY, -TINY):                                       # the first oriented voxel: dot < 0 turns it
        scalp_row("s_zero", "zero_%r" % v, {1: ((v, 0.0, 0.3), 1.0)}, THR_SMALL, guard=True)
    for v in OCC_VALUES:                                                     # occ == 0 and not Grow_Inner
        scalp_row("s_occ", "socc_%r" % v, {1: (E, v), 2: (E, 0.0)}, THR8)
    assert len(c.trace) <= 1024 and len(c.scalp) <= 256
    return c


def volume_arrays(c):
    """(occ [X,Y,Z] float64, ori [X,Y,Z,3] float64) in the reference's array layout: (e_x, -e_y, -e_z) is stored"""
    return c.occ.astype(np.float64), (c.e * np.array([1, -1, -1], F)).astype(np.float64)


def vox_of_cases(c):
    """[Z, H, W, 4] float32 as the walks read it: the field and the occupancy"""
    return np.ascontiguousarray(np.concatenate([c.e, c.occ[..., None]], -1).transpose(2, 1, 0, 3))


def readers_arrays(c):
    """what get_ground_truth_3D_occ / _ori return: occ [Z,Y,X,1], ori [Z,Y,X,3] (as stored: y, z negated)"""
    occ, ori = volume_arrays(c)
    return occ.transpose(2, 1, 0)[..., None].astype(F), ori.transpose(2, 1, 0, 3).astype(F)


# ---------------------------------------------------------------------------------------------- the occupancy ratio
VMIN64 = np.array([-0.32, -0.32, -0.24], F).astype(np.float64)     # points_to_voxel's float32 voxel_min, as float64
VS = 0.005 / 2
BOX = (256, 256, 192)


def world_of(idx):
    """a float64 world point whose voxel index (before rounding) is about idx: p = (idx * vs + vmin) * (1, -1, -1)"""
    return (np.asarray(idx, np.float64) * VS + VMIN64) * np.array([1.0, -1.0, -1.0])


def search_half(k, axis):
    """a float64 coordinate for which (p * sign - vmin) / vs is exactly k + 1/2, or None: the quotient's spacing is finer
    than the coordinate's for part of the range, so not every k has one"""
    sgn = 1.0 if axis == 0 else -1.0
    p = ((k + 0.5) * VS + VMIN64[axis]) * sgn
    q = p
    for step in range(64):
        for cand in ((q, p) if step else (p,)):
            if (cand * sgn - VMIN64[axis]) / VS == k + 0.5:
                return cand
        q, p = np.nextafter(q, -np.inf), np.nextafter(p, np.inf)
    return None


def half_indices(axis, count=2, start=40):
    """the first `count` even and `count` odd k >= start for which a coordinate lies exactly on k + 1/2: [(k, p)]"""
    out, have = [], {0: 0, 1: 0}
    for k in range(start, BOX[axis] - 2):
        if have[k % 2] < count:
            p = search_half(k, axis)
            if p is not None:
                out.append((k, p))
                have[k % 2] += 1
        if have[0] == count and have[1] == count:
            return out
    raise AssertionError("too few coordinates exactly on k + 1/2 on axis %d" % axis)


def occ_volume():
    """[192, 256, 256] float32: voxels with an even x + y + z are occupied -- a point's status follows its rounding"""
    z, y, x = np.meshgrid(np.arange(BOX[2]), np.arange(BOX[1]), np.arange(BOX[0]), indexing="ij")
    return ((x + y + z) % 2 == 0).astype(F)


def occ_strands():
    """(strands: list of float64 [n,3] world points, names).  On occ_volume a point of index (i, j, k) is occupied when
    i + j + k is even."""
    S, names = [], []

    def pts(idx):
        return world_of(np.asarray(idx, np.float64))

    def ratio(n_occ, n):
        rows = [(10 + 2 * t, 20, 30) for t in range(n_occ)] + [(11 + 2 * t, 20, 30) for t in range(n - n_occ)]
        return pts(rows)
    for n_occ, n in ((4, 5), (8, 10), (12, 15), (5, 6), (9, 11), (7, 7), (0, 7), (1, 1), (0, 1)):
        S.append(ratio(n_occ, n))
        names.append("ratio_%d_of_%d" % (n_occ, n))
    # a point exactly on k + 1/2 (half to even): one point strands; accepted when the rounded index is occupied
    for axis in range(3):
        for k, half in half_indices(axis):
            idx = [50.0, 60.0, 70.0]
            p = pts([idx])
            p[0, axis] = half
            S.append(p)
            names.append("half_axis%d_%d" % (axis, k))
    # the faces of the reference's box
    for axis, top in enumerate(BOX):
        for v in (top, top - 1):
            idx = [10.0, 20.0, 30.0]
            idx[axis] = v
            S.append(pts([idx, [10, 20, 30]]))
            names.append("face_axis%d_%d" % (axis, v))
    # negative indices: torch wraps -1 .. -dim (the last voxels of the axis); below -dim it raises IndexError
    for axis in range(3):
        for v in (-1, -2, -BOX[axis]):
            idx = [10.0, 20.0, 30.0]
            idx[axis] = v
            S.append(pts([idx]))
            names.append("neg_axis%d_%d" % (axis, v))
    idx = [-257.0, 20.0, 30.0]
    S.append(pts([idx]))
    names.append("refused_x")
    S.append(pts([[10, 20, 193], [-300, 20, 30]]))      # outside the box and refused: the box answers first
    names.append("box_and_refused")
    return S, names


def occ_status_np(strand, occ, ratio_op=">", rounding="even", thr64=False):
    """One attempt of the occupancy test (:517-528): 1 accepted, 0 rejected, 2 outside the reference's box (its three
    clauses), 3 where torch's indexing raises.  A negative index down to -dim wraps, as torch's does."""
    p = np.asarray(strand, np.float64) * np.array([1.0, -1.0, -1.0])
    q = (p - VMIN64) / VS
    idx = (np.rint(q) if rounding == "even" else np.floor(q + 0.5)).astype(np.int64)
    if idx[:, 2].max() >= 192 or (idx[:, 1] >= 256).any() or (idx[:, 0] >= 256).any():
        return 2
    dims = np.array([occ.shape[2], occ.shape[1], occ.shape[0]])
    if (idx < -dims).any() or (idx >= dims).any():
        return 3
    idx = np.where(idx < 0, idx + dims, idx)
    s = F(0)
    for v in occ[idx[:, 2], idx[:, 1], idx[:, 0]]:
        s = F(s + v)
    r = F(s / F(len(idx)))
    if thr64:
        return int(float(r) >= 0.8) if ratio_op == ">=" else int(float(r) > 0.8)
    return int(r >= F(0.8)) if ratio_op == ">=" else int(r > F(0.8))


def tile_strands(S, n):
    return [S[i % len(S)] for i in range(n)]
