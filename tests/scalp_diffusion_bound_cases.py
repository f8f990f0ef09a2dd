"""Hand-written cases that put every decision of the scalp diffusion (the reference's diffusion_scalp,
Utils/PMVO_utils.py:467-593; csrc/hairdiffuse.hip) ON its bound: a 16 x 24 x 48 (Z, Y, X) volume, one slot of voxels per
case, one batch of samples.  build() -> dict(points, normals, ori, occ, expect, info): expect[name] = sample indices as in
gen_golden_diffusion.edge_case, info = what a search found (JSON-able).  Values "by search" come from seeded searches with
the numpy restatement (tests/scalp_diffusion_np.py) which assert what they found; tools/gen_golden_diffusion_bounds.py
then asserts on the REFERENCE's run that every case reaches what it exists for.

Layout: slots of 3 x 3 x 3 voxels (hair in the centre voxel (3a+1, 3b+1, 3c+1), c = 0..2) for walks of one step in any
direction, and rows (y = 3b+1, z = 10 or 13, three stretches of 16 voxels in x) for straight walks along +x.

Not reachable: a cosine of -0.0.  torch sums the three products into +0.0, and three products of -0.0 give +0.0 there
(recorded: cos(-g, n) of g = (0, 1, 0), n = (1, 0, 0) is +0.0); a kernel that adds them without that start would need all
three products to be -0.0, and the normal's unit vector has a component of 0.57 or more whose partner would have to be
-0.0 itself, which no component of the normal is after the first blend 0.8 n + 0.2 * (+0.0).
"""
import numpy as np

import scalp_diffusion_np as rs

F32 = np.float32
Z, Y, X = 16, 24, 48
HALF, HALF_LO, HALF_HI = F32(0.5), np.nextafter(F32(0.5), F32(0)), np.nextafter(F32(0.5), F32(1))
EX = np.array([1, 0, 0], F32)
EY = np.array([0, 1, 0], F32)
FLIP = np.array([1, -1, -1], F32)
ORIENTATIONS = dict(axis=np.array([1, 0, 0], F32), long=np.array([2, 0, 0], F32), oblique=np.array([0.6, 0.8, 0], F32))
OCC_END = dict(one=1.0, half=0.5, two=2.0, minus_one=-1.0, nan=np.nan, denormal_min=1e-45, denormal=1e-39)
FORMS = rs.COS_FORMS[1:]
FORM_ROWS, FORM_TRIALS = 8, 10 ** 6


def blend_rows(n):
    """the first turn's normal of [M,3] float32 normals: 0.8 n + 0.2 * 0, divided by its norm"""
    t = (F32(0.8) * np.asarray(n, F32) + F32(0.2) * F32(0)).astype(F32)
    return (t / rs.norm32_rows(t)[..., None]).astype(F32)


def normals_at_60_degrees(rng, g, m):
    """m float32 normals turned away from g by acos(0.5) +- 2e-7 rad about seeded axes"""
    b = np.asarray(g, np.float64) / np.linalg.norm(np.asarray(g, np.float64), axis=-1, keepdims=True)
    b = np.broadcast_to(b, (m, 3))
    t = rng.normal(size=(m, 3))
    t -= (t * b).sum(1, keepdims=True) * b
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    ang = np.arccos(0.5) + rng.uniform(-2e-7, 2e-7, m)
    return (np.cos(ang)[:, None] * b + np.sin(ang)[:, None] * t).astype(F32)


def find_bound_normal(seed, stored, target):
    """a normal whose first turn gives cos(stored, normal) == target (float32, bit for bit), by search"""
    rng = np.random.default_rng(seed)
    n = normals_at_60_degrees(rng, np.sign(target) * stored, 4000)
    c = rs.cosine32_rows(np.broadcast_to(stored, n.shape), blend_rows(n))
    hit = np.flatnonzero(c == F32(target))
    assert len(hit), (stored, target)
    return n[hit[0]], int(len(hit))


def find_form_rows(seed, form):
    """up to FORM_ROWS (orientation, normal) rows on which `form` falls on the other side of 0.5 than torch's cosine"""
    rng = np.random.default_rng(seed)
    out, trials = [], 0
    while len(out) < FORM_ROWS and trials < FORM_TRIALS:
        m = 100000
        g = rng.normal(size=(m, 3))
        g = (g / np.linalg.norm(g, axis=1, keepdims=True) * rng.uniform(0.3, 3.0, (m, 1))).astype(F32)
        n = normals_at_60_degrees(rng, g, m)
        nc = blend_rows(n)
        d = np.flatnonzero((rs.cosine32_rows(g, nc) > HALF) != (rs.cosine32_rows(g, nc, form) > HALF))
        out += [(g[k], n[k]) for k in d[:FORM_ROWS - len(out)]]
        trials += m
    return out, trials


class Builder:
    def __init__(self):
        self.occ, self.ori = np.zeros((1, Z, Y, X), F32), np.zeros((3, Z, Y, X), F32)
        self.pts, self.nrm, self.expect, self.owner, self.g_of = [], [], {}, {}, {}
        self.slots = [(3 * a + 1, 3 * b + 1, 3 * c + 1) for c in range(3) for b in range(8) for a in range(16)
                      if not (b == 0 and c == 0)]
        self.rows = [(16 * s, 3 * b + 1, z) for z in (10, 13) for b in range(8) for s in range(3)]

    def hair(self, name, x, y, z, o, occ=1.0):
        assert (x, y, z) not in self.owner, (name, self.owner[(x, y, z)])
        self.owner[(x, y, z)] = name
        self.occ[0, z, y, x] = F32(occ)
        self.ori[:, z, y, x] = np.asarray(o, F32)

    def sample(self, name, v, n=EX, world=None):
        self.expect.setdefault(name, []).append(len(self.pts))
        self.pts.append(rs.to_world(v) if world is None else np.asarray(world, F32))
        self.nrm.append(np.asarray(n, F32))
        return len(self.pts) - 1

    def slot(self):
        return self.slots.pop(0)

    def row(self):
        return self.rows.pop(0)

    def whole_row(self):
        """a row of the volume that no other case walks in"""
        while self.rows[0][0] != 0:
            self.rows.pop(0)
        x0, y, z = self.rows.pop(0)
        del self.rows[:2]
        return x0, y, z

    def one_step(self, name, g, n, occ=1.0):
        """hair with orientation g in a slot's centre voxel and a sample one step of normal n before its centre"""
        hx, hy, hz = self.slot()
        self.hair(name, hx, hy, hz, g, occ)
        c = np.array([hx, hy, hz], np.float64) + 0.5
        i = self.sample(name, c - np.asarray(blend_rows(n), np.float64) * FLIP, n)
        self.g_of[i] = np.asarray(g, F32)
        return i


def _walk(b, i, rules=None):
    cos = []
    return rs.walk(b.pts[i], b.nrm[i], b.occ[0], b.ori, None, rules, cos) + (cos,)


def _f32(p):
    return (F32(p) - rs.VMIN[0]) / rs.VS32


def _f64(p):
    return (np.float64(F32(p)) - np.float64(rs.VMIN[0])) / rs.VS


def _f64w(p):
    return (np.float64(F32(p)) - np.float64(rs.VMIN[0])) / np.float64(rs.VS32)


def _near(k):
    """the float32 coordinates within two steps of k * vs + vmin"""
    p = F32(F32(k) * rs.VS32 + rs.VMIN[0])
    out = [p]
    for d in (F32(-np.inf), F32(np.inf)):
        q = p
        for _ in range(2):
            q = np.nextafter(q, d)
            out.append(q)
    return sorted(out)


def build():
    b, info = Builder(), {}

    # ---- occupancy test conf == 0: what ends a walk, and the splat's weights on the end voxel
    for name, v in OCC_END.items():
        b.one_step("occ_" + name, EX, EX, v)
    rng = np.random.default_rng(3)
    o = rng.uniform(-1.0, -0.5, 4000).astype(F32)
    odd = o[(o + (F32(1) - o)) != F32(1)]
    assert len(odd), "an occupancy with occ + (1 - occ) != 1"
    info["occ_not_one"] = float(odd[0])
    b.one_step("occ_not_one", EX, EX, odd[0])
    for name, v in (("occ_minus_zero", -0.0), ("occ_zero", 0.0)):
        hx, hy, hz = b.slot()
        b.hair(name, hx, hy, hz, EY, v)                 # occupancy +-0.0 with an orientation that disagrees: walked through
        b.hair(name, hx + 1, hy, hz, EX)
        b.sample(name, [hx - 0.5, hy + 0.5, hz + 0.5])

    # ---- acceptance cos > 0.5, then cos(-g) > 0.5: the cosine on float32(0.5) and its two neighbours
    info["bound_hits"] = {}
    for oi, (oname, g) in enumerate(ORIENTATIONS.items()):
        for si, (sname, sign) in enumerate((("pos", 1.0), ("neg", -1.0))):
            stored = (F32(0) - g).astype(F32) if sign < 0 else g      # 0 - g: no -0.0 in the volume
            for ti, (tname, t) in enumerate((("lo", HALF_LO), ("on", HALF), ("hi", HALF_HI))):
                name = "cos_%s_%s_%s" % (oname, sname, tname)
                n, hits = find_bound_normal(100 + 9 * oi + 3 * si + ti, stored, sign * t)
                info["bound_hits"][name] = hits
                i = b.one_step(name, stored, n)
                assert _walk(b, i)[6][0] == F32(sign * t)
    info["form_trials"] = {}
    for fi, form in enumerate(FORMS):
        rows, trials = find_form_rows(200 + fi, form)
        info["form_trials"][form] = [len(rows), trials]
        for g, n in rows:
            b.one_step("form_" + form, g, n)

    # ---- sign of the bias cos < 0: cosines +0.0 and +- the smallest float32, then restarts that end in acceptance
    tiny = F32(1e-45)
    for name, ny in (("bias_zero", F32(0)), ("bias_plus_tiny", tiny), ("bias_minus_tiny", -tiny)):
        hx, hy, hz = b.slot()
        for dy in (-1, 0, 1):
            b.hair(name, hx, hy + dy, hz, EY)
        i = b.sample(name, [hx - 0.5, hy + 0.5, hz + 0.5], [1, ny, 0])
        st, step, pe, nf, nl, fail, cos = _walk(b, i)
        assert st == rs.ACCEPTED and fail >= 1 and cos[0] == ny and np.signbit(cos[0]) == np.signbit(ny)
        other = _walk(b, i, dict(bias_sign="le"))
        assert (name == "bias_zero") == (not np.array_equal(other[2], pe)), name

    # ---- step < 10, asked before the cosine; walks of every step count (the arc parameter)
    for s in range(1, 11):
        x0, y, z = b.row()
        name = "step%d" % s
        b.hair(name, x0 + s, y, z, EX)
        i = b.sample(name, [x0 + 0.5, y + 0.5, z + 0.5])
        st, step = _walk(b, i)[:2]
        assert (st, step) == ((rs.ACCEPTED, s) if s < 10 else (rs.STEPS, 10))
    differ = {s for s in range(1, 10) if any(k * (1.0 / s) != k / float(s) for k in range(s + 1))}
    assert differ == {5, 6, 7, 9}, differ
    info["param_steps_that_differ"] = sorted(differ)
    assert all(s * (1.0 / s) == 1.0 for s in range(1, 10))       # linspace's forced last 1 cannot show below 49 steps
    # a walk on which k * (1 / step) and k / step give different rows.  The start cannot decide it (a float32 coordinate
    # has no bits where the two products differ), the slope n * vs * step does: the normal by search
    found = None
    for s in sorted(differ):
        x0, y, z = b.row()
        b.hair("param_div", x0 + s, y, z, EX)
        rng = np.random.default_rng(40 + s)
        p = rs.to_world([x0 + 0.5, y + 0.5, z + 0.5])
        for _ in range(200):
            n = np.array([1, rng.uniform(-0.03, 0.03), rng.uniform(-0.03, 0.03)])
            n = (n / np.linalg.norm(n)).astype(F32)
            st, step, pe, nf, nl, fail = rs.walk(p, n, b.occ[0], b.ori)
            assert st == rs.ACCEPTED and step == s
            if not np.array_equal(rs.arc(p, pe, nf, nl, s)[0], rs.arc(p, pe, nf, nl, s, dict(param="div"))[0]):
                found = s
                b.sample("param_div", None, n, world=p)
                break
        if found:
            break
    assert found, "no normal found on which k / step changes a row"
    info["param_div_step"] = found

    # ---- fail_count > 8: accepted after exactly 8 restarts, abandoned after 9; the bias is the raw orientation
    def restart_case(name, m):
        hx, hy, hz = b.slot()
        b.hair(name, hx, hy, hz, [0, m, 0])
        b.hair(name, hx, hy - 1, hz, EX)
        return b.sample(name, [hx - 0.5, hy + 0.051, hz + 0.5])

    probe = Builder()
    probe.hair("p", 4, 4, 4, [0, 1, 0])
    probe.hair("p", 4, 3, 4, EX)
    res = {}
    for m in np.arange(0.0200, 0.0320, 0.0005).astype(F32):
        probe.ori[1, 4, 4, 4] = m
        st, step, pe, nf, nl, fail = rs.walk(rs.to_world([3.5, 4.051, 4.5]), EX, probe.occ[0], probe.ori)
        res[float(m)] = (st, fail)
    ms = sorted(res)
    pair = [(lo, hi) for lo, hi in zip(ms[:-1], ms[1:]) if res[lo] == (rs.RESTARTS, 9) and res[hi] == (rs.ACCEPTED, 8)]
    assert len(pair) == 1, res
    info["restart_magnitudes"] = list(pair[0])
    for name, m, want in (("restarts8", pair[0][1], (rs.ACCEPTED, 8)), ("restarts9", pair[0][0], (rs.RESTARTS, 9))):
        i = restart_case(name, F32(m))
        w = _walk(b, i)
        assert (w[0], w[5]) == want, (name, w)
        assert _walk(b, i, dict(unit_bias=True))[5] == 1

    # ---- float32 voxel conversion of walk points
    _, y, z = b.whole_row()
    cand = [(k, p) for k in range(2, 40) for p in _near(k)
            if _f32(p) == F32(k) and _f32(np.nextafter(p, F32(-np.inf))) < F32(k)]
    assert cand, "no float32 coordinate with the index exactly k.0"
    k, p = cand[0]
    info["index_k"] = [int(k), float(p)]
    b.hair("index_k", k - 1, y, z, EX)
    b.hair("index_k", k + 2, y, z, EX)
    wy, wz = rs.to_world([0, y + 0.5, z + 0.5])[1:]
    i = b.sample("index_k", None, EX, world=[p, wy, wz])
    j = b.sample("index_below_k", None, EX, world=[np.nextafter(p, F32(-np.inf)), wy, wz])
    assert _walk(b, i)[0] == rs.ACCEPTED and _walk(b, j)[0] == rs.INSIDE
    # an index in (-1, 0) on each axis: truncation says voxel 0 (floor would leave the volume)
    _, y, z = b.whole_row()
    b.hair("negative_x", 2, y, z, EX)
    b.sample("negative_x", [-0.5, y + 0.5, z + 0.5])
    b.hair("negative_y", 18, 0, 10, EX)
    b.sample("negative_y", [17.5, -0.5, 10.5])
    b.hair("negative_z", 4, 1, 0, EX)
    b.sample("negative_z", [3.5, 1.5, -0.5])
    for name in ("negative_x", "negative_y", "negative_z"):
        i = b.expect[name][0]
        assert _walk(b, i)[0] == rs.ACCEPTED and _walk(b, i, dict(index="floor"))[0] == rs.LEFT
    # a step that lands exactly on an integer index, from a start that is not on one
    _, y, z = b.whole_row()
    land = None
    for k in range(2, 40):                              # the coordinates one voxel before those whose index is k.0
        for q in _near(k):
            p = F32(q - rs.VS32)
            for d in (F32(-np.inf), F32(np.inf)):
                for c in (p, np.nextafter(p, d), np.nextafter(np.nextafter(p, d), d)):
                    if land is None and F32(c + rs.VS32) == q and _f32(q) == F32(k) and F32(k - 1) < _f32(c) < F32(k):
                        land = (k, c)
    info["step_lands_on_integer"] = None if land is None else [int(land[0]), float(land[1])]
    if land is not None:
        b.hair("lands_on_integer", land[0], y, z, EX)
        wy, wz = rs.to_world([0, y + 0.5, z + 0.5])[1:]
        i = b.sample("lands_on_integer", None, EX, world=[land[1], wy, wz])
        w = _walk(b, i)
        assert (w[0], w[1]) == (rs.ACCEPTED, 1) and _f32(w[2][0]) == F32(land[0])

    # ---- float64 voxel of the rows: 0.0025 in float64, not the widened float32 voxel size
    lo = [(k, p) for k in range(2, 40) for p in _near(k) if _f32(p) == F32(k) and _f64(p) < k <= _f64w(p)]
    hi = [(k, p) for k in range(2, 40) for p in _near(k) if _f32(p) < F32(k) and _f64(p) >= k > _f64w(p)]
    assert lo, "no coordinate whose float32 index is k.0 and whose float64 index lies below k"
    info["row_voxel_candidates"] = [len(lo), len(hi)]
    for name, cands in (("row_voxel_below", lo), ("row_voxel_above", hi)):
        if not cands:
            continue
        x0, y, z = b.whole_row()
        k, p = cands[len(cands) // 2]
        b.hair(name, k + 2, y, z, EX)
        wy, wz = rs.to_world([0, y + 0.5, z + 0.5])[1:]
        i = b.sample(name, None, EX, world=[p, wy, wz])
        assert _walk(b, i)[0] == rs.ACCEPTED
        v64, v32 = rs.voxel64(np.array([[p, wy, wz]], np.float64))[1][0, 0], rs.voxel32(np.array([p, wy, wz], F32))[0]
        assert (v64, v32) == ((k - 1, k) if name == "row_voxel_below" else (k, k - 1)), (name, v64, v32)
        assert rs.voxel64(np.array([[p, wy, wz]], np.float64), "f32")[1][0, 0] == v32

    # ---- splat order: one voxel with the rows of four samples, one with exactly one row
    hx, hy, hz = b.slot()
    b.hair("splat_four", hx, hy, hz, EX)
    rng = np.random.default_rng(9)
    chosen = None
    for _ in range(300):
        ns = np.concatenate([np.ones((4, 1)), rng.uniform(-0.15, 0.15, (4, 2))], 1)
        ns = (ns / np.linalg.norm(ns, axis=1, keepdims=True)).astype(F32)
        ps = rs.to_world(np.array([hx - 0.4, hy + 0.5, hz + 0.5]) + rng.uniform(-0.05, 0.05, (4, 3)))
        units = []
        for p, n in zip(ps, ns):
            st, step, pe, nf, nl, fail = rs.walk(p, n, b.occ[0], b.ori)
            assert st == rs.ACCEPTED and step == 1
            t = rs.arc(p, pe, nf, nl, 1)[1][0]
            units.append(t / rs.norm3(t, np.float64))
        fwd, rev, f64 = np.zeros(3, F32), np.zeros(3, F32), np.zeros(3)
        for u in units:
            fwd = (fwd.astype(np.float64) + u).astype(F32)
            f64 = f64 + u
        for u in units[::-1]:
            rev = (rev.astype(np.float64) + u).astype(F32)
        q = F32(4)
        if not np.array_equal(fwd / q, rev / q) and not np.array_equal(fwd / q, f64.astype(F32) / q):
            chosen = (ps, ns)
            break
    assert chosen, "no four samples whose sum depends on the order and on the accumulator"
    for p, n in zip(*chosen):
        b.sample("splat_four", None, n, world=p)
    b.expect["one_row"] = list(b.expect["step1"])

    pts, nrm = np.array(b.pts, F32), np.array(b.nrm, F32)
    ori, occ = b.ori.copy(), b.occ.copy()
    assert not (np.signbit(ori) & (ori == 0)).any()      # no -0.0 orientation: the reference's sum would make it +0.0
    stored = np.array([b.g_of.get(i, np.zeros(3, F32)) for i in range(len(pts))], F32)
    return dict(points=pts, normals=nrm, ori=ori, occ=occ, expect={k: np.array(v, np.int32) for k, v in b.expect.items()},
                info=info, orientation=stored)


def tiled(case, n):
    """the batch repeated cyclically to n samples"""
    m = len(case["points"])
    idx = np.arange(n) % m
    return case["points"][idx], case["normals"][idx]


# the switches of the restatement that are NOT the reference, and the cases built to tell each from it; a switch in
# UNREACHABLE changes no record and cannot (the reason stands beside it)
SWITCHES = {
    "accept_pos=ge": (dict(accept_pos="ge"), ("cos_", "form_")),
    "accept_neg=ge": (dict(accept_neg="ge"), ("cos_",)),
    "bias_sign=le": (dict(bias_sign="le"), ("bias_zero", "restarts")),
    "max_fail=7": (dict(max_fail=7), ("restarts",)),
    "max_fail=9": (dict(max_fail=9), ("restarts9",)),
    "trace_step=9": (dict(trace_step=9), ("step9", "step10", "param_div")),
    "trace_step=11": (dict(trace_step=11), ("step10",)),
    "cos_first": (dict(cos_first=True), ("step10",)),
    "cos_form=dot_over_norms": (dict(cos_form="dot_over_norms"), ("form_", "cos_")),
    "cos_form=dot_over_max": (dict(cos_form="dot_over_max"), ("form_", "cos_")),
    "cos_form=plain_norms": (dict(cos_form="plain_norms"), ("form_", "cos_")),
    "cos_form=dot_rtl": (dict(cos_form="dot_rtl"), ("form_", "cos_")),
    "unit_bias": (dict(unit_bias=True), ("restarts", "cos_", "form_", "bias_")),
    "occ_test=le0": (dict(occ_test="le0"), ("occ_minus_one", "occ_not_one")),
    "occ_test=flush": (dict(occ_test="flush"), ("occ_denormal",)),
    "index=floor": (dict(index="floor"), ("negative_",)),
    "row_vs=f32": (dict(row_vs="f32"), ("row_voxel_",)),
    "param=div": (dict(param="div"), ("param_div", "step")),
    "acc=f64": (dict(acc="f64"), ("splat_four",)),
    "row_order=reverse": (dict(row_order="reverse"), ("splat_four",)),
    "occ_rule=one": (dict(occ_rule="one"), ("occ_nan", "occ_not_one")),
    "weight=one": (dict(weight="one"), ("",)),           # every end voxel: its weight is 0
}
UNREACHABLE = {
    "force_last=False": (dict(force_last=False), "k * (1 / k) == 1.0 in float64 for every k below 49; walks have at most 9 steps"),
}

PER_SAMPLE = ("status", "step", "restarts", "end_point", "first_normal", "last_normal")


def same_bits(a, b):
    """equal bit for bit, NaN == NaN"""
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return bool(((np.ascontiguousarray(a).view(u) == np.ascontiguousarray(b).view(u)) | (np.isnan(a) & np.isnan(b))).all())


def differ_bits(a, b):
    """elementwise: not the same bits (NaN == NaN)"""
    u = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    return (np.ascontiguousarray(a).view(u) != np.ascontiguousarray(b).view(u)) & ~(np.isnan(a) & np.isnan(b))


def store_volume(out, tag, ori, occ):
    """the volume, sparse: every voxel whose occupancy or orientation has a bit set, with the values themselves"""
    nz = np.argwhere((occ[0].view(np.uint32) != 0) | (ori.view(np.uint32) != 0).any(0))
    out[tag + "_shape"] = np.array(occ.shape[1:], np.int32)
    out[tag + "_vox_nz"] = nz.astype(np.int16)
    out[tag + "_occ_nz"] = occ[0, nz[:, 0], nz[:, 1], nz[:, 2]].copy()
    out[tag + "_ori_nz"] = ori[:, nz[:, 0], nz[:, 1], nz[:, 2]].T.copy()


def load(z, tag):
    """(points, normals, ori [3,Z,Y,X], occ [1,Z,Y,X]) float32 from the record, occupancies bit for bit"""
    d = tuple(int(v) for v in z[tag + "_shape"])
    nz = z[tag + "_vox_nz"].astype(np.int64)
    occ, ori = np.zeros((1,) + d, F32), np.zeros((3,) + d, F32)
    occ[0, nz[:, 0], nz[:, 1], nz[:, 2]] = z[tag + "_occ_nz"]
    ori[:, nz[:, 0], nz[:, 1], nz[:, 2]] = z[tag + "_ori_nz"].T
    return z[tag + "_points"], z[tag + "_normals"], ori, occ


def expected_volumes(z, tag, ori, occ):
    """the reference's returned volumes: the input with the recorded changed voxels replaced"""
    ch = z[tag + "_changed"].astype(np.int64)
    o, c = ori.copy(), occ.copy()
    o[:, ch[:, 0], ch[:, 1], ch[:, 2]] = z[tag + "_changed_ori"].T
    c[0, ch[:, 0], ch[:, 1], ch[:, 2]] = z[tag + "_changed_occ"]
    return o, c


def calls_of(det):
    """the values torch.cosine_similarity returns to the reference, call by call, of a restatement's run -> (values, offsets
    per sample): a turn that fails asks three times (g, -g, g), one accepted by -g twice, one accepted by g once"""
    vals, offs = [], [0]
    for i, cs in enumerate(det["cosines"]):
        for j, c in enumerate(cs):
            last = j == len(cs) - 1 and det["status"][i] == rs.ACCEPTED
            neg = F32(0) - c                          # of -g: the exact negative, but +0.0 for a cosine of +0.0
            vals += [c] if last and c > HALF else ([c, neg] if last else [c, neg, c])
        offs.append(len(vals))
    return np.array(vals, F32), np.array(offs, np.int32)


def row_offsets(det):
    return np.concatenate([[0], np.cumsum(np.where(det["status"] == rs.ACCEPTED, det["step"] + 1, 0))])


def check_record(z, tag, res):
    """a run (ori, occ, details) of the restatement or of the kernels against the record `tag`, everything exact"""
    o, c, det = res
    pts, nrm, ori, occ = load(z, tag)
    assert np.array_equal(det["status"], z[tag + "_status"]) and np.array_equal(det["step"], z[tag + "_step"])
    acc = z[tag + "_status"] == 0
    for k in ("end_point", "first_normal", "last_normal"):
        got = np.asarray(det[k])
        assert got.dtype == F32 and same_bits(got[acc], z["%s_%s" % (tag, k)][acc]), k
    assert np.array_equal(np.asarray(det["voxel"], np.int64), z[tag + "_voxel"].astype(np.int64)), "voxel"
    for k in ("total_sample", "total_normal"):
        got = np.asarray(det[k])
        assert got.dtype == np.float64 and same_bits(got, z["%s_%s" % (tag, k)]), k
    eo, ec = expected_volumes(z, tag, ori, occ)
    assert same_bits(c, ec), "occ"
    assert same_bits(o, eo), "ori"
    if "cosines" in det:
        assert np.array_equal(det["restarts"], z[tag + "_restarts"])
        vals, offs = calls_of(det)
        assert np.array_equal(offs, z[tag + "_cos_offsets"]) and same_bits(vals, z[tag + "_cos_values"]), "cosines"


def differing_samples(a, b):
    """the samples on which two runs (ori, occ, details) of the restatement differ: in a per-sample quantity, in a row,
    or in a voxel of the returned volumes that one of their rows falls into"""
    (oa, ca, da), (ob, cb, db) = a, b
    out = set()
    for k in PER_SAMPLE:
        d = differ_bits(da[k], db[k]) if da[k].dtype.kind == "f" else da[k] != db[k]
        out |= set(np.flatnonzero(d.reshape(len(d), -1).any(1)).tolist())
    fa, fb = row_offsets(da), row_offsets(db)
    for i in range(len(da["status"])):
        ra, rb = slice(fa[i], fa[i + 1]), slice(fb[i], fb[i + 1])
        if fa[i + 1] - fa[i] != fb[i + 1] - fb[i] or any(not same_bits(da[k][ra], db[k][rb]) for k in
                                                         ("total_sample", "total_normal", "total_normal_unit", "voxel")):
            out.add(i)
    bad = differ_bits(oa, ob).any(0) | differ_bits(ca, cb)[0]
    for det, f in ((da, fa), (db, fb)):
        for i in range(len(det["status"])):
            v = det["voxel"][f[i]:f[i + 1]]
            v = v[(v >= 0).all(1)]
            if len(v) and bad[v[:, 2], v[:, 1], v[:, 0]].any():
                out.add(i)
    return out


def names_of(expect, samples, m):
    """the case names of sample indices of the batch (or of the batch tiled: index mod m)"""
    s = {int(i) % m for i in samples}
    return sorted(k for k, v in expect.items() if s & set(int(x) for x in v))


def assert_properties(case, rec):
    """every property a case exists for, on the reference's record of the case batch alone (rec: the quantities
    run_reference returns and the cosine calls; case: build())"""
    m = len(case["points"])
    e, info = case["expect"], case["info"]
    pts, nrm, ori, occ = case["points"], case["normals"], case["ori"], case["occ"]
    st, sp, rt = rec["status"], rec["step"], rec["restarts"]
    cv, co = rec["cos_values"], rec["cos_offsets"]
    calls = lambda i: cv[co[i]:co[i + 1]]                                   # noqa: E731
    off = np.concatenate([[0], np.cumsum(np.where(st == 0, sp + 1, 0))])
    rows = lambda i: slice(off[i], off[i + 1])                              # noqa: E731
    vox = rec["voxel"].astype(np.int64)
    ch = {tuple(v): k for k, v in enumerate(rec["changed"].tolist())}       # (z, y, x) -> row of the changed record
    bits = lambda x: np.asarray(x, F32).view(np.uint32)                     # noqa: E731

    def end_voxel(i):
        return tuple(vox[off[i + 1] - 1][::-1].tolist())

    # occupancy: the walk ends on anything but +-0.0, and the end voxel shows the splat's weight
    for name, v in list(OCC_END.items()) + [("not_one", info["occ_not_one"])]:
        i = e["occ_" + name][0]
        assert (st[i], sp[i], rt[i]) == (0, 1, 0), name
        z, y, x = end_voxel(i)
        o = occ[0, z, y, x]
        assert bits(o) == bits(F32(v)) or np.isnan(v)
        if v == 1.0:
            assert (z, y, x) not in ch
            continue
        k = ch[(z, y, x)]
        with np.errstate(invalid="ignore"):
            d = rec["total_normal"][off[i + 1] - 1]
            d = (d / rs.norm3(d, np.float64)).astype(F32) / F32(1)
            assert same_bits(rec["changed_occ"][k], F32(o + F32(F32(1) - o) * F32(1))), name
            assert same_bits(rec["changed_ori"][k], (ori[:, z, y, x] + F32(F32(1) - o) * d).astype(F32)), name
    k = ch[end_voxel(e["occ_not_one"][0])]
    assert rec["changed_occ"][k] != 1 and np.isnan(rec["changed_occ"][ch[end_voxel(e["occ_nan"][0])]])
    for name in ("occ_minus_zero", "occ_zero"):
        i = e[name][0]
        assert (st[i], sp[i], rt[i]) == (0, 2, 0) and len(calls(i)) == 1, name
    # acceptance: the cosine the reference computed is float32(0.5) or a neighbour of it
    for oname in ORIENTATIONS:
        for sname, call in (("pos", 0), ("neg", 1)):
            for tname, t in (("lo", HALF_LO), ("on", HALF), ("hi", HALF_HI)):
                i = e["cos_%s_%s_%s" % (oname, sname, tname)][0]
                assert bits(calls(i)[call]) == bits(t), (oname, sname, tname, calls(i))
                assert st[i] == 0 and (rt[i] == 0) == (tname == "hi")
    for form in FORMS:
        n_rows, trials = info["form_trials"][form]
        assert n_rows == len(e.get("form_" + form, [])) and (n_rows >= FORM_ROWS or trials >= FORM_TRIALS)
        for i in e.get("form_" + form, []):
            g = case["orientation"][i]
            c_ref = calls(i)[0]
            c_form = rs.cosine32(g, blend_rows(nrm[i]), form)
            assert bits(rs.cosine32(g, blend_rows(nrm[i]))) == bits(c_ref)
            assert (c_ref > HALF) != (c_form > HALF), (form, i, c_ref, c_form)
    # the sign of the bias
    for name, want in (("bias_zero", F32(0)), ("bias_plus_tiny", F32(1e-45)), ("bias_minus_tiny", F32(-1e-45))):
        i = e[name][0]
        assert bits(calls(i)[0]) == bits(want) and st[i] == 0 and rt[i] >= 1, (name, calls(i))
        assert np.array_equal(rec["last_normal"][i], EY * (-1 if name == "bias_minus_tiny" else 1))
        assert np.sign(rec["first_normal"][i][1]) == (-1 if name == "bias_minus_tiny" else 1)
    # steps and restarts
    for s in range(1, 10):
        i = e["step%d" % s][0]
        assert (st[i], sp[i]) == (0, s)
        tn = rec["total_normal"][rows(i)]
        assert len(tn) == s + 1 and np.array_equal(tn[-1], tn[-2])
    assert (st[e["step10"][0]], sp[e["step10"][0]]) == (2, 10) and len(calls(e["step10"][0])) == 0
    assert (st[e["restarts8"][0]], rt[e["restarts8"][0]]) == (0, 8) and (st[e["restarts9"][0]], rt[e["restarts9"][0]]) == (3, 9)
    i = e["param_div"][0]
    assert st[i] == 0 and sp[i] == info["param_div_step"]
    # voxel conversions
    assert st[e["index_k"][0]] == 0 and st[e["index_below_k"][0]] == 1
    for ax, name in enumerate(("negative_x", "negative_y", "negative_z")):
        i = e[name][0]
        f = (pts[i] * FLIP - rs.VMIN) / rs.VS32
        assert st[i] == 0 and -1 < f[ax] < 0 and vox[off[i]][ax] == 0
    if "lands_on_integer" in e:
        i = e["lands_on_integer"][0]
        assert (st[i], sp[i]) == (0, 1) and (rec["end_point"][i][0] - rs.VMIN[0]) / rs.VS32 == F32(info["step_lands_on_integer"][0])
    i = e["row_voxel_below"][0]
    assert st[i] == 0 and vox[off[i]][0] == rs.voxel32(pts[i])[0] - 1
    if "row_voxel_above" in e:
        i = e["row_voxel_above"][0]
        assert st[i] == 0 and vox[off[i]][0] == rs.voxel32(pts[i])[0] + 1
    # splat order: the shared voxel holds the row-order float32 sum, which is neither the reverse nor the float64 one
    four = e["splat_four"]
    assert (st[four] == 0).all() and len({tuple(vox[off[i]]) for i in four}) == 1
    units = []
    for i in four:
        t = rec["total_normal"][off[i]]
        units.append(t / rs.norm3(t, np.float64))
    fwd, rev, f64 = np.zeros(3, F32), np.zeros(3, F32), np.zeros(3)
    for u in units:
        fwd, f64 = (fwd.astype(np.float64) + u).astype(F32), f64 + u
    for u in units[::-1]:
        rev = (rev.astype(np.float64) + u).astype(F32)
    got = rec["changed_ori"][ch[tuple(vox[off[four[0]]][::-1].tolist())]]
    assert same_bits(got, fwd / F32(4)) and not same_bits(got, rev / F32(4)) and not same_bits(got, f64.astype(F32) / F32(4))
    _, cnt = np.unique(vox, axis=0, return_counts=True)
    i = e["one_row"][0]
    assert (vox == vox[off[i]]).all(1).sum() == 1 and (cnt == 1).any()
    # nothing outside, nothing of zero length, no two cases in one voxel
    f = (rec["total_sample"] * np.array([1.0, -1.0, -1.0]) - rs.VMIN.astype(np.float64)) / rs.VS
    assert ((f > -1) & (f < np.array([X, Y, Z]))).all() and (vox >= 0).all() and (vox < np.array([X, Y, Z])).all()
    assert rec["total_normal"].any(1).all()
    owner = {}
    for i in range(m):
        for v in map(tuple, vox[rows(i)].tolist()):
            names = set(names_of(e, [i], m)) - {"one_row"}
            assert owner.setdefault(v, names) & names or not names, (v, names, owner[v])
