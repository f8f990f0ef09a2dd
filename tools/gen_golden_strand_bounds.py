"""Golden vectors of the strand tracer's decisions on their bounds (tests/golden/strand_bounds.npz), run by the imported
reference on the CPU.

    python tools/gen_golden_strand_bounds.py

The cases come from tests/strand_bound_cases.py.  HairGrowing.trace and traceFromScalp are called seed by seed (trace's
own random shift is made zero for these calls, so that the walk starts from the exact seed the case asks for), trace
again with preset flag volumes, then GenerateGuideStrandFromScalp and randomlyGenerateSegments run as a whole under
torch.manual_seed.

Before the file is written, on the reference's output alone: every property a case exists for; the numpy restatement of
strand_bound_cases reproduces every record; each opposite form of a comparison changes at least one recorded strand and
only strands of the cases built for that bound.  The file holds data only and is written with fixed zip time stamps, so a
second run reproduces it byte for byte."""
import contextlib
import io
import os
import shutil
import sys
import tempfile
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

from ref_import import import_reference  # noqa: E402
import strand_bound_cases as C  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "strand_bounds.npz")
DRIVER_SEED = 77
# the guide run at the reference's default; the segment run at a bound low enough for the row of half-length steps to be
# walked, so that strands with two points in one voxel pass the gate again and again
GUIDE_THR, RANDOM_THR = 0.8, 0.05


def save_npz_fixed(path, arrays):
    """np.savez_compressed with a fixed time stamp in every zip entry"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[k]), allow_pickle=False)
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def same(a, b):
    """a strand or None against another"""
    if a is None or b is None:
        return a is None and b is None
    return a.shape == b.shape and np.array_equal(a, b)


def make_solver(HairGrow, c, tmp):
    import scipy.io

    occ, ori = C.volume_arrays(c)
    X, Y, Zd = C.DIMS
    o = ori.transpose((0, 1, 3, 2)).reshape(X, Y, Zd * 3).transpose((1, 0, 2))
    scipy.io.savemat(os.path.join(tmp, "Ori3D.mat"), {"Ori": o})
    scipy.io.savemat(os.path.join(tmp, "Occ3D.mat"), {"Occ": occ.transpose((1, 0, 2))})
    solver = HairGrow.HairGrowing(os.path.join(tmp, "Occ3D.mat"), os.path.join(tmp, "Ori3D.mat"), device="cpu")
    assert tuple(solver.occ.shape[1:]) == (Zd, Y, X)
    return solver


@contextlib.contextmanager
def no_shift():
    """trace draws its shift with torch.rand_like: zero for the per-seed calls"""
    orig = torch.rand_like
    torch.rand_like = lambda t, *a, **k: torch.zeros_like(t)
    try:
        yield
    finally:
        torch.rand_like = orig


def ref_trace(solver, seed, flag, thr):
    """the reference's trace from exactly `seed` -> strand or None"""
    X, Y, Zd = C.DIMS
    s_in = (np.asarray(seed, np.float32) - np.float32(0.5)).astype(np.float32)
    assert np.array_equal((s_in + np.float32(0.5)).astype(np.float32), seed), seed
    t = torch.from_numpy(s_in.copy())
    with no_shift():
        st = solver.trace(t, flag, thr, X, Y, Zd)
    assert np.array_equal(t.numpy(), seed)
    return None if st is False else st.numpy().copy()


def main():
    import_reference()
    os.chdir(tempfile.gettempdir())
    import HairGrow

    c = C.build_cases()
    vox = C.vox_of_cases(c)
    X, Y, Zd = C.DIMS
    tmp = tempfile.mkdtemp(prefix="mh_sb_")
    solver = make_solver(HairGrow, c, tmp)
    # the solver holds the volume as the restatement reads it, every bit (NaN, the denormals and -0.0 included)
    held = np.concatenate([solver.ori.numpy().transpose(1, 2, 3, 0), solver.occ.numpy().transpose(1, 2, 3, 0)], -1)
    assert held.dtype == np.float32 or np.array_equal(held.astype(np.float32).astype(held.dtype), held, equal_nan=True)
    assert np.array_equal(held.astype(np.float32).view(np.uint32), vox.view(np.uint32))

    out = {}
    nz = np.argwhere((c.e != 0).any(-1) | (c.occ != 0) | np.signbit(c.occ))
    occ64, ori64 = C.volume_arrays(c)
    out.update(shape=np.array(C.DIMS, np.int32), vol_nz=nz.astype(np.int16),
               vol_ori=ori64[tuple(nz.T)].astype(np.float32), vol_occ=occ64[tuple(nz.T)].astype(np.float32))

    # ---- trace, seed by seed, empty flag volume
    flag0 = torch.zeros_like(solver.occ)[0]
    rec_t = [ref_trace(solver, t["seed"], flag0, t["thr"]) for t in c.trace]
    assert float(flag0.max()) == 0
    first = []
    for t, st in zip(c.trace, rec_t):
        if st is None:
            first.append(-1)
            continue
        k = np.flatnonzero((st == t["seed"]).all(1))
        assert len(k) == 1, t["name"]
        first.append(256 - int(k[0]))
    out.update(trace_seeds=np.stack([t["seed"] for t in c.trace]), trace_thr=np.array([t["thr"] for t in c.trace]),
               trace_group=np.array([t["group"] for t in c.trace]), trace_name=np.array([t["name"] for t in c.trace]),
               trace_first=np.array(first, np.int32), trace_len=np.array([0 if s is None else len(s) for s in rec_t], np.int32),
               trace_pts=np.concatenate([s for s in rec_t if s is not None], 0))

    # ---- traceFromScalp, seed by seed
    rec_s = []
    for s in c.scalp:
        st = solver.traceFromScalp(torch.from_numpy(s["seed"].copy()), torch.from_numpy(s["normal"].copy()), s["thr"], X, Y, Zd, None)
        rec_s.append(None if st is None else st.numpy().copy())
    out.update(scalp_points=np.stack([s["seed"] for s in c.scalp]), scalp_normals=np.stack([s["normal"] for s in c.scalp]),
               scalp_thr=np.array([s["thr"] for s in c.scalp]), scalp_group=np.array([s["group"] for s in c.scalp]),
               scalp_name=np.array([s["name"] for s in c.scalp]),
               scalp_len=np.array([0 if s is None else len(s) for s in rec_s], np.int32),
               scalp_pts=np.concatenate([s for s in rec_s if s is not None], 0))

    # ---- trace with a preset flag volume
    rec_g = []
    for i, v in c.gate:
        flag = torch.zeros_like(solver.occ)[0]
        x, y, z = C.voxel_of(c.trace[i]["seed"])
        flag[z, y, x] = v
        rec_g.append(ref_trace(solver, c.trace[i]["seed"], flag, c.trace[i]["thr"]))
    out.update(gate_case=np.array([i for i, _ in c.gate], np.int32), gate_flag=np.array([v for _, v in c.gate], np.float32),
               gate_len=np.array([0 if s is None else len(s) for s in rec_g], np.int32))

    # ---- the two drivers, as a whole
    sp, sn = out["scalp_points"], out["scalp_normals"]
    drivers = {}
    for name in ("guide", "random"):
        solver = make_solver(HairGrow, c, tmp)
        torch.manual_seed(DRIVER_SEED)
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            if name == "guide":
                strands, num_root = solver.GenerateGuideStrandFromScalp(torch.from_numpy(sp.copy()), torch.from_numpy(sn.copy()),
                                                                        None, GUIDE_THR)
                out["guide_num_root"] = np.int32(num_root)
            else:
                strands = solver.randomlyGenerateSegments(RANDOM_THR)
        drivers[name] = [s.numpy().copy() for s in strands]
        out[name + "_len"] = np.array([len(s) for s in strands], np.int32)
        out[name + "_pts"] = np.concatenate(drivers[name], 0).astype(np.float32)
    out.update(driver_seed=np.int32(DRIVER_SEED), guide_thr=np.float64(GUIDE_THR), random_thr=np.float64(RANDOM_THR))
    shutil.rmtree(tmp)

    check_properties(c, vox, rec_t, rec_s, rec_g, drivers, int(out["guide_num_root"]))
    save_npz_fixed(OUT, out)
    print("strand_bounds written: %.1f kB, %d trace and %d scalp cases, guide %d strands, random %d strands" %
          (os.path.getsize(OUT) / 1024, len(c.trace), len(c.scalp), len(drivers["guide"]), len(drivers["random"])))


def driver_jitter(n_occ, rounds):
    torch.manual_seed(DRIVER_SEED)
    return torch.rand(rounds * n_occ, 3).numpy()


def check_properties(c, vox, rec_t, rec_s, rec_g, drivers, num_root):
    T = {t["name"]: (t, s) for t, s in zip(c.trace, rec_t)}
    S = {s["name"]: (s, r) for s, r in zip(c.scalp, rec_s)}
    ln = lambda r: 0 if r is None else len(r)      # noqa: E731

    # every per-seed walk stays in its own row
    for case, r in list(T.values()) + list(S.values()):
        if r is not None:
            idx = np.array([C.voxel_of(p) for p in r])
            assert (idx[:, 1] == case["row"][0]).all(), case["name"]
            if case["group"] != "s_zero":          # (these end in the empty rows kept free beside them)
                assert (idx[:, 2] == case["row"][1]).all(), case["name"]

    # ---- what each case exists for
    for thr in (C.THR8, C.THR7):
        lo, at, hi = (float(v) for v in C.around(thr))
        for d in "fb":
            assert [ln(T["thr%g_%r_%s" % (thr, v, d)][1]) for v in (lo, at, hi)] == [6, 7, 7], (thr, d)
        assert [ln(S["out_thr%g_%r" % (thr, v)][1]) for v in (lo, at, hi)] == [2, 3, 3]
        assert [ln(S["neg_thr%g_%r" % (thr, v)][1]) for v in (lo, at, hi)] == [2, 4, 4]
        turned = S["neg_thr%g_%r" % (thr, at)][1]
        assert turned[3, 0] == np.float32(turned[2, 0] + np.float32(thr)), "the step after the turn is +float32(thr)"
    assert float(np.float32(0.7)) < 0.7 and float(np.float32(0.8)) > 0.8
    for kind, want in (("hi", 7), ("lo", 6), ("eq", 7)):
        got = [ln(r) for t, r in T.values() if t["group"] == "t_round_" + kind]
        assert len(got) >= 8 and set(got) == {want}, (kind, got)
    assert [ln(T["occ_%r" % v][1]) for v in C.OCC_VALUES] == [7, 7, 7, 7, 7, 7, 0, 0]
    assert [ln(S["socc_%r" % v][1]) for v in C.OCC_VALUES] == [3, 3, 3, 3, 3, 3, 2, 2]
    five = {n: ln(T["five_" + n][1]) for n in ("4+0", "0+4", "2+2", "2+1", "3+0", "0+3", "5+0", "3+2")}
    assert five == {"4+0": 5, "0+4": 5, "2+2": 5, "2+1": 0, "3+0": 0, "0+3": 0, "5+0": 6, "3+2": 6}, five
    assert ln(T["at_k"][1]) == 8 and ln(T["below_k"][1]) == 0 and ln(T["step_on_int"][1]) == 7
    st = T["step_on_int"][1]
    assert (st[:, 0] == np.round(st[:, 0])).sum() == 6, "every step but the seed lands on an integer"
    for a in range(3):
        r = [T["axis%d_%g" % (a, v)][1] for v in (-0.25, -0.875, 0.25)]
        assert len({len(x) for x in r}) <= 2 and all(len(x) >= 7 for x in r)      # voxel 0 for all three seeds
        assert all(np.array_equal(x[1] - x[0], r[2][1] - r[2][0]) for x in r)
    assert ln(T["w_exact"][1]) == 264 and ln(T["w_minus"][1]) == 263 and ln(T["w_999"][1]) == 263
    rep = T["half_steps"][1]
    idx = np.array([C.voxel_of(p) for p in rep])
    assert len(rep) == 14 and (np.abs(np.diff(idx[:, 0])) == 0).sum() >= 6, "two consecutive points share a voxel"
    assert [ln(S["norm_" + k][1]) for k in ("below", "at", "above")] == [3, 2, 2]
    got = [ln(r) for s, r in S.values() if s["group"] == "s_norm3"]
    assert got.count(3) >= 4 and got.count(2) >= 4 and len(got) >= 8, got
    below, at, above = (S["d085_" + k][1] for k in ("below", "at", "above"))
    assert below[2, 1] == below[0, 1] and at[2, 1] > at[0, 1] and above[2, 1] > above[0, 1], "kept below 0.85, lifted from it on"
    lifts = {y: S["lift_%r" % y][1] for y in (0.0, -0.0, 1e-10, -1e-10, 0.5, -0.5, -1.0, -2.0)}
    assert all(len(v) == 2 for v in lifts.values())
    step = {y: v[1] - v[0] for y, v in lifts.items()}
    assert all(np.array_equal(step[y], step[0.0]) for y in (-0.0, 1e-10, -1e-10)), "y + 1 rounds to 1"
    assert step[-0.5][1] == 0 and step[-1.0][1] < 0 and step[-2.0][1] < step[-1.0][1] and step[0.5][1] > step[0.0][1]
    assert [ln(S["first_at_%d" % k][1]) for k in (24, 25, 26)] == [26, 27, 0]
    z = {v: S["zero_%r" % v][1] for v in (0.0, -0.0, C.TINY, -C.TINY)}
    assert all(len(v) == 3 for v in z.values())
    assert all(z[v][2, 2] > z[v][1, 2] for v in (0.0, -0.0, C.TINY)) and z[-C.TINY][2, 2] < z[-C.TINY][1, 2], "only dot < 0 turns"
    gate = {float(v): ln(r) for (_, v), r in zip(c.gate, rec_g)}
    assert gate == {0.0: 5, 2.0: 5, 2.5: 5, 3.0: 0, 4.0: 0}, gate

    # ---- the restatement reproduces every record
    def restate(f):
        t = [C.trace_gated_np(vox, np.zeros(vox.shape[:3], np.float32), x["seed"], x["thr"], f) for x in c.trace]
        s = [C.scalp_np(vox, x["seed"], x["normal"], x["thr"], f) for x in c.scalp]
        g = []
        for i, v in c.gate:
            flag = np.zeros(vox.shape[:3], np.float32)
            x, y, zz = C.voxel_of(c.trace[i]["seed"])
            flag[zz, y, x] = v
            g.append(C.trace_gated_np(vox, flag, c.trace[i]["seed"], c.trace[i]["thr"], f))
        return t, s, g

    t0, s0, g0 = restate(C.DEFAULT_FORMS)
    for a, b, x in zip(t0, rec_t, c.trace):
        assert same(a, b), ("trace", x["name"])
    for a, b, x in zip(s0, rec_s, c.scalp):
        assert same(a, b), ("scalp", x["name"])
    for a, b in zip(g0, rec_g):
        assert same(a, b)
    n_occ = int((vox[..., 3] != 0).sum())
    sp, sn = np.stack([s["seed"] for s in c.scalp]), np.stack([s["normal"] for s in c.scalp])

    def restate_drivers(f):
        g, nr = C.guide_np(vox, sp, sn, GUIDE_THR, driver_jitter(n_occ, 2), f)
        return g, nr, C.random_np(vox, RANDOM_THR, driver_jitter(n_occ, 3), f)

    g, nr, r = restate_drivers(C.DEFAULT_FORMS)
    assert nr == num_root and len(g) == len(drivers["guide"]) and len(r) == len(drivers["random"])
    assert all(same(a, b) for a, b in zip(g, drivers["guide"])) and all(same(a, b) for a, b in zip(r, drivers["random"]))

    # ---- the drivers' run: a seed whose trace has >= 5 points is refused by flag >= 3; an accepted strand with two
    # points in one voxel
    flag = np.zeros(vox.shape[:3], np.float32)
    pos = np.argwhere(vox[..., 3] != 0)[:, ::-1].astype(np.float32)
    jit = driver_jitter(n_occ, 3)
    refused = 0
    for rnd in range(3):
        for i in range(n_occ):
            pos[i] = pos[i] + np.float32(0.5)
            pos[i] = pos[i] + jit[rnd * n_occ + i] * np.float32(0.5)
            x, y, zz = C.voxel_of(pos[i])
            _, n, pts = C.trace_np(vox, pos[i], RANDOM_THR)
            if flag[zz, y, x] >= 3:
                refused += n >= 5
            elif n >= 5:
                C._mark(flag, pts, 0, C.DEFAULT_FORMS, C.DIMS)
    assert refused > 0, "no seed with a trace of >= 5 points refused by flag >= 3"
    shared = 0
    for s in drivers["random"] + drivers["guide"]:
        idx = np.array([C.voxel_of(p) for p in s])
        shared += len({tuple(i) for i in idx}) < len(idx)
    assert shared > 0, "no accepted strand with two points in one voxel"

    # ---- each opposite form changes at least one record, and only records of the cases built for that bound
    report = {}
    for name, sw in C.OPPOSITE_FORMS.items():
        f = C.forms(**sw)
        t1, s1, g1 = restate(f)
        changed = {x["group"] for a, b, x in zip(t1, rec_t, c.trace) if not same(a, b)}
        changed |= {x["group"] for a, b, x in zip(s1, rec_s, c.scalp) if not same(a, b)}
        gate_changed = any(not same(a, b) for a, b in zip(g1, rec_g))
        allowed = C.FORM_GROUPS[name]
        if name in ("flag_gt", "flag_per_point", "min_points_4", "min_points_6"):
            g, nr, r = restate_drivers(f)
            drv = not (len(g) == len(drivers["guide"]) and len(r) == len(drivers["random"]) and
                       all(same(a, b) for a, b in zip(g + r, drivers["guide"] + drivers["random"])))
        else:
            drv = None
        report[name] = (sorted(changed), gate_changed, drv)
        assert changed <= allowed, (name, changed - allowed)
        if name == "index_floor":
            assert not changed and not gate_changed, "floor and trunc agree after the clamp"
        elif name == "flag_gt":
            assert gate_changed and not changed and drv
        elif name == "flag_per_point":
            assert drv and not changed and not gate_changed
        else:
            assert changed, name
            assert not gate_changed or name in ("min_points_6",), name      # (the gated strand has five points)
    for k, v in report.items():
        print("  %-20s changes %s%s%s" % (k, ", ".join(v[0]) or "-", ", the gate records" if v[1] else "",
                                         "" if v[2] is None else (", the drivers' lists" if v[2] else ", NOT the drivers' lists")))


if __name__ == "__main__":
    main()
