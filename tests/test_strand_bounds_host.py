"""CPU: the strand tracer's decisions on their bounds (tests/strand_bound_cases.py) against what the reference recorded
on them (tests/golden/strand_bounds.npz, tools/gen_golden_strand_bounds.py): the C oracle, the numpy restatement with each
opposite form shown to fail on its own cases, the host gate mh_strands_accept through ctypes, and the occupancy rule held
to the installed torch.  Every comparison is equality."""
import ctypes
import os

import numpy as np
import pytest
import torch

import oracle
import strand_bound_cases as C
from conftest import GOLDEN


@pytest.fixture(scope="module")
def rec():
    z = np.load(os.path.join(GOLDEN, "strand_bounds.npz"))
    c = C.build_cases()
    vox = C.vox_of_cases(c)
    occ_r, ori_r = C.readers_arrays(c)
    vol = oracle.Volume(occ_r[..., 0], ori_r)
    return z, c, vox, vol


def split(pts, lens):
    o = np.concatenate([[0], np.cumsum(lens)])
    return [pts[o[i]:o[i + 1]] for i in range(len(lens))]


def same(a, b):
    if a is None or b is None or len(a) == 0 or len(b) == 0:
        return (a is None or len(a) == 0) and (b is None or len(b) == 0)
    return a.shape == b.shape and np.array_equal(a, b)


def test_fixture_holds_the_cases(rec):
    """the seeds, normals, thresholds and the volume of the fixture are the ones the module builds, bit for bit"""
    z, c, vox, vol = rec
    assert tuple(z["shape"]) == C.DIMS and len({*C.DIMS}) == 3
    assert np.array_equal(z["trace_seeds"], np.stack([t["seed"] for t in c.trace]))
    assert np.array_equal(z["trace_thr"], np.array([t["thr"] for t in c.trace]))
    assert np.array_equal(z["scalp_points"], np.stack([s["seed"] for s in c.scalp]))
    assert np.array_equal(z["scalp_normals"].view(np.uint32), np.stack([s["normal"] for s in c.scalp]).view(np.uint32))
    assert list(z["trace_name"]) == [t["name"] for t in c.trace] and list(z["scalp_name"]) == [s["name"] for s in c.scalp]
    occ = np.zeros(C.DIMS, np.float32)
    ori = np.zeros(C.DIMS + (3,), np.float32)
    nz = tuple(z["vol_nz"].T.astype(np.int64))
    occ[nz], ori[nz] = z["vol_occ"], z["vol_ori"]
    built = np.concatenate([ori * np.array([1, -1, -1], np.float32), occ[..., None]], -1).transpose(2, 1, 0, 3)
    built = np.ascontiguousarray(built)
    # (the fixture lists the voxels that hold something: elsewhere the sign of a zero orientation is not recorded)
    assert np.array_equal(built, vox, equal_nan=True)
    assert np.array_equal(built[..., 3].view(np.uint32), vox[..., 3].view(np.uint32))
    assert np.array_equal(vol.vox.view(np.uint32), vox.view(np.uint32))
    assert len(c.trace) <= 1024 and len(c.scalp) <= 256


def test_oracle_equals_the_record(rec):
    """oracle.trace_seeds / trace_scalp on every seed: first, len and every point"""
    z, c, vox, vol = rec
    ref = split(z["trace_pts"], z["trace_len"])
    for thr in sorted(set(z["trace_thr"])):
        sel = np.flatnonzero(z["trace_thr"] == thr)
        out, first, ln = oracle.trace_seeds(vol, z["trace_seeds"][sel], thr)
        for k, i in enumerate(sel):
            if z["trace_len"][i] == 0:
                assert ln[k] < 5, c.trace[i]["name"]
            else:
                assert (first[k], ln[k]) == (z["trace_first"][i], z["trace_len"][i]), c.trace[i]["name"]
                assert np.array_equal(out[k, first[k]:first[k] + ln[k]], ref[i]), c.trace[i]["name"]
    ref = split(z["scalp_pts"], z["scalp_len"])
    for thr in sorted(set(z["scalp_thr"])):
        sel = np.flatnonzero(z["scalp_thr"] == thr)
        out, ln = oracle.trace_scalp(vol, z["scalp_points"][sel], z["scalp_normals"][sel], thr)
        for k, i in enumerate(sel):
            assert ln[k] == z["scalp_len"][i], c.scalp[i]["name"]
            assert np.array_equal(out[k, :ln[k]], ref[i]), c.scalp[i]["name"]


def _restate(c, vox, f):
    zero = np.zeros(vox.shape[:3], np.float32)
    t = [C.trace_gated_np(vox, zero, x["seed"], x["thr"], f) for x in c.trace]
    s = [C.scalp_np(vox, x["seed"], x["normal"], x["thr"], f) for x in c.scalp]
    g = []
    for i, v in c.gate:
        flag = zero.copy()
        x, y, zz = C.voxel_of(c.trace[i]["seed"])
        flag[zz, y, x] = v
        g.append(C.trace_gated_np(vox, flag, c.trace[i]["seed"], c.trace[i]["thr"], f))
    return t, s, g


def _changed(z, c, t, s, g):
    rt, rs = split(z["trace_pts"], z["trace_len"]), split(z["scalp_pts"], z["scalp_len"])
    groups = {x["group"] for a, b, x in zip(t, rt, c.trace) if not same(a, b)}
    groups |= {x["group"] for a, b, x in zip(s, rs, c.scalp) if not same(a, b)}
    gate = [0 if a is None else len(a) for a in g] != list(z["gate_len"])
    return groups, gate


def test_restatement_equals_the_record(rec):
    z, c, vox, vol = rec
    groups, gate = _changed(z, c, *_restate(c, vox, C.DEFAULT_FORMS))
    assert not groups and not gate
    assert list(z["gate_flag"]) == [0.0, 2.0, 2.5, 3.0, 4.0] and list(z["gate_len"]) == [5, 5, 5, 0, 0]


@pytest.mark.parametrize("name", sorted(C.OPPOSITE_FORMS))
def test_opposite_form_fails_on_its_own_cases(rec, name):
    """the opposite operator, order or precision changes recorded rows, and only rows of the cases built for that bound.
    floor for truncation changes none and cannot (the clamp that follows makes -1 and 0 the same voxel); the flag forms
    change the gate's records or the drivers' lists (test_drivers_restated)"""
    z, c, vox, vol = rec
    groups, gate = _changed(z, c, *_restate(c, vox, C.forms(**C.OPPOSITE_FORMS[name])))
    assert groups <= C.FORM_GROUPS[name], groups - C.FORM_GROUPS[name]
    if name == "index_floor":
        assert not groups and not gate
    elif name == "flag_gt":
        assert gate and not groups
    elif name == "flag_per_point":
        assert not gate and not groups
    else:
        assert groups


@pytest.fixture(scope="module")
def drivers(rec):
    z, c, vox, vol = rec
    n_occ = int((vox[..., 3] != 0).sum())

    def jitter(rounds):
        torch.manual_seed(int(z["driver_seed"]))
        return torch.rand(rounds * n_occ, 3).numpy()
    return n_occ, jitter


def _lists_equal(z, guide, num_root, random):
    return (num_root == int(z["guide_num_root"]) and [len(s) for s in guide] == list(z["guide_len"]) and
            [len(s) for s in random] == list(z["random_len"]) and
            np.array_equal(np.concatenate(guide, 0), z["guide_pts"]) and np.array_equal(np.concatenate(random, 0), z["random_pts"]))


def test_drivers_restated(rec, drivers):
    """both drivers as a whole: the restatement equals the reference's lists; counting a repeated voxel once per point, or
    `flag > 3`, or another point minimum gives other lists"""
    z, c, vox, vol = rec
    n_occ, jitter = drivers
    sp, sn = z["scalp_points"], z["scalp_normals"]

    def run(f):
        g, nr = C.guide_np(vox, sp, sn, float(z["guide_thr"]), jitter(2), f)
        return g, nr, C.random_np(vox, float(z["random_thr"]), jitter(3), f)
    assert _lists_equal(z, *run(C.DEFAULT_FORMS))
    for name in ("flag_per_point", "flag_gt", "min_points_4", "min_points_6"):
        assert not _lists_equal(z, *run(C.forms(**C.OPPOSITE_FORMS[name]))), name
    shared = sum(len({C.voxel_of(p) for p in s}) < len(s) for s in split(z["random_pts"], z["random_len"]))
    assert shared > 0


def test_oracle_drivers_equal_the_record(rec, drivers):
    z, c, vox, vol = rec
    n_occ, jitter = drivers
    g, nr, _ = oracle.generate_guide_strands(vol, z["scalp_points"], z["scalp_normals"], float(z["guide_thr"]), jitter(2))
    r, _ = oracle.randomly_generate_segments(vol, float(z["random_thr"]), jitter(3))
    assert _lists_equal(z, g, nr, r)


def _accept(vox_dims, flag, pts, first, ln, seeds, mode):
    from monohair_amd import _lib

    L = _lib.lib()
    acc = np.zeros(len(ln), np.uint8)
    p = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    rc = L.mh_strands_accept(vox_dims[0], vox_dims[1], vox_dims[2], p(flag), p(pts), p(first), p(ln), pts.shape[1], p(seeds),
                             len(ln), mode, p(acc))
    assert rc == 0
    return acc.astype(bool)


def test_strands_accept_equals_the_recorded_gate(rec, drivers):
    """mh_strands_accept through ctypes on the oracle's traces: the preset flag values at a seed voxel (2, 2.5 pass, 3
    does not), the strands of 4 and 5 points, and both drivers' whole lists with their repeated voxels"""
    z, c, vox, vol = rec
    n_occ, jitter = drivers
    # per-seed records: every trace case behind an empty flag volume, the gate cases behind their preset value
    for thr in sorted(set(z["trace_thr"])):
        sel = np.flatnonzero(z["trace_thr"] == thr)
        seeds = np.ascontiguousarray(z["trace_seeds"][sel])
        out, first, ln = oracle.trace_seeds(vol, seeds, thr)
        for k, i in enumerate(sel):            # one call per seed: the record is of one call with an empty flag volume
            flag = np.zeros(vox.shape[:3], np.float32)
            acc = _accept(C.DIMS, flag, out[k:k + 1], first[k:k + 1], ln[k:k + 1], seeds[k:k + 1], 0)
            assert bool(acc[0]) == bool(z["trace_len"][i] > 0), c.trace[i]["name"]
            idx = np.array([C.voxel_of(p) for p in out[k, first[k]:first[k] + ln[k]]])
            want = np.zeros_like(flag)
            if acc[0]:
                want[idx[:, 2], idx[:, 1], idx[:, 0]] = 1          # once per distinct voxel
            assert np.array_equal(flag, want), c.trace[i]["name"]
    for (i, v), want in zip(c.gate, z["gate_len"]):
        seeds = np.ascontiguousarray(z["trace_seeds"][i:i + 1])
        out, first, ln = oracle.trace_seeds(vol, seeds, float(z["trace_thr"][i]))
        flag = np.zeros(vox.shape[:3], np.float32)
        x, y, zz = C.voxel_of(seeds[0])
        flag[zz, y, x] = v
        assert bool(_accept(C.DIMS, flag, out, first, ln, seeds, 0)[0]) == bool(want > 0), v
    # the drivers: the oracle's traces through the library's gate
    for name, rounds in (("guide", 2), ("random", 3)):
        thr = float(z[name + "_thr"])
        flag = np.zeros(vox.shape[:3], np.float32)
        strands = []
        if name == "guide":
            sp, sl = oracle.trace_scalp(vol, z["scalp_points"], z["scalp_normals"], thr)
            acc = _accept(C.DIMS, flag, sp, np.zeros(len(sl), np.int32), sl, np.ascontiguousarray(z["scalp_points"]), 1)
            strands += [sp[i, :sl[i]] for i in np.flatnonzero(acc)]
            assert len(strands) == int(z["guide_num_root"])
        pos = np.argwhere(vox[..., 3] != 0)[:, ::-1].astype(np.float32)
        jit, seeds = jitter(rounds), []
        for r in range(rounds):
            pos = pos + np.float32(0.5)
            pos = pos + jit[r * n_occ:(r + 1) * n_occ] * np.float32(0.5)
            seeds.append(pos)
        seeds = np.ascontiguousarray(np.concatenate(seeds, 0))
        out, first, ln = oracle.trace_seeds(vol, seeds, thr)
        acc = _accept(C.DIMS, flag, out, first, ln, seeds, 0)
        assert (~acc & (ln >= 5)).any(), "no seed with a trace of >= 5 points refused by flag >= 3"
        strands += [out[i, first[i]:first[i] + ln[i]] for i in np.flatnonzero(acc)]
        assert [len(s) for s in strands] == list(z[name + "_len"])
        assert np.array_equal(np.concatenate(strands, 0), z[name + "_pts"])


# ---------------------------------------------------------------------------------------------- the occupancy ratio
def _torch_status(strand, occ_t):
    """the lines of the reference's test (HairGrow.py:521-528) with the installed torch"""
    p = torch.from_numpy(np.asarray(strand, np.float64).copy())
    vmin = torch.tensor([-0.32, -0.32, -0.24], dtype=torch.float)
    p[..., 1:] *= -1
    idx = torch.round((p - vmin) / (0.005 / 2)).type(torch.long)
    if torch.max(idx[:, 2]) >= 192 or torch.max(idx[:, 1] >= 256) or torch.max(idx[:, 0] >= 256):
        return 2
    try:
        v = occ_t[0, idx[:, 2], idx[:, 1], idx[:, 0]]
    except IndexError:
        return 3
    return int(bool(torch.sum(v) / v.size(0) > 0.8))


def test_occupancy_rule_is_torchs(rec):
    """the restatement of the occupancy test, torch's own ops and monohair_amd.hairgrow._occ_eval_host agree on every
    strand: the ratio exactly 0.8 is rejected (4/5, 8/10, 12/15), 5/6 and 9/11 pass, k + 1/2 goes to the even index, an
    index of 256 / 256 / 192 leaves the box, a negative index wraps down to -dim and is refused below it"""
    from monohair_amd import _lib
    from monohair_amd.hairgrow import _occ_eval_host

    occ = C.occ_volume()
    occ_t = torch.from_numpy(occ)[None]
    S, names = C.occ_strands()
    got = {}
    for s, n in zip(S, names):
        st = C.occ_status_np(s, occ)
        assert st == _torch_status(s, occ_t), n
        if st == 3:
            with pytest.raises(_lib.MhError):
                _occ_eval_host(s.copy(), occ)
        else:
            assert _occ_eval_host(s.copy(), occ) == st, n
        got[n] = st
    assert [got["ratio_%d_of_%d" % k] for k in ((4, 5), (8, 10), (12, 15), (5, 6), (9, 11), (7, 7), (0, 7))] == [0, 0, 0, 1, 1, 1, 0]
    for axis in range(3):
        # index 50 + 60 + 70 is even; k + 1/2 rounds to the even one of k and k + 1, replacing that axis' index
        base = 180 - (50, 60, 70)[axis]
        ks = [k for k, _ in C.half_indices(axis)]
        assert sum(k % 2 for k in ks) == 2 and len(ks) == 4
        for k in ks:
            even = k if k % 2 == 0 else k + 1
            assert got["half_axis%d_%d" % (axis, k)] == int((base + even) % 2 == 0), (axis, k)
        assert got["face_axis%d_%d" % (axis, C.BOX[axis])] == 2 and got["face_axis%d_%d" % (axis, C.BOX[axis] - 1)] in (0, 1)
        assert all(got["neg_axis%d_%d" % (axis, v)] in (0, 1) for v in (-1, -2, -C.BOX[axis]))
    assert got["refused_x"] == 3 and got["box_and_refused"] == 2
    # the opposite forms change rows: >= accepts 4/5; half away from zero moves k + 1/2 for even k; a float64 bound
    # accepts float32(4/5) = 0.800000011920929 > 0.8
    ge = [C.occ_status_np(s, occ, ratio_op=">=") for s in S]
    up = [C.occ_status_np(s, occ, rounding="up") for s in S]
    d64 = [C.occ_status_np(s, occ, thr64=True) for s in S]
    base = [got[n] for n in names]
    assert ge[names.index("ratio_4_of_5")] == 1 and up != base and d64[names.index("ratio_8_of_10")] == 1
    assert [n for n, a, b in zip(names, up, base) if a != b] == ["half_axis%d_%d" % (a, k) for a in range(3) for k, _ in C.half_indices(a) if k % 2 == 0]
    # float32 facts the cases rest on
    t = lambda a, n: bool(torch.tensor(float(a)) / n > 0.8)      # noqa: E731
    assert [t(4, 5), t(8, 10), t(5, 6), t(9, 11)] == [False, False, True, True]
    assert not bool(torch.tensor(0.7) < 0.7) and float(np.float32(0.7)) < 0.7


def test_torch_dot_and_norm_forms():
    """torch.dot of three float32 is the left-to-right sum of separately rounded products and torch.linalg.norm the root
    of the fma chain, on the very pairs and rows whose other forms decide differently"""
    pairs = C.search_dot_pairs()
    for kind in ("hi", "lo", "eq"):
        T, N = pairs[kind]
        assert len(T) >= 8
        for a, b in zip(T, N):
            d = torch.dot(torch.from_numpy(b), torch.from_numpy(a)).numpy()
            assert d == C.dot3(b, a, "ltr")
            others = (C.dot3(b, a, "rtl"), C.dot3(b, a, "fma"))
            thr = np.float32(0.8)
            if kind == "hi":
                assert d >= thr and min(others) < thr
            elif kind == "lo":
                assert d < thr and max(others) >= thr
            else:
                assert d == thr
    rows = C.search_norm_rows()
    sides = 0
    for v in rows:
        n = torch.linalg.norm(torch.from_numpy(v), 2).numpy()
        assert n == C.norm3(v, "fma")
        assert (n < np.float32(0.1)) != (C.norm3(v, "plain") < np.float32(0.1))
        sides += int(n < np.float32(0.1))
    assert len(rows) >= 8 and 0 < sides < len(rows)
    below, at, above = (C.norm3(np.array([v, 0, 0], np.float32)) for v in C.search_norm_axis())
    assert (below, at, above) == C.around(0.1)
