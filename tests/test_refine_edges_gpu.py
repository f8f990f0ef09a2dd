"""GPU: refine()'s decisions with the compared value ON its bound and one float either side (tests/refine_edge_cases.py,
tests/golden/refine_edges.npz, tools/gen_golden_refine_edges.py; tests/test_refine_edges_host.py holds the oracle and the numpy
restatements to the same record): the 0.95 rule in mh_replace_dissimilar and mh_refine_combine, the 4 cm and the height test
of mh_nearest_distance, mh_flag_less, the sign flip / p2v / stable order of mh_voxel_group with the fits built on it, and
refine() itself in every form of the driver.  Plain equality everywhere (NaN == NaN; the sign of a zero where `* -1` decides
it).  Reads the fixture only."""
import ctypes
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.spatial import KDTree

import refine_edge_cases as rc

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
SIZES = (1, 255, 256, 257)
FORMS = {"device_pass": ({}, "device"), "host_driven": ({"MH_REFINE_DEVICE": "0"}, "device"),
         "four_launches": ({"MH_REFINE_CHAIN": "0"}, "device"), "host_knn": ({}, "host")}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return t.cpu().numpy()


def ctx():
    from monohair_amd.pmvo_utils import _ctx_for

    return _ctx_for(DEV)


@pytest.fixture(scope="module")
def fx():
    return rc.load()


@pytest.fixture(scope="module")
def sweep():
    """(center, ori, torch's max-cosine on the CPU, the replaced rows) with rows on the bound, its neighbours and the degenerate
    rows in front, so that the launches of 1, 255, 256 and 257 rows hold them"""
    c, o = rc.cos_sweep()
    sim = rc.max_cos(c, o)
    with np.errstate(invalid="ignore"):
        front = np.concatenate([np.flatnonzero(sim[:20000] == v)[:40] for v in (rc.COS, rc.COS_LO, rc.COS_HI)]
                               + [np.linspace(20000, len(c) - 1, 120).astype(np.int64)])
    order = np.concatenate([front, np.setdiff1d(np.arange(len(c)), front)])        # (row 0 sits on the bound itself)
    c, o, sim = c[order], o[order], sim[order]
    with np.errstate(invalid="ignore"):
        assert sim[0] == rc.COS and all((sim[:255] == v).sum() >= 10 for v in (rc.COS, rc.COS_LO, rc.COS_HI))
        assert np.isnan(sim[:255]).sum() >= 5
        return c, o, sim, rc.replace_rule(sim, c, o)


@pytest.mark.parametrize("n", SIZES + (None,))
def test_replacement_rule_across_the_bound(sweep, n):
    """mh_replace_dissimilar, and mh_refine_combine with `ori` given and without, against torch.cosine_similarity on the CPU:
    head flags that give -1 -> 0.5, a loss that is -1 already, NaN losses"""
    from monohair_amd import _lib

    c, o, sim, want = (a[:n] for a in sweep)
    N = len(c)
    L, st = _lib.lib(), _lib.stream_ptr()
    cd, got = dev(c), dev(o)
    _lib.check(L.mh_replace_dissimilar(ctx(), _lib.ptr(cd), _lib.ptr(got), 0.95, N, st), "mh_replace_dissimilar")
    assert rc.bits_equal(host(got), want)
    rng = np.random.default_rng(3)
    loss_u = rng.random(N).astype(F)
    loss_u[::5], loss_u[1::7], loss_u[2::11] = np.nan, -1.0, 0.5
    head, top = (rng.random(N) < 0.5).astype(np.uint8), (rng.random(N) < 0.5).astype(np.uint8)
    head[:2], top[:2] = 1, (0, 1)[:N]
    want_loss = np.where((head != 0) & (top == 0), F(-1), loss_u)
    want_loss = np.where(want_loss == -1, F(0.5), want_loss).astype(F)
    lu, hd, td = dev(loss_u), dev(head), dev(top)
    for with_ori in (True, False):
        got, out = dev(o), torch.full((N,), 7.0, device=DEV)
        _lib.check(L.mh_refine_combine(ctx(), _lib.ptr(cd), _lib.ptr(lu), _lib.ptr(hd), _lib.ptr(td), 0.95,
                                       _lib.ptr(got) if with_ori else None, _lib.ptr(out), N, st), "mh_refine_combine")
        assert rc.eq(host(out), want_loss), with_ori
        assert rc.bits_equal(host(got), want if with_ori else o), with_ori


def scalp_of(z, M):
    """M vertices: random ones 6 cm or more from the six designed points, then the vertices of the two neighbours of 0.04, of
    the height points and -- twice, as the last two vertices -- the one exactly 0.04 away: with M = 1025 and 2049 the two copies
    lie either side of a border of the kernel's 1024-vertex tiles, the second alone in the last tile"""
    sa = z["loop_scalp_a"]
    v_eq, v_lo, v_hi, v_h = sa[0], sa[1], sa[2], sa[3]
    if M == 1:
        return v_eq[None].copy()
    pts = z["loop_points"][np.concatenate([z["loop_rows_dist"], z["loop_rows_height"]])].astype(np.float64)
    rng = np.random.default_rng(M)
    r = rng.uniform(-0.3, 0.3, (4 * M, 3))
    r = r[np.linalg.norm(r[:, None] - pts[None], axis=-1).min(1) > 0.06][:M - 5]
    assert len(r) == M - 5
    return np.concatenate([r, [v_lo, v_hi, v_h, v_eq, v_eq]])


@pytest.mark.parametrize("M", [1, 1023, 1024, 1025, 2049])
def test_scalp_distance_and_height_on_the_bounds(fx, M):
    """mh_nearest_distance == scipy's KDTree in float64: distance, mask, and the mask alone -- with L no float32 (z ==
    float32(L) < L is below it) and with L that float32 itself (it is not)"""
    from monohair_amd import _lib

    _, z = fx
    scalp = scalp_of(z, M)
    La, Lb = (float(v) for v in z["loop_L"])
    first = np.concatenate([z["loop_rows_dist"], z["loop_rows_height"]])
    pts_all = np.concatenate([z["loop_points"][first], np.delete(z["loop_points"], first, 0)])
    ref = dev(scalp)
    for N in SIZES:
        pts = pts_all[:N]
        want_d, _ = KDTree(data=scalp).query(pts, k=1)
        want_m = rc.head_top_rule(want_d, pts[:, 2], La)
        assert want_d[0] == rc.DIST
        if N > 1 and M > 1:
            assert list(want_d[:3]) == [rc.DIST, rc.DIST_LO, rc.DIST_HI] and list(want_m[:6]) == [0, 1, 0, 1, 1, 0]
        p = dev(pts)
        d = torch.empty((N,), dtype=torch.float64, device=DEV)
        m, m2 = torch.full((N,), 9, dtype=torch.uint8, device=DEV), torch.full((N,), 9, dtype=torch.uint8, device=DEV)
        call = lambda out, mask, L: _lib.check(_lib.lib().mh_nearest_distance(                        # noqa: E731
            ctx(), _lib.ptr(p), N, _lib.ptr(ref), M, _lib.ptr(out), 0.04, L, _lib.ptr(mask), _lib.stream_ptr()), "mh_nearest_distance")
        call(d, m, La)
        call(None, m2, La)
        assert np.array_equal(host(d), want_d), (M, N)
        assert np.array_equal(host(m).astype(bool), want_m) and np.array_equal(host(m2).astype(bool), want_m), (M, N)
        want_b = rc.head_top_rule(want_d, pts[:, 2], Lb)
        if N > 1 and M > 1:
            assert list(want_b[:6]) == [0, 1, 0, 0, 1, 0]
        call(None, m2, Lb)
        assert np.array_equal(host(m2).astype(bool), want_b), (M, N)


@pytest.fixture(scope="module")
def scene():
    import golden_drivers

    _, meta, pm = golden_drivers.golden_pmvo(DEV)
    return meta, pm


def test_head_top_mask_on_the_loop_case(fx, scene):
    """PMVO.head_top_mask and head_top_mask_device with both scalps: L no float32 (the float64 rule decides z == float32(L)) and
    L a float32 (`<` decides it)"""
    _, z = fx
    _, pm = scene
    pts = z["loop_points"]
    for s, ml in (("a", z["loop_ref_min_loss"]), ("b", z["loop_b_min_loss"])):
        scalp = z["loop_scalp_" + s]
        pm.set_head(None, KDTree(data=scalp), np.max(scalp, axis=0))
        want = rc.head_top_rule(z["loop_dist"], pts[:, 2], float(z["loop_L"]["ab".index(s)]))
        assert np.array_equal(z["loop_votes"] & ~want, ml == 0.5)
        assert np.array_equal(pm.head_top_mask(pts), want), s
        assert np.array_equal(host(pm.head_top_mask_device(dev(pts))).astype(bool), want), s


def test_flag_less_on_the_threshold(fx):
    from monohair_amd import _lib

    _, z = fx
    x = np.concatenate([z["fit_loss"], z["loop_ref_min_loss"], np.array([0.0, -0.0, 0.05, 0.5], F)])
    zeros = np.array([0.0, -0.0], F)
    with np.errstate(invalid="ignore"):
        for xs, thr in [(x, 0.05), (x, 0.5), (x, float(z["loop_thresholds"][1])), (x, float(z["loop_thresholds"][2])),
                        (zeros, 0.0), (zeros, -0.0), (x, 0.0), (x, -0.0)]:
            xd, out = dev(xs), torch.full((len(xs),), 9, dtype=torch.uint8, device=DEV)
            _lib.check(_lib.lib().mh_flag_less(ctx(), _lib.ptr(xd), thr, len(xs), _lib.ptr(out), _lib.stream_ptr()), "mh_flag_less")
            want = xs < F(thr)
            assert np.array_equal(host(out), want.astype(np.uint8)), thr
            assert not want[xs == F(thr)].any() and not want[np.isnan(xs)].any()
    assert (x == F(0.05)).any() and (x == F(0.5)).sum() > 50 and np.isnan(x).any()


def voxel_group(pts, ori, vmin, vs, grid):
    """mh_voxel_group -> (sorted keys, order, canonicalised rows in that order)"""
    from monohair_amd import _lib

    L, n = _lib.lib(), len(pts)
    ks, order, o = (torch.empty(n, dtype=torch.int64, device=DEV), torch.empty(n, dtype=torch.int32, device=DEV),
                    torch.empty((n, 3), dtype=torch.float32, device=DEV))
    scratch = torch.empty(int(L.mh_voxel_group_scratch_bytes(n)), dtype=torch.uint8, device=DEV)
    vmin, dims = np.ascontiguousarray(vmin, np.float64), np.ascontiguousarray(grid, np.int32)
    pd, od = dev(pts), dev(ori)
    _lib.check(L.mh_voxel_group(ctx(), _lib.ptr(pd), 1 if pts.dtype == np.float64 else 0, _lib.ptr(od), n,
                                vmin.ctypes.data_as(ctypes.c_void_p), float(vs), dims.ctypes.data_as(ctypes.c_void_p),
                                _lib.ptr(scratch), scratch.numel(), _lib.ptr(ks), _lib.ptr(order), _lib.ptr(o), _lib.stream_ptr()),
               "mh_voxel_group")
    return host(ks), host(order), host(o)


def check_group_and_fits(pts, ori, n_surface, vmin, vs, grid, want_vox=None, want_ori=None):
    from monohair_amd import pmvo_utils as U

    g = np.asarray(grid).astype(np.int64)
    k = rc.p2v_rule(pts, vmin, vs, grid)
    key = (k[:, 0] * g[1] + k[:, 1]) * g[2] + k[:, 2]
    want_order = np.argsort(key, kind="stable")
    ks, order, rows = voxel_group(pts, ori, vmin, vs, grid)
    assert np.array_equal(ks, key[want_order]) and np.array_equal(order, want_order)
    assert rc.bits_equal(rows, rc.canon_rule(ori)[want_order])
    vox, med, scores = rc.fit_rule(pts, ori, n_surface, vmin, vs, grid)
    assert any(len(s) == 1 for s in scores)                                     # (a group of one)
    if want_vox is not None:
        assert np.array_equal(vox, want_vox) and rc.bits_equal(med, want_ori)
    res = U.voxel_fit(pts, ori, DEV, vmin, vs, grid, dense=False)
    assert np.array_equal(host(res["voxels"]), vox) and rc.bits_equal(host(res["ori"]), med)
    if pts.dtype == np.float32:
        v2, m2 = U.voxel_fit_device(dev(pts), dev(ori), len(pts), DEV, vmin, vs, grid)
        assert np.array_equal(v2, vox) and rc.bits_equal(m2, med)


@pytest.mark.parametrize("name", ["f32", "f64"])
def test_voxel_keys_on_halves_and_outside_int32(fx, name):
    """case p2v: the keys equal the reference's recorded indices; order, canonicalised rows (the rows of case fit, zeros of both
    signs among them) and both fits against the restatement"""
    _, z = fx
    pts, idx = z["p2v_%s_points" % name], z["p2v_%s_index" % name].astype(np.int64)
    ori = np.resize(z["fit_ori"][110:], (len(pts), 3)).astype(F)
    g = rc.BIN_GRID.astype(np.int64)
    ks, _, _ = voxel_group(pts, ori, rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID)
    assert np.array_equal(ks, np.sort((idx[:, 0] * g[1] + idx[:, 1]) * g[2] + idx[:, 2]))
    check_group_and_fits(pts, ori, len(pts), rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID)


def fit_inputs(z):
    kept = rc.keep_rule(z["fit_loss"], rc.FIT_THR)
    return (np.concatenate([z["fit_points"][kept], z["fit_filter_unvisible"]]),
            np.concatenate([z["fit_ori"][kept], z["fit_filter_unvisible_ori"]]), len(kept))


def test_voxel_fit_on_the_hand_written_rows(fx):
    """case fit: sign flip at y = +-0 / +-1e-45 / tiny, points outside the six faces and at +-1e7, exact ties in both member
    orders and between a surface and a shell row -- the reference's recorded voxels and orientations"""
    _, z = fx
    p, o, n_surface = fit_inputs(z)
    check_group_and_fits(p, o, n_surface, rc.VOXEL_MIN, rc.VOXEL_SIZE, rc.GRID, z["fit_voxels"], z["fit_voxel_ori"])


def run_refine(scene, tmp_path, monkeypatch, form, points, ori, loss, shell, threshold, only=False, dense=False):
    import golden_drivers
    from monohair_amd.pmvo import refine

    meta, pm = scene
    env, knn = FORMS[form]
    for k in ("MH_REFINE_DEVICE", "MH_REFINE_CHAIN"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    args = golden_drivers.driver_args(str(tmp_path), meta)
    args.knn = knn
    if only:
        for k, v in (("select_p", points), ("select_o", ori), ("min_loss", loss)):
            np.save(os.path.join(args.save_path, k + ".npy"), v)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                   # (numpy's cast of 4e9 to int32 warns)
        res = refine(points.copy(), ori.copy(), loss.copy(), pm, shell.copy(), args, infer_inner=False, threshold=threshold,
                     genrate_ori_only=only, return_dense=dense)
    return res, {k: np.load(os.path.join(args.save_path, k + ".npy")) for k in rc.FILES}, dict(pm.last_refine)


@pytest.mark.parametrize("form", list(FORMS))
def test_refine_on_the_loop_case(fx, scene, tmp_path, monkeypatch, form):
    """refine() on case loop with scalp "a" at the three thresholds and with scalp "b": the reference's five files"""
    _, z = fx
    _, pm = scene
    runs = [("a", "loop_t%d_" % i, float(t), z["loop_ref_min_loss"]) for i, t in enumerate(z["loop_thresholds"])]
    runs.append(("b", "loop_b_", 0.5, z["loop_b_min_loss"]))
    for i, (s, key, thr, want_loss) in enumerate(runs):
        scalp = z["loop_scalp_" + s]
        pm.set_head(None, KDTree(data=scalp), np.max(scalp, axis=0))
        _, got, info = run_refine(scene, tmp_path / str(i), monkeypatch, form, z["loop_points"], z["loop_ori"], z["loop_loss"],
                                  z["loop_shell"], thr)
        assert info["device_pass"] == (form == "device_pass"), info
        assert rc.eq(got["select_p"], z["loop_ref_select_p"]) and rc.eq(got["select_o"], z["loop_ref_select_o"]), (form, key)
        assert rc.eq(got["min_loss"], want_loss), (form, key, np.flatnonzero(got["min_loss"] != want_loss))
        for k in ("filter_unvisible", "filter_unvisible_ori"):
            assert got[k].dtype == np.float32 and rc.eq(got[k], z[key + k]), (form, key, k)


@pytest.mark.parametrize("form", ["device_pass", "host_knn"])
def test_refine_on_the_hand_written_files(fx, scene, tmp_path, monkeypatch, form):
    """refine(genrate_ori_only=True) on case fit: both shell files, the voxels and their orientations"""
    _, z = fx
    _, pm = scene
    scalp = z["loop_scalp_a"]
    pm.set_head(None, KDTree(data=scalp), np.max(scalp, axis=0))
    (occ, ori), got, _ = run_refine(scene, tmp_path, monkeypatch, form, z["fit_points"], z["fit_ori"], z["fit_loss"], z["fit_shell"],
                                    rc.FIT_THR, only=True, dense=True)
    for k in ("filter_unvisible", "filter_unvisible_ori"):
        assert rc.eq(got[k], z["fit_" + k]), k
    vox, vori = rc.voxel_list(occ, ori)
    assert np.array_equal(vox, z["fit_voxels"]) and rc.bits_equal(vori, z["fit_voxel_ori"])
