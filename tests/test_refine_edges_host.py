"""CPU: refine()'s decisions with the compared value ON its bound (tests/refine_edge_cases.py, tests/golden/refine_edges.npz,
tools/gen_golden_refine_edges.py) -- the oracle and the numpy restatements against the reference's own record, and
oracle.replace_dissimilar against the installed torch.cosine_similarity on a sweep across the 0.95 bound.  Everything is compared
for plain equality (NaN == NaN); the sign of a zero where the reference's `* -1` decides it."""
import os
import warnings

import numpy as np
import pytest
import torch
from scipy.spatial import KDTree

import oracle
import refine_edge_cases as rc
from conftest import GOLDEN, golden_records, golden_scene, scene_views

F = np.float32


@pytest.fixture(scope="module")
def fx():
    meta, z = rc.load()
    views = scene_views(golden_scene(meta), golden_records(np.load(os.path.join(GOLDEN, "e2e_multichunk.npz"))))
    return meta, z, views


def test_the_fixture_holds_rows_on_every_bound(fx):
    meta, z, _ = fx
    assert meta["numpy"].startswith("2.") and meta["height_rule"] == "float64"
    assert z["loop_points"].shape == (rc.N_SURFACE, 3) and z["loop_shell"].shape == (rc.N_SHELL, 3)
    sim = z["loop_similar"][z["loop_rows_cos"]]
    assert [(sim == v).sum() for v in (rc.COS, rc.COS_LO, rc.COS_HI)] == [3, 3, 3]
    assert list(z["loop_dist"][z["loop_rows_dist"]]) == [rc.DIST, rc.DIST_LO, rc.DIST_HI]
    La, Lb = z["loop_L"]
    zs = z["loop_points"][z["loop_rows_height"], 2]
    assert float(F(La)) != La and F(La) < La and float(F(Lb)) == Lb                 # scalp "a": L is no float32; "b": it is
    assert zs[0] == F(La) == F(Lb) and zs[1] == np.nextafter(zs[0], F(-9)) and zs[2] == np.nextafter(zs[0], F(9))
    for s, L in (("a", La), ("b", Lb)):
        assert np.max(z["loop_scalp_" + s], axis=0)[2] - 0.01 == L
    t = z["loop_thresholds"]
    ml = z["loop_ref_min_loss"]
    assert t[0] == 0.5 and (ml == 0.5).sum() > 50 and (ml == F(t[1])).sum() == 1 and F(t[2]) == np.nextafter(F(t[1]), F(9))
    loss = z["fit_loss"]
    thr = F(rc.FIT_THR)
    for v in (thr, np.nextafter(thr, F(0)), np.nextafter(thr, F(1)), F(-1), F(0.5)):
        assert (loss == v).sum() >= 1
    assert np.isnan(loss).sum() == 1 and (np.signbit(loss) & (loss == 0)).sum() == 1
    y = z["fit_ori"][:, 1]
    assert ((y == 0) & np.signbit(y)).sum() >= 1 and (y == F(1e-45)).sum() == 1 and (y == F(-1e-45)).sum() == 1
    assert (np.abs(z["fit_points"]) == F(1e7)).sum() == 6 and (z["fit_int32_of_4e9"] == rc.INT_MIN).all()
    for name in ("f32", "f64"):
        p = z["p2v_%s_points" % name]
        assert rc.on_a_half(p, rc.BIN_MIN, rc.BIN_SIZE).sum() > 30 and rc.outside_int32(p, rc.BIN_MIN, rc.BIN_SIZE).sum() >= 15
        assert rc.eq(p, rc.p2v_points(p.dtype))


def test_oracle_smoothing_loop_on_the_bounds(fx):
    """oracle.refine_loop on case loop with both scalps, then the shell stage at the three thresholds: the five files"""
    meta, z, views = fx
    pts, shell = z["loop_points"], z["loop_shell"]
    for s, want in (("a", z["loop_ref_min_loss"]), ("b", z["loop_b_min_loss"])):
        scalp = z["loop_scalp_" + s]
        ori, loss = z["loop_ori"].copy(), z["loop_loss"].copy()
        oracle.refine_loop(views, pts, ori, loss, meta["patch"], meta["thr"], meta["vis_thr"], KDTree(data=scalp), np.max(scalp, axis=0))
        assert rc.eq(ori, z["loop_ref_select_o"]) and rc.eq(loss, want), s
        runs = [("loop_t%d_" % i, t) for i, t in enumerate(z["loop_thresholds"])] if s == "a" else [("loop_b_", 0.5)]
        for key, t in runs:
            keep = np.where(loss < t)[0]
            kp, ko = oracle.shell_orientations(views, pts[keep], ori[keep], shell, meta["patch"], meta["thr"], meta["vis_thr"],
                                               KDTree(data=scalp), np.max(scalp, axis=0))
            assert rc.eq(kp, z[key + "filter_unvisible"]) and rc.eq(ko, z[key + "filter_unvisible_ori"]), (s, t)
    assert rc.eq(pts, z["loop_ref_select_p"])


def test_oracle_replacement_and_scalp_test_on_the_bounds(fx):
    _, z, _ = fx
    ori = z["loop_ori"].copy()
    n = oracle.replace_dissimilar(z["loop_center"], ori, 0.95)
    assert rc.eq(ori, z["loop_ref_select_o"]) and n == int((z["loop_similar"] < rc.COS).sum())
    assert rc.eq(rc.max_cos(z["loop_center"], z["loop_ori"]), z["loop_similar"])
    pts, votes = z["loop_points"], z["loop_votes"]
    for s, ml in (("a", z["loop_ref_min_loss"]), ("b", z["loop_b_min_loss"])):
        scalp = z["loop_scalp_" + s]
        top = oracle.head_top_mask(pts, KDTree(data=scalp), np.max(scalp, axis=0))
        assert np.array_equal(votes & ~top, ml == 0.5), s


def test_restatements_reproduce_the_record_and_the_opposite_forms_do_not(fx):
    _, z, _ = fx
    sim, cen, ori, ref_o = z["loop_similar"], z["loop_center"], z["loop_ori"], z["loop_ref_select_o"]
    assert rc.eq(rc.replace_rule(sim, cen, ori), ref_o)
    d = np.flatnonzero((rc.replace_rule(sim, cen, ori, "le") != ref_o).any(1))
    assert len(d) == 3 and (sim[d] == rc.COS).all()
    dist, zz, votes = z["loop_dist"], z["loop_points"][:, 2], z["loop_votes"]
    La, Lb = z["loop_L"]
    for L, ml, other in ((La, z["loop_ref_min_loss"], "f32_lt"), (Lb, z["loop_b_min_loss"], "f64_le")):
        assert np.array_equal(votes & ~rc.head_top_rule(dist, zz, L), ml == 0.5)
        d = np.flatnonzero(rc.head_top_rule(dist, zz, L, dist_op="le") != rc.head_top_rule(dist, zz, L))
        assert len(d) >= 1 and (dist[d] == rc.DIST).all()
        d = np.flatnonzero(rc.head_top_rule(dist, zz, L, z_form=other) != rc.head_top_rule(dist, zz, L))
        assert len(d) >= 1 and (zz[d] == F(L)).all()
    assert np.array_equal(rc.head_top_rule(dist, zz, La, z_form="f64_le"), rc.head_top_rule(dist, zz, La))


def test_oracle_and_host_p2v_on_halves_and_outside_int32(fx):
    from monohair_amd import pmvo_utils as U

    _, z, _ = fx
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")               # (the cast of NaN / 4e9 to int32 warns)
        for name in ("f32", "f64"):
            pts, want = z["p2v_%s_points" % name], z["p2v_%s_index" % name]
            for fn in (oracle.p2v, U.p2v):
                got = np.stack(fn(pts.copy(), rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID), 1)
                assert np.array_equal(got, want), (name, fn.__module__)
            assert np.array_equal(rc.p2v_rule(pts, rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID), want)
            half, big = rc.on_a_half(pts, rc.BIN_MIN, rc.BIN_SIZE), rc.outside_int32(pts, rc.BIN_MIN, rc.BIN_SIZE)
            d = rc.p2v_rule(pts, rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID, rounding="floor") != want
            e = rc.p2v_rule(pts, rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID, clip_first=True) != want
            assert d.any() and half[d].all() and e.any() and big[e].all()
            # the fit on these points with the hand-written orientations (what the GPU test holds the kernels to): the
            # restatement and the oracle agree
            ori = np.resize(z["fit_ori"][110:], (len(pts), 3)).astype(F)
            vox, med, _ = rc.fit_rule(pts, ori, len(pts), rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID)
            v2, m2 = rc.voxel_list(*oracle.voxel_fit(pts.copy(), ori.copy(), rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID))
            assert np.array_equal(vox, v2) and rc.bits_equal(med, m2), name


def fit_inputs(z):
    kept = rc.keep_rule(z["fit_loss"], rc.FIT_THR)
    return (np.concatenate([z["fit_points"][kept], z["fit_filter_unvisible"]]),
            np.concatenate([z["fit_ori"][kept], z["fit_filter_unvisible_ori"]]), len(kept))


def test_oracle_shell_stage_and_voxel_fit_on_the_hand_written_files(fx):
    meta, z, views = fx
    scalp = z["loop_scalp_a"]
    keep = np.where(z["fit_loss"] < rc.FIT_THR)[0]
    assert np.array_equal(keep, rc.keep_rule(z["fit_loss"], rc.FIT_THR)) and len(keep) >= 100
    kp, ko = oracle.shell_orientations(views, z["fit_points"][keep], z["fit_ori"][keep], z["fit_shell"], meta["patch"], meta["thr"],
                                       meta["vis_thr"], KDTree(data=scalp), np.max(scalp, axis=0))
    assert rc.eq(kp, z["fit_filter_unvisible"]) and rc.eq(ko, z["fit_filter_unvisible_ori"])
    p, o, n_surface = fit_inputs(z)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        occ, ori = oracle.voxel_fit(p.copy(), o.copy(), rc.VOXEL_MIN, rc.VOXEL_SIZE, rc.GRID)
    vox, vori = rc.voxel_list(occ, ori)
    assert np.array_equal(vox, z["fit_voxels"]) and rc.bits_equal(vori, z["fit_voxel_ori"])
    v, m, scores = rc.fit_rule(p, o, n_surface)
    assert np.array_equal(v, z["fit_voxels"]) and rc.bits_equal(m, z["fit_voxel_ori"])
    assert any(len(s) == 1 for s in scores) and sum(len(s) == 2 and s[0] == s[1] for s in scores) >= 3
    for kw in (dict(flip="ge"), dict(clip_first=True), dict(tie="last"), dict(shell_first=True)):
        v2, m2, _ = rc.fit_rule(p, o, n_surface, **kw)
        assert not (np.array_equal(v2, v) and rc.bits_equal(m2, m)), kw
    kept_le = rc.keep_rule(z["fit_loss"], rc.FIT_THR, "le")
    assert len(kept_le) == n_surface + 1


def test_oracle_replacement_rule_across_the_bound_and_on_degenerate_rows():
    """oracle.replace_dissimilar == torch.cosine_similarity + torch.lt of the installed torch on 20 000 pairs rotated by
    acos(0.95) +- 2e-7 and on zero, denormal, tiny, overflowing, infinite and NaN rows in either operand"""
    c, o = rc.cos_sweep()
    sim = rc.max_cos(c, o)
    with np.errstate(invalid="ignore"):
        for v in (rc.COS, rc.COS_LO, rc.COS_HI):
            assert (sim[:20000] == v).sum() > 100
        assert np.isnan(sim[20000:]).sum() > 50 and (sim[20000:] < rc.COS).sum() > 50 and (sim[20000:] >= rc.COS).sum() > 20
        want = rc.replace_rule(sim, c, o)
        t = torch.lt(torch.from_numpy(sim), 0.95).numpy()
        assert np.array_equal(t, sim < rc.COS)
    got = o.copy()
    n = oracle.replace_dissimilar(c, got, 0.95)
    assert rc.bits_equal(got, want) and n == int(t.sum())
