"""CPU: the C oracle's border rules against tests/golden/pmvo_border.npz (tools/gen_golden_border.py: the reference's own
results for centres on the image edges, in the corners, one pixel either side of them, on exact rounding ties and for degenerate
projections, over maps that are random per pixel), element for element; the conditions on the case itself (every class of
(view, point) pair occurs, the ties are exact); and the sensitivity of the fixture to wrong border rules, re-run from the file."""
import os

import numpy as np
import pytest

import border_cases as bc
import cascade_cases as cc
import oracle
from conftest import GOLDEN, rows_equal

eq = lambda a, b: np.array_equal(a, b, equal_nan=True)       # noqa: E731


@pytest.fixture(scope="module")
def fx():
    meta, z = bc.load()
    codes, maps, rec, pts = bc.case(z)
    views = oracle.Views(rec, maps["depth"], maps["ori"], maps["conf"], maps["mask"])
    return meta, z, maps, rec, pts, views


def test_every_class_of_pair_occurs_and_the_ties_are_exact(fx):
    meta, z, maps, rec, pts, views = fx
    assert meta["capability"] == "AVX2" and meta["torch"].startswith("2.10.") and meta["threads"] == [1, 8]
    assert len(pts) == meta["N"] and len(pts) % 64 != 0 and len(pts) % 16 != 0
    classes = bc.classify(rec, pts)
    counts = {k: int(v.sum()) for k, v in classes.items()}
    assert counts == meta["class_counts"] and min(counts.values()) > 0, counts
    for k in range(bc.HALF + 1):          # every distance 0..5 from every edge
        for name in ("col_%d", "col_W-1-%d", "row_%d", "row_H-1-%d"):
            assert counts[name % k] > 0
    tags = z["tags"]
    assert {t: int((tags == t).sum()) for t in "abcde"} == dict(a=144, b=24, c=48, d=20, e=60)
    # (c): the oracle's unrounded pixel IS the intended k + 0.5, in both coordinates
    tie = tags == "c"
    pixf = bc.project(rec, pts)[3]
    assert np.array_equal(pixf[bc.HAND][tie].astype(np.float64), z["target"][tie, 1:3])
    want_c = {-0.5, 0.5, 1.5, 2.5, bc.W - 1.5, bc.W - 0.5}
    want_r = {-0.5, 0.5, 1.5, 2.5, bc.H - 1.5, bc.H - 0.5}
    assert want_c <= set(pixf[bc.HAND][tie][:, 1].tolist()) and want_r <= set(pixf[bc.HAND][tie][:, 0].tolist())
    # about half of the pairs whose window is clamped pass the depth test, the rest do not
    wc = classes["window_clamped"]
    share = float((z["visible"][wc] > -1).mean())
    assert 0.25 < share < 0.75, share
    # the regenerated case is the stored one
    cams = bc.cameras()
    p2, t2, g2 = bc.build_points(cams, bc.code_maps(int(z["seed"]))[3], int(z["seed"]))
    assert np.array_equal(g2, tags) and np.allclose(p2, pts, rtol=1e-6, atol=0, equal_nan=True)
    assert np.array_equal(bc.golden_pairs(classes, z["target"], tags), z["pairs"])


def test_float_to_long_rule_the_reference_leans_on(fx):
    """what round(x).long() gave where the fixture was made (x86): NaN, +-inf and |x| >= 2^63 -> INT64_MIN, i.e. negative"""
    meta, z, maps, rec, pts, views = fx
    assert np.array_equal(bc._to_long(np.rint(z["cast_in"])), z["cast_out"])
    bad = ~(np.abs(z["cast_in"]) < np.float32(2.0 ** 63))
    assert bad.sum() == 7 and (z["cast_out"][bad] == bc.I64_MIN).all()


def test_oracle_project_points_equal_the_reference(fx):
    meta, z, maps, rec, pts, views = fx
    rc, zp, oob, _ = bc.project(rec, pts)
    assert np.array_equal(rc, z["uv"]) and eq(zp, z["zp"]) and np.array_equal(oob, z["out_index"])


@pytest.mark.parametrize("patch", bc.PATCHES)
def test_oracle_visible_and_ori_equal_the_reference(fx, patch):
    meta, z, maps, rec, pts, views = fx
    o = oracle.visible_and_ori(views, pts, patch)
    for k in ("visible", "Ori", "Conf", "mask"):
        assert eq(o[k], z[k]), k
    pr = z["pairs"]
    for k in ("Ori_patch", "Conf_patch"):
        assert eq(o[k][pr[:, 0], pr[:, 1]], z["p%d_%s" % (patch, k)]), k
    # ... and, on every pair, the restatement the generator proved equal to the reference's full tensors
    _, zp, _, pixf = bc.project(rec, pts)
    assert not bc.differs(bc.front_end(pixf, zp, maps, patch), o)


def test_oracle_votes_and_refine_loss_equal_the_reference(fx):
    meta, z, maps, rec, pts, views = fx
    patch = meta["vote_patch"]
    for pre, p in (("", pts), ("tiled_", np.tile(pts, (bc.TILE, 1)))):
        surf, filt, unv, _ = oracle.filter_votes(views, p, patch, bc.THR, bc.VIS_THR)
        assert np.array_equal(surf, z[pre + "surface_index"]) and np.array_equal(filt, z[pre + "filter_index"])
        assert np.array_equal(unv, z[pre + "unvisible_index"])
    assert 0 < z["surface_index"].sum() < len(pts) and 0 < z["unvisible_index"].sum() < len(pts)
    rows = z["refine_rows"]
    rl, _ = oracle.refine_loss(views, pts[rows], z["dirs"][rows], patch, bc.THR)
    head = oracle.filter_votes(views, pts[rows], patch, bc.THR, bc.VIS_THR)[3]
    rl[head & ~cc.head_top(pts[rows], cc.toy_head()[1])] = -1
    assert eq(rl, z["refine_loss"]) and (np.isfinite(rl) & (rl != -1)).sum() > 64


@pytest.mark.parametrize("patch", (7, 11))
def test_oracle_forward_equals_the_reference_in_three_batch_compositions(fx, patch):
    """as tests/test_oracle_golden.py holds the other forward fixtures: every row of the original, the reversed and the doubled
    batch; then the batch-independent form through conftest.check_forward_against_reference, as it is"""
    import conftest

    meta, z, maps, rec, pts, views = fx
    offs = np.load(os.path.join(GOLDEN, "depth_offsets.npy"))
    N, pre = len(pts), "f%d_" % patch
    fwd = lambda p, **kw: oracle.forward(views, p, patch, bc.THR, offs, **kw)[1:]     # noqa: E731
    got = fwd(pts, base_idx=z[pre + "base_idx"], base_val=z[pre + "base_val"])
    assert rows_equal(got, tuple(z[pre + k] for k in ("fwd_ori", "fwd_loss", "fwd_hc"))).all()
    got = tuple(a[::-1] for a in fwd(pts[::-1].copy()))
    assert rows_equal(got, tuple(z[pre + "rev_" + k] for k in ("ori", "loss", "hc"))).all()
    got = tuple(a[:N] for a in fwd(np.concatenate([pts, pts], 0)))
    assert rows_equal(got, tuple(z[pre + "dup_" + k] for k in ("ori", "loss", "hc"))).all()
    assert np.isfinite(z[pre + "fwd_loss"]).sum() > 200
    # the library's own ranking gives the recorded values (indices of equal values are not compared)
    vo = oracle.visible_and_ori(views, pts, patch)
    assert np.array_equal(oracle.topk_views(vo["visible"], vo["Conf"])[1], z[pre + "base_val"])
    name = "pmvo_border_p%d" % patch
    conftest.recompose_golden("pmvo_small", "dup")          # (loads the shared table)
    conftest._recompose.update({"%s__%s_%s" % (name, t, k): z[pre + "%s_%s" % (t, k)] for t in ("dup", "rev")
                                for k in ("ori", "loss", "hc")})
    prev = oracle.set_reproject_rule("mid"), oracle.set_sum_block(0)
    try:
        _, ori, loss, hc = oracle.forward(views, pts, patch, bc.THR, offs, base_idx=z[pre + "base_idx"],
                                          base_val=z[pre + "base_val"])
    finally:
        oracle.set_reproject_rule(*prev[0])
        oracle.set_sum_block(prev[1])
    conftest.check_forward_against_reference(name, {k: z[pre + k] for k in ("fwd_ori", "fwd_loss", "fwd_hc")}, ori, loss, hc)


def test_the_fixture_tells_wrong_border_rules_from_the_right_one(fx):
    """the generator's sensitivity check from the file: the restatement equals the recorded results, every wrong rule changes
    one at every patch size it can affect (on the stored pairs, for the patch tensors)"""
    meta, z, maps, rec, pts, views = fx
    _, zp, _, pixf = bc.project(rec, pts)
    pr = z["pairs"]

    def cut(d):
        out = {k: d[k] for k in ("visible", "Ori", "Conf", "mask")}
        out.update({k: d[k][pr[:, 0], pr[:, 1]] for k in ("Ori_patch", "Conf_patch")})
        return out

    for patch in bc.PATCHES:
        ref = {k: z[k] for k in ("visible", "Ori", "Conf", "mask")}
        ref.update({k: z["p%d_%s" % (patch, k)] for k in ("Ori_patch", "Conf_patch")})
        assert not bc.differs(cut(bc.front_end(pixf, zp, maps, patch)), ref)
        for rule in bc.WRONG_RULES:
            if bc.side(patch) == 1 and rule in bc.RULE_NEEDS_WINDOW:
                continue
            assert bc.differs(cut(bc.front_end(pixf, zp, maps, patch, rule)), ref), (patch, rule)
            assert meta["wrong_rules"][rule][patch]
