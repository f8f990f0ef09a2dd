"""CPU: the C oracle on soft hair masks and on compared quantities that equal their thresholds, against
tests/golden/pmvo_softmask.npz (tools/gen_golden_softmask.py: the reference's own results on the cases of tests/softmask_cases.py)
-- every row of every batch composition, plain equality; the conditions on the cases themselves (every tie family occurs, the
depth gaps ARE 0.1f / 0.9f / 1.0 and their neighbours); and the sensitivity of the fixture to another summation order and to the
opposite operator of each rule, recomputed from the file."""
import os

import numpy as np
import pytest

import cascade_cases as cc
import oracle
import softmask_cases as sc
from conftest import GOLDEN

eq = lambda a, b: np.array_equal(a, b, equal_nan=True)       # noqa: E731
INDISTINGUISHABLE = ["positive_4", "positive_5"]      # families the generator searched for and did not find (docs/PARITY.md lists them)


@pytest.fixture(scope="module")
def fx():
    meta, z = sc.load()
    cases = {}
    for V in sc.VIEW_COUNTS:
        case, maps, rec = sc.case_of(z, V)
        views = {p: oracle.Views(rec, *[maps[p][k] for k in ("depth", "ori", "conf", "mask")]) for p in sc.PALETTES}
        cases[V] = (case, maps, rec, views)
    return meta, z, cases


def combos():
    return [(thr, patch) for thr in sc.THRS for patch in sc.PATCHES]


def test_every_tie_family_occurs_and_the_gaps_are_exact(fx):
    meta, z, cases = fx
    assert meta["capability"] == "AVX2" and meta["torch"].startswith("2.10.") and meta["threads"] == [1, 8]
    for V, (case, maps, rec, views) in cases.items():
        N = len(case["points"])
        assert N == meta["cases"][V]["N"] and N % 32 != 0 and N * sc.TILE >= 4096 and (N * sc.TILE) % 32 != 0
        assert np.array_equal(case["tags"], z["v%d_tags" % V]) and np.array_equal(case["info"], z["v%d_info" % V])
        assert set(np.unique(case["m8"]).tolist()) == set(sc.CODES.tolist())
        hands = np.flatnonzero(np.arange(V) % sc.NCAM == sc.HAND)
        for pal in sc.PALETTES:
            info = meta["cases"][V]["palettes"][pal]
            vis = oracle.visible_and_ori(views[pal], case["points"], 1)["visible"]
            t3 = sc.pair_terms(rec, case["points"], case, maps[pal], 3)
            gaps = sc.gap_families(t3, case["tags"], case["info"], hands)
            assert gaps == info["gap_families"] and len(gaps) == len(sc.G_FAMILIES) and min(gaps.values()) == 3, gaps
            for thr, patch in combos():
                t = sc.pair_terms(rec, case["points"], case, maps[pal], patch)
                rec_c = info["combos"]["t%dp%d" % (sc.thr_code(thr), patch)]
                fam = sc.families(t, vis, thr)
                assert fam == rec_c["families"], (V, pal, thr, patch)
                assert min(fam.values()) > 0 or patch != 3, fam
                assert sc.sensitivity(t, thr, N) == rec_c["sensitivity"], (V, pal, thr, patch)
        values = np.unique(maps["planes"]["mask"])
        assert np.array_equal(values, np.sort(sc.PLANE_PALETTE))
        assert np.float32(51 / 255.0) == np.float32(0.2) and z["lut"][51, 3] == np.float32(0.2) and z["lut"][49, 3] == 0
    # what the fixture can tell from the right rule, over all its cases -- and what it cannot (docs/PARITY.md)
    found = meta["sensitive_rows"]
    for need in ("order_main_surface", "order_main_filter", "order_main_head", "order_tail_surface", "order_tail_filter",
                 "order_tail_head", "op_gap01", "op_gap_vis", "op_gap09", "op_gap_head", "op_cmax", "op_mask", "op_search_cmax",
                 "op_search_tap", "op_search_weight", "weight_on_thr"):
        assert found[need] > 0, need
    assert meta["indistinguishable"] == INDISTINGUISHABLE
    for V in sc.VIEW_COUNTS:
        for srep in meta["cases"][V]["search"].values():
            assert srep["rows"] == meta["cases"][V]["N"] and srep["agree"] >= 0.95 * srep["rows"]


def test_recorded_flags_of_the_points_whose_weight_is_the_threshold(fx):
    """class w: one view sees the point and every tap of its 3 x 3 patch is the code T, so sum(weight) / sum(weight > 0) is
    float32(T / 255) for every sample.  The reference's flag is `> conf_threshold` (PMVO.py:198): False where T / 255 IS the
    threshold (it would be True under `>=`) and below it, True above it."""
    meta, z, cases = fx
    seen = 0
    for V, (case, maps, rec, views) in cases.items():
        w = np.flatnonzero(case["tags"] == "w")
        assert len(w) == sc.N_W
        for pal in sc.PALETTES:
            for thr in sc.THRS:
                hc = z["v%d_%s_t%dp3_fwd_hc_batch" % (V, pal, sc.thr_code(thr))]
                loss = z["v%d_%s_t%dp3_fwd_loss_batch" % (V, pal, sc.thr_code(thr))]
                T = case["info"][w, 0]
                assert np.isfinite(loss[w]).all()
                assert np.array_equal(hc[w], T > sc.thr_code(thr)), (V, pal, thr)
                seen += int((T == sc.thr_code(thr)).sum())
    assert seen > 0


@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("pal", sc.PALETTES)
def test_oracle_votes_equal_the_reference_in_every_composition(fx, V, pal):
    meta, z, cases = fx
    case, maps, rec, views = cases[V]
    scalp = cc.toy_head()[1]
    pp = "v%d_%s_" % (V, pal)
    changed = 0
    for name, p in sc.compositions(case).items():
        for thr, patch in combos():
            key = pp + "t%dp%d_" % (sc.thr_code(thr), patch)
            got = oracle.filter_votes(views[pal], p, patch, thr, sc.VIS_THR)
            for k, a in zip(("surface", "filter", "unvisible"), got):
                assert np.array_equal(a, z[key + k + "_" + name]), (name, thr, patch, k)
        for vt in meta["head_vis"]:
            head = oracle.filter_votes(views[pal], p, 3, sc.THRS[0], vt)[3] & ~cc.head_top(p, scalp)
            assert np.array_equal(head, z[pp + "head%g_%s" % (vt, name)]), (name, vt)
            changed += int(head.sum())
    assert changed > 0
    b = z[pp + "t102p3_surface_batch"]
    assert 0 < b.sum() < len(b) and 0 < z[pp + "t102p3_filter_batch"].sum()


@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("pal", sc.PALETTES)
def test_oracle_refine_loss_and_front_end_equal_the_reference(fx, V, pal):
    meta, z, cases = fx
    case, maps, rec, views = cases[V]
    scalp = cc.toy_head()[1]
    pp = "v%d_%s_" % (V, pal)
    dirs = z["v%d_dirs" % V]
    o = oracle.visible_and_ori(views[pal], case["points"], 1)
    for k in ("visible", "Conf", "mask"):
        assert eq(o[k][-meta["kept_views"]:], z[pp + k]), k
    for name, p in sc.compositions(case).items():
        if name == "tiled":
            continue
        dr = dirs if name == "batch" else dirs[case["singles"][int(name[3:])]][None]
        head = oracle.filter_votes(views[pal], p, 3, sc.THRS[0], sc.VIS_THR)[3] & ~cc.head_top(p, scalp)
        for thr, patch in combos():
            rl, _ = oracle.refine_loss(views[pal], p, dr, patch, thr)
            rl[head] = -1
            assert eq(rl, z[pp + "t%dp%d_refine_%s" % (sc.thr_code(thr), patch, name)]), (name, thr, patch)
    want = z[pp + "t102p3_refine_batch"]
    assert (want == -1).sum() > 0 and (np.isfinite(want) & (want != -1)).sum() > 32


@pytest.mark.parametrize("V", sc.VIEW_COUNTS)
@pytest.mark.parametrize("pal", sc.PALETTES)
@pytest.mark.parametrize("thr", sc.THRS)
def test_oracle_forward_equals_the_reference(fx, V, pal, thr):
    meta, z, cases = fx
    case, maps, rec, views = cases[V]
    offs = np.load(os.path.join(GOLDEN, "depth_offsets.npy"))
    ran_tiled = False
    for patch in sc.PATCHES:
        key = "v%d_%s_t%dp%d_" % (V, pal, sc.thr_code(thr), patch)
        for name, p in sc.compositions(case).items():
            if key + "fwd_loss_" + name not in z.files:
                assert name == "tiled" and (V, thr, patch) != tuple(meta["tiled_forward"])
                continue
            ran_tiled |= name == "tiled"
            _, ori, loss, hc = oracle.forward(views[pal], p, patch, thr, offs, base_idx=z[key + "base_idx_" + name],
                                              base_val=z[key + "base_val_" + name])
            assert eq(loss, z[key + "fwd_loss_" + name]) and eq(ori, z[key + "fwd_ori_" + name]), (patch, name)
            assert np.array_equal(hc, z[key + "fwd_hc_" + name]), (patch, name)
        hc = z[key + "fwd_hc_batch"]
        assert 0 < hc.sum() < len(hc) and np.isfinite(z[key + "fwd_loss_batch"]).sum() > 200
    assert ran_tiled == ((V, thr) == tuple(meta["tiled_forward"][:2]))
