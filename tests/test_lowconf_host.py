"""The CPU oracle on both sides of the search's low-confidence rule `lt(sum(positive_index), 5)` (PMVO.py:198-206), against the
reference itself: tests/golden/pmvo_lowconf.npz (tools/gen_golden_lowconf.py) holds the reference's forward() and its rank-0
compute_prj_loss on the hand-edited patches of tests/lowconf_cases.py -- points with exactly 0, 1, 4, 5, 6 and 90 positive
samples, 4 and 5 counted from the far end of the sweep, with patch 7, at 4 and 5 samples in all, and with the deciding rank
moved by the base-view ranking.  Every row, bit for bit, NaN == NaN.  CPU only."""
import numpy as np
import pytest

import lowconf_cases as lc
import oracle
import softmask_cases as sc
from conftest import rows_equal


@pytest.fixture(scope="module")
def fx():
    meta, z = lc.load()
    case, rec = lc.case_of(z)          # (regenerates the maps and the points and checks them against the file)
    return meta, z, case, lc.views_of(rec, case["maps"])


def recorded(z, key):
    return tuple(z[key + k] for k in ("fwd_ori", "fwd_loss", "fwd_hc"))


def test_the_fixture_regenerates_and_holds_the_wanted_counts(fx):
    meta, z, case, views = fx
    assert [tuple(c) for c in meta["cases"]] == list(lc.CASES) and [tuple(r) for r in meta["runs"]] == list(lc.RUNS)
    for patch, S in lc.RUNS:
        npos = z["p%ds%d_r0_npos" % (patch, S)]
        mine = lc.case_rows(patch, S)
        assert mine and all(npos[ci] == lc.CASES[ci][3] for ci in mine)
    both = np.concatenate([z["p%ds%d_r0_npos" % r][lc.case_rows(*r)] for r in lc.RUNS])
    assert (both == 4).sum() >= 4 and (both == 5).sum() >= 4
    assert meta["rows_changed_by_lt_4"] > 0 and meta["rows_changed_by_lt_6"] > 0


@pytest.mark.parametrize("run", lc.RUNS)
def test_oracle_forward_equals_the_reference(fx, run):
    meta, z, case, views = fx
    patch, S = run
    key = "p%ds%d_" % run
    for kw in (dict(), dict(base_idx=z[key + "base_idx"], base_val=z[key + "base_val"])):      # the oracle's own ranking, the reference's
        got = oracle.forward(views, case["points"], patch, lc.THR, lc.offsets(S), **kw)[1:]
        assert rows_equal(got, recorded(z, key)).all(), (run, sorted(kw))


@pytest.mark.parametrize("run", lc.RUNS)
def test_oracle_prj_loss_of_rank_0_equals_the_reference(fx, run):
    """(loss, index, flag) of the reference's own compute_prj_loss call; the count of positive samples it compared with 5 equals
    the restatement's on the oracle's tensors; and the fixture tells `< 5` from `< 4` and `< 6`: the restatement with either
    bound leaves the recorded (index, flag) on some row of the run whose count is 4 / 5"""
    meta, z, case, views = fx
    patch, S = run
    key = "p%ds%d_" % run
    o, bidx, bval, D = lc.rank0(views, case["points"], S, patch)
    assert np.array_equal(bidx, z[key + "base_idx"]) and np.array_equal(bval, z[key + "base_val"])
    loss, idx, hc = oracle.prj_loss(D, o["Ori_patch"], o["Conf_patch"], o["visible"], lc.THR)
    assert np.array_equal(loss, z[key + "r0_loss"], equal_nan=True)
    assert np.array_equal(idx, z[key + "r0_idx"]) and np.array_equal(hc, z[key + "r0_hc"])
    args = (D, o["Ori_patch"], o["Conf_patch"], o["visible"], lc.THR)
    st = sc.prj_loss_np(*args)
    assert np.array_equal(st["npos"], z[key + "r0_npos"]) and np.array_equal(st["hc"], hc)
    mine = lc.case_rows(patch, S)
    assert np.array_equal(st["idx"][mine], idx[mine])
    for bound, count in ((4, 4), (6, 5)):
        alt = sc.prj_loss_np(*args, low_below=bound)
        moved = (alt["idx"] != st["idx"]) | (alt["hc"] != st["hc"])
        assert not moved[st["npos"] != count].any()
        tuned = [ci for ci in mine if lc.CASES[ci][3] == count and count < S]       # (all S samples positive: both regimes agree)
        assert moved[tuned].all(), (run, bound)


@pytest.mark.parametrize("name", lc.RANKINGS)
def test_oracle_forward_with_the_recorded_rankings_equals_the_reference(fx, name):
    meta, z, case, views = fx
    idx, val = z["rk_%s_idx" % name], z["rk_%s_val" % name]
    mine = lc.rankings(lc.records(z), case)[name]
    assert np.array_equal(mine[0], idx) and np.array_equal(mine[1], val)
    got = oracle.forward(views, case["points"], 3, lc.THR, lc.offsets(90), base_idx=idx, base_val=val, extra=True)
    assert rows_equal(got[1:4], recorded(z, "rk_%s_" % name)).all()
    a, b = lc.NAMES.index("k4"), lc.NAMES.index("k5")
    if name == "rep":          # equal losses at ranks 0 and 2: the strict `lt` keeps rank 0
        assert (idx[2] == idx[0]).all() and (got[4]["best_rank"] != 1).all()
    else:                      # base_val exactly 0 is not taken, TINY is: the smaller loss, and on one point the other flag
        assert (val[2, [a, b]] == (0 if name == "zero" else np.float32(lc.TINY))).all()
        assert (got[4]["best_rank"][[a, b]] == (0 if name == "zero" else 1)).all()
        zero, tiny = recorded(z, "rk_zero_"), recorded(z, "rk_tiny_")
        assert (tiny[1][[a, b]] < zero[1][[a, b]]).all() and (tiny[2][[a, b]] != zero[2][[a, b]]).any()


def test_oracle_on_the_code_map_pair_equals_the_reference(fx):
    """the 4 / 5 pair on 8-bit code maps (orientation codes 1 degree apart), decoded through the loaders' table"""
    meta, z, case, _ = fx
    assert meta["codes"] is not None, "the generator found no 4 / 5 pair on code maps: this test goes with the c8_* records"
    cc = lc.codes_case_of(z)
    views, pts = lc.views_of(lc.records(z), lc.decode(cc["codes"])), cc["points"]
    assert z["c8_r0_npos"].tolist() == [k for _, k in lc.CODE_CASES]
    for kw in (dict(), dict(base_idx=z["c8_base_idx"], base_val=z["c8_base_val"])):
        assert rows_equal(oracle.forward(views, pts, 3, lc.THR, lc.offsets(90), **kw)[1:], recorded(z, "c8_")).all()
    o, bidx, bval, D = lc.rank0(views, pts, 90, 3)
    loss, idx, hc = oracle.prj_loss(D, o["Ori_patch"], o["Conf_patch"], o["visible"], lc.THR)
    assert np.array_equal(loss, z["c8_r0_loss"]) and np.array_equal(idx, z["c8_r0_idx"]) and np.array_equal(hc, z["c8_r0_hc"])
