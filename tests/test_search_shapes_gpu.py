"""GPU: the fused search (mh_forward, mh_search_prepared, mh_search_forward; csrc/pmvo_search.hip) at sample counts and rank
sets other than the reference's 90 x (0, 2, ..., 18).  The C ABI takes any S <= 256 and any nrank <= 16 ranks with
(nrank - 1) * rank_step < 20 and nrank * S <= 1024 items; what the shipped kernel does with a point's nact = nvalid * S items --
slices of 64 per wave (`ka`), the L = nact % 64 leftover items of the last wave, the division by S in registers, the per-rank
epilogue over S in rounds of 64 lanes, the trailing N * S % 32 columns of the batch -- is arithmetic on S.  Every output of
forward() (line_ori, min_loss, high_conf, best_s, best_rank) is compared bit for bit, NaN == NaN, with oracle.forward, for
the shipped kernel by the maps, with the key body and with the select body, and for the portable kernel (search_variant 1256).

The scenes are the hand-written ones of tests/test_search_staging_gpu.py: 22 views of 32 x 64 (70 for the second 64-view
block), patch 7, every list complete (49 taps); k views see a point, the others have its pixel hidden.  A rank is usable while
its value is > 0, so k views give nvalid = min(nrank, ceil(k / rank_step)) ranks.  Each test states the case it means to
reach as literals -- nvalid, nact, L, whether the last wave takes the leftover items (0 < L <= 16 and L * V <= 544) and the
slices of the four waves -- checks them against plan(), a restatement of the kernel's prologue, and checks k and nvalid
against what the context reports (search_work).  Each case runs as one batch, then its first three points, then points alone
(a point alone is the batch's last point: its last S % 32 samples are trailing columns)."""
import numpy as np
import pytest
import torch

import oracle
from test_search_leftover_gpu import show_only, spread
from test_search_staging_gpu import DEV, THR, Scene, run

gpu = pytest.mark.gpu
ALL = ((0, 0), (1, 0), (2, 0), (0, 1256))
CODES = ((0, 0), (2, 0), (0, 1256))
REF_RANKS = range(0, 20, 2)


def plan(S, ranks, k, V=22):
    """(nvalid, nact, L, the last wave takes the L items, slices of waves 0 .. 3) of a point that k views see: the prologue of
    mh_search3_kernel (256 lanes; slice j of wave w holds the items from j * 256 + w * 64)"""
    step = ranks[1] - ranks[0] if len(ranks) > 1 else 1
    nvalid = max(1, min(len(ranks), -(-k // step)))
    nact = nvalid * S
    L = nact % 64
    left = 0 < L <= 16 and L * V <= 544
    body = nact - (L if left else 0)
    return nvalid, nact, L, left, tuple(sum(1 for j in range(4) if j * 256 + w * 64 < body) for w in range(4))


def check_case(S, ranks, vis, stated, codes=False, alone=(0, 1), V=22, seed=1, min_dist=2, shown=None):
    """One table row: the scene of len(vis) points, point n seen by vis[n] views (`shown`: the views, else spread()); the
    stated plan; the batch, its first three points, the points `alone`.  Returns the info dict of the whole batch.  (The
    plan's leftover lanes are the key kernels'; the select body and contexts of 8-bit codes keep the slice whatever L is.)"""
    ranks = list(ranks)
    assert [plan(S, ranks, k, V) for k in vis] == list(stated)
    sc = Scene(V, 32, 64, 7, len(vis), min_dist=min_dist, codes=codes, seed=seed)
    for n, k in enumerate(vis):
        views = shown[n] if shown else spread(V, n, k)
        assert len(views) == k
        show_only(sc, n, views)
    runs = CODES if codes else ALL
    info = {}
    cnt, loss = run(sc, None, runs=runs, ranks=ranks, num_sample=S, info=info)
    assert cnt.shape == (V, len(vis)) and [(cnt[:, n] > 0).sum() for n in range(len(vis))] == list(vis)
    assert (cnt[cnt > 0] == 49).all() and np.isfinite(loss).all()
    assert list(info["nvalid"]) == [p[0] for p in stated]
    run(sc, None, runs=runs, ranks=ranks, num_sample=S, pts=sc.pts[:3])
    for n in alone:
        run(sc, None, runs=runs, ranks=ranks, num_sample=S, pts=sc.pts[n:n + 1])
    return info


def test_division_by_the_sample_count_in_registers():
    """(it * ((1 << 20) / S + 1)) >> 20 == it / S for every item of every sample count the search takes (mh_search_slices_lds,
    mh_left_batch), in 32-bit unsigned arithmetic"""
    for S in range(1, 257):
        inv = (1 << 20) // S + 1
        it = np.arange(1024, dtype=np.uint32)
        assert int(it[-1]) * inv < 1 << 32
        assert np.array_equal((it * np.uint32(inv)) >> np.uint32(20), it // np.uint32(S)), S


@gpu
@pytest.mark.parametrize("npts", [5, 40])
def test_one_sample_every_item_a_leftover(npts):
    """S = 1: 10, 4 and 1 items, all of them leftover items -- no wave has a slice; fewer than five samples, so the
    low-confidence rule (npos < 5) always holds.  Five points: 5 columns, every one trailing; 40 points: columns 32 .. 39
    (40 points of distinct pixels in every view: hiding touches the point's own pixel only).  A point alone is a batch of ONE
    candidate, N * S = 1: the reference projects the sample through the single-column sgemm and adds the views as a
    contiguous sum (mh_search_one_column_kernel; before it existed min_loss of point 0 alone was 0.05470384, the oracle's and
    -- tests/golden/pmvo_samples.npz holds its forward() at S = 1 on points handed to it alone, tests/test_sample_counts_*.py --
    the reference's 0.05470383).  mh_launch_search sends that shape to the one kernel whatever the plan is, so for a point alone
    search_variant 1256 is no second implementation here: the oracle is the only independent reference."""
    vis = ((22, 7, 1) * 14)[:npts]
    stated = (((10, 10, 10, True, (0, 0, 0, 0)), (4, 4, 4, True, (0, 0, 0, 0)), (1, 1, 1, True, (0, 0, 0, 0))) * 14)[:npts]
    assert (npts * 1) % 32 == (5 if npts == 5 else 8)
    info = check_case(1, REF_RANKS, vis, stated, alone=(0, 2), min_dist=2 if npts == 5 else 1)
    assert (info["best_s"] == 0).all() and len(set(info["best_rank"])) > 2


@gpu
@pytest.mark.parametrize("rule,block", [(0, 32), (0, 0), (1, 32), (1, 0)])
def test_one_candidate_in_all_under_the_batch_options(rule, block):
    """N = 1, S = 1 with reproject_rule 0 / 1 (the sample's projection follows the batch or not) and sum_block 32 / 0 (the
    views are added as ATen adds a [V, 1] tensor, or in cascade order): 22, 7 and 1 views, each point alone.  (Variants 0 and
    1256 run the same kernel at this shape unless both options are off: the oracle is the independent reference.)"""
    sc = Scene(22, 32, 64, 7, 3, min_dist=2, seed=1)
    for n, k in enumerate((22, 7, 1)):
        show_only(sc, n, spread(22, n, k))
    pm = sc.context()
    pm.set_num_sample(1)
    pm.set_option("reproject_rule", rule)
    pm.set_option("sum_block", block)
    prev = oracle.set_reproject_rule("mid" if rule else "group"), oracle.set_sum_block(block)
    try:
        from monohair_amd.pmvo import depth_offsets

        for n in range(3):
            p = sc.pts[n:n + 1]
            _, o_ori, o_loss, o_hc, o_ex = oracle.forward(sc.views(), p, 7, THR, depth_offsets(1), extra=True)
            for variant in (0, 1256):
                pm.set_option("search_variant", variant)
                _, ori, loss, hc, ex = pm.forward(p, extras=True)
                got = tuple(x.cpu().numpy() for x in (ori, loss, hc, ex["best_s"], ex["best_rank"], ex["best_sample"]))
                for a, b in zip(got, (o_ori, o_loss, o_hc, o_ex["best_s"], o_ex["best_rank"], o_ex["best_sample"])):
                    assert a.shape == b.shape and np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), (n, variant)
            assert np.isfinite(o_loss).all()
    finally:
        oracle.set_reproject_rule(*prev[0])
        oracle.set_sum_block(prev[1])


@gpu
def test_16_samples_waves_without_a_slice_next_to_waves_with_one():
    """S = 16: 16 items (all leftover), 64 (one slice, wave 0 alone, no leftover), 80 (a slice and 16 leftover items), 160 (L = 32:
    a slice).  Five points: 80 columns, point 4 is made of trailing columns; three points: point 2; a point alone: all 16."""
    stated = ((1, 16, 16, True, (0, 0, 0, 0)), (4, 64, 0, False, (1, 0, 0, 0)), (5, 80, 16, True, (1, 0, 0, 0)),
              (10, 160, 32, False, (1, 1, 1, 0)), (1, 16, 16, True, (0, 0, 0, 0)))
    assert (5 * 16) % 32 == 16 and (3 * 16) % 32 == 16
    check_case(16, REF_RANKS, (2, 8, 10, 22, 2), stated, alone=(2, 3))


@gpu
@pytest.mark.parametrize("codes", [False, True])
def test_65_samples_every_leftover_count_1_to_10(codes):
    """S = 65 = one lane round and one sample: nvalid ranks leave L = nvalid items, 1 .. 10"""
    stated = ((1, 65, 1, True, (1, 0, 0, 0)), (2, 130, 2, True, (1, 1, 0, 0)), (3, 195, 3, True, (1, 1, 1, 0)),
              (4, 260, 4, True, (1, 1, 1, 1)), (5, 325, 5, True, (2, 1, 1, 1)), (6, 390, 6, True, (2, 2, 1, 1)),
              (7, 455, 7, True, (2, 2, 2, 1)), (8, 520, 8, True, (2, 2, 2, 2)), (9, 585, 9, True, (3, 2, 2, 2)),
              (10, 650, 10, True, (3, 3, 2, 2)))
    info = check_case(65, REF_RANKS, tuple(range(2, 21, 2)), stated, codes=codes, alone=(4, 9))
    assert (info["best_s"] == 64).any()       # a winner in the second lane round of the epilogue


@gpu
def test_16_ranks_of_64_samples_exactly_1024_items():
    """nrank = 16, rank_step = 1, S = 64: 1024 items = MH_MAX_ITEMS, the last wave has four slices too; 15 views: 960, it has three"""
    stated = ((16, 1024, 0, False, (4, 4, 4, 4)), (15, 960, 0, False, (4, 4, 4, 3)), (16, 1024, 0, False, (4, 4, 4, 4)))
    info = check_case(64, range(16), (22, 15, 22), stated)
    assert (info["best_rank"] > 0).any()


@gpu
@pytest.mark.parametrize("codes", [False, True])
def test_100_samples_the_largest_count_of_ten_ranks(codes):
    """S = 100: 1000 items (L = 40: a fourth slice in every wave), 900 (L = 4), 400 (L = 16), 200 (L = 8), 100 (L = 36); three
    points: 300 columns, the last 12 samples of point 2 are trailing columns"""
    stated = ((10, 1000, 40, False, (4, 4, 4, 4)), (9, 900, 4, True, (4, 4, 3, 3)), (4, 400, 16, True, (2, 2, 1, 1)),
              (2, 200, 8, True, (1, 1, 1, 0)), (1, 100, 36, False, (1, 1, 0, 0)))
    assert (3 * 100) % 32 == 12
    info = check_case(100, REF_RANKS, (22, 18, 8, 4, 2), stated, codes=codes, alone=(1, 2))
    assert (info["best_s"] >= 64).any()


@gpu
def test_256_samples_four_lane_rounds():
    """nrank = 4, rank_step = 5, S = 256: 1024, 512 and 256 items, no leftover and (256 = 8 x 32) no trailing column.  The
    epilogue's argmin runs over four rounds of 64 lanes: with seed 1 of the point choice the oracle's winners are samples 255,
    0, 255, 45, 250 and 59 (seeds were to be tried on the CPU against oracle.forward until one had a winner >= 192 and one
    < 64; the first did)."""
    stated = ((4, 1024, 0, False, (4, 4, 4, 4)), (2, 512, 0, False, (2, 2, 2, 2)), (1, 256, 0, False, (1, 1, 1, 1))) + \
        ((4, 1024, 0, False, (4, 4, 4, 4)),) * 3
    assert (6 * 256) % 32 == 0 and 256 % 32 == 0
    info = check_case(256, range(0, 20, 5), (22, 6, 5, 22, 22, 22), stated, alone=(0, 5))
    assert (info["best_s"] >= 192).any() and (info["best_s"] < 64).any()
    assert list(info["best_s"]) == [255, 0, 255, 45, 250, 59]


@gpu
def test_255_samples_leftovers_of_60_to_63_stay_slices():
    """nrank = 4, rank_step = 1, S = 255 (odd): L = 60, 61, 62, 63; four points: 1020 columns, the trailing 28 lie inside point 3"""
    stated = ((4, 1020, 60, False, (4, 4, 4, 4)), (3, 765, 61, False, (3, 3, 3, 3)), (2, 510, 62, False, (2, 2, 2, 2)),
              (1, 255, 63, False, (1, 1, 1, 1)))
    assert (4 * 255) % 32 == 28 and (3 * 255) % 32 == 29 and 255 % 32 == 31
    info = check_case(255, range(4), (22, 3, 2, 1), stated, alone=(0, 3))
    assert (info["best_s"] >= 192).any()


@gpu
def test_one_rank_and_ranks_of_step_3():
    """RANKS = range(0, 1): one rank (rank_step 1), 90 items.  RANKS = 0, 3, ..., 18: the usable prefix is judged at
    base_val[3 r] -- 630 items, 450 (L = 2), 360, 180"""
    one = ((1, 90, 26, False, (1, 1, 0, 0)),) * 3
    check_case(90, range(0, 1), (22, 1, 22), one, alone=(0, 1))
    stated = ((7, 630, 54, False, (3, 3, 2, 2)), (5, 450, 2, True, (2, 2, 2, 1)), (4, 360, 40, False, (2, 2, 1, 1)),
              (2, 180, 52, False, (1, 1, 1, 0)))
    info = check_case(90, range(0, 21, 3), (22, 14, 10, 4), stated, alone=(1, 3))
    assert (info["best_rank"] > 0).any()


@gpu
def test_70_views_leftover_pairs_over_the_budget():
    """V = 70, the second 64-view block.  S = 100: every view (L = 40), 18 views (L = 4: 280 pairs fit), 4 views (L = 8:
    560 pairs > MH_S3_LEFT_PAIRS, the slice is kept).  S = 90: 6 views (L = 14: 980 pairs, the slice)"""
    v18 = [1, 5, 15, 16, 17, 31, 32, 33, 40, 47, 48, 49, 55, 63, 64, 65, 68, 69]
    v4, v6 = [3, 20, 64, 69], [2, 16, 33, 47, 64, 69]
    assert 4 * 70 <= 544 < 8 * 70 < 14 * 70
    stated = ((10, 1000, 40, False, (4, 4, 4, 4)), (9, 900, 4, True, (4, 4, 3, 3)), (2, 200, 8, False, (1, 1, 1, 1)))
    check_case(100, REF_RANKS, (70, 18, 4), stated, alone=(1, 2), V=70, seed=5, shown=[list(range(70)), v18, v4])
    stated = ((10, 900, 4, True, (4, 4, 3, 3)), (3, 270, 14, False, (2, 1, 1, 1)), (9, 810, 42, False, (4, 3, 3, 3)))
    check_case(90, REF_RANKS, (70, 6, 18), stated, alone=(1, 0), V=70, seed=5, shown=[list(range(70)), v6, v18])


# ---- what the entry points refuse, before they launch anything --------------------------------------------------------------
def refused(pm, pts, match):
    """forward() through mh_forward, mh_search_prepared and mh_search_forward raises MhError(match); the outputs keep their fill"""
    from monohair_amd import _lib

    N = len(pts)
    base = None
    for kw in (dict(), dict(base_view=True), dict(fused=False)):
        out = (torch.full((N, 3), -7.0, device=DEV), torch.full((N,), -7.0, device=DEV), torch.ones((N,), dtype=torch.bool, device=DEV))
        if kw.get("base_view"):
            kw["base_view"] = base
        with pytest.raises(_lib.MhError, match=match):
            pm.forward(pts, out=out, **kw)
        torch.cuda.synchronize()
        assert (out[0] == -7.0).all() and (out[1] == -7.0).all() and out[2].all()
        if base is None:        # (the ranking of these points, by the stand-alone calls)
            pm.Compute_Visible_and_Ori(pts)
            base = pm.Find_max_conf_from_visible_view()


@gpu
def test_rank_and_item_limits_are_refused_with_their_names():
    from monohair_amd import _lib
    from monohair_amd.pmvo import depth_offsets as offsets_of

    sc = Scene(22, 32, 64, 7, 3, min_dist=2, seed=1)
    pm = sc.context()
    pm.RANKS = range(20)                    # nrank = 20, rank_step = 1, S = 50: 1000 items, but more than MH_MAX_RANKS ranks
    pm.set_num_sample(50)
    refused(pm, sc.pts, r"nrank = 20 exceeds the limit of 16 base-view ranks \(MH_MAX_RANKS\)")
    pm.RANKS = range(0, 20, 2)              # nrank = 10, S = 128: 1280 items
    pm.set_num_sample(128)
    refused(pm, sc.pts, r"nrank \* S = 10 \* 128 items exceed the limit of 1024 items per point \(MH_MAX_ITEMS\)")
    assert len(offsets_of(257)) == 257
    with pytest.raises(_lib.MhError, match="S = 257 exceeds the limit of 256 samples"):
        pm.set_num_sample(257)
    assert pm.NUM_SAMPLE == 128             # ... and the context keeps the offsets it had
    pm.set_num_sample(90)
    pm.RANKS = range(0, 21, 2)              # (nrank - 1) * rank_step = 20: rank 20 of 20 ranked views
    refused(pm, sc.pts, r"nrank = 11, rank_step = 2 .*\(nrank - 1\) \* rank_step < 20")
    # the context still works, and at the limits: 16 ranks, 1024 items (compared in test_16_ranks_of_64_samples_exactly_1024_items)
    del pm.RANKS
    _, ori, loss, hc = pm.forward(sc.pts)
    _, o_ori, o_loss, o_hc = oracle.forward(sc.views(), sc.pts, 7, THR, offsets_of(90))
    assert np.array_equal(loss.cpu().numpy(), o_loss) and np.array_equal(ori.cpu().numpy(), o_ori)
    assert np.array_equal(hc.cpu().numpy(), o_hc)
