"""GPU: the leftover items of the shipped search (csrc/pmvo_search.hip: mh_left_batch, mh_left_sums).  A point's nvalid * 90
items fill whole 64-lane slices and leave L = (nvalid * 90) % 64; for 0 < L <= MH_S3_LEFT_MAX = 16 the workgroup's last wave
evaluates them one (item, view) pair per lane, per staging batch, and adds them up per item afterwards; every other L keeps
the slice.  Every output of forward() is compared bit for bit with oracle.forward, for the shipped kernel with the key body and
with the select body and for the portable kernel (search_variant 1256).

nvalid follows from how many views see a point: the ranks are every second entry of the 20 best views and a rank is usable
while its value is > 0, so k visible views give min(10, ceil(k / 2)) ranks:
    22 views -> 10 ranks, 900 items, L = 4        10 views -> 5 ranks, 450 items, L = 2
     6 views ->  3 ranks, 270 items, L = 14       16 views -> 8 ranks, 720 items, L = 16
    11 views ->  6 ranks, 540 items, L = 28: the first L above MH_S3_LEFT_MAX (the slice, as before)
    14 views ->  7 ranks, 630 items, L = 54: the control
The scenes are the hand-written ones of tests/test_search_staging_gpu.py (background depth: every view sees every point unless
the point's pixel is hidden; distinct tap angles; lists cut to a known length), 22 views of 32 x 64 (70 for the second 64-view
block).  Points that are only hidden may lie two pixels apart; points whose lists are cut lie a patch apart."""
import numpy as np
import pytest

import oracle
from test_search_staging_gpu import CAP, THR, Scene, batches, run

gpu = pytest.mark.gpu
LEFT_MAX = 16             # MH_S3_LEFT_MAX
LEFT_PAIRS = 544          # MH_S3_LEFT_PAIRS


def ranks(nvis):
    return max(1, min(10, (nvis + 1) // 2))


def leftover(nvis):
    """L of a point that nvis views see, and whether the last wave takes it"""
    L = (ranks(nvis) * 90) % 64
    return L, 0 < L <= LEFT_MAX


def show_only(sc, n, views):
    for v in range(sc.V):
        if v not in views:
            sc.hide(v, n)


def spread(V, n, k):
    """k of V views, spread over the range, with views that do not see the point between views that do"""
    return [v for v in range(V) if (v * 7 + n) % V < k]


VIS = (22, 10, 6, 16, 11, 14)


def counted_scene(codes, patch=7, vis=VIS):
    # seed 1: see test_every_leftover_count
    sc = Scene(22, 32, 64, patch, len(vis), min_dist=2, codes=codes, seed=1)
    for n, k in enumerate(vis):
        show_only(sc, n, spread(22, n, k))
    return sc


@gpu
@pytest.mark.parametrize("codes", [False, True])
def test_every_leftover_count(codes, depth_offsets):
    """L = 4, 2, 14, 16 (the last wave's job), 28 and 54 (slices) in one call, then three points, then every point alone: a
    point alone is the batch's last point, all its samples are trailing columns and overwrite what the leftover lanes wrote.
    Seed 1 of the point choice was found on the CPU (seeds 1, 2, ... against oracle.forward until one qualified; the first did):
    with it the oracle's winner of point 0 is (rank 9, sample 89) = item 899, the last of the four leftover items of 900."""
    assert [leftover(k) for k in VIS] == [(4, True), (2, True), (14, True), (16, True), (28, False), (54, False)]
    sc = counted_scene(codes)
    runs = ((0, 0), (2, 0), (0, 1256)) if codes else ((0, 0), (1, 0), (2, 0), (0, 1256))
    cnt, loss = run(sc, depth_offsets, runs=runs)
    assert [(cnt[:, n] > 0).sum() for n in range(len(VIS))] == list(VIS)
    assert (cnt[cnt > 0] == 49).all() and np.isfinite(loss).all()
    for n in range(len(VIS)):       # a view that does not see the point between two that do
        seen = np.nonzero(cnt[:, n])[0]
        assert VIS[n] == 22 or (np.diff(seen) > 1).any()
    if not codes:
        ex = oracle.forward(sc.views(), sc.pts, sc.patch, THR, depth_offsets, extra=True)[4]
        assert (int(ex["best_rank"][0]), int(ex["best_s"][0])) == (9, 89)       # item 899 >= 900 - 4
    run(sc, depth_offsets, runs=runs, pts=sc.pts[:3])
    for n in range(4):
        run(sc, depth_offsets, runs=runs, pts=sc.pts[n:n + 1])


@gpu
def test_short_lists_and_a_nan_tap_under_the_leftover_lanes(depth_offsets):
    """Two points a patch apart, 22 views each (L = 4).  Point 0: a one-tap list, a 10-tap and an 11-tap list (both sides of
    MH_KEY_MIN_TAPS: select body and key body in the slices, the same walk in the leftover lanes) among 49-tap lists, so the
    lanes of one pass walk lists of different lengths.  Point 1: the orientation of the second tap of view 6 and of the last
    tap of view 13 is NaN -- a NaN loss never replaces the running minimum."""
    sc = Scene(22, 32, 64, 7, 2, min_dist=9)
    expect = {(3, 0): 1, (8, 0): 10, (12, 0): 11, (4, 0): 49, (6, 1): 49, (13, 1): 49}
    for (v, n), c in expect.items():
        if c < 49:
            sc.cut(v, n, c)
    r, c = sc.pix[6, 1]
    sc.ori[6, r - 3, c - 2] = np.nan
    r, c = sc.pix[13, 1]
    sc.ori[13, r + 3, c + 3] = np.nan
    cnt, loss = run(sc, depth_offsets, expect)
    assert (cnt > 0).all() and np.isfinite(loss).all()


@gpu
@pytest.mark.parametrize("patch", [3, 9])
def test_patch_3_and_9(patch, depth_offsets):
    """patch 3: nine taps, every list through the select body; patch 9: the kernel for lists of more than 64 taps, and 22 lists
    of 82 records do not fit the staging buffer -- the leftover pairs of point 0 are evaluated in two batches and added up
    across them.  L = 4, 2, 16."""
    vis = (22, 10, 16)
    sc = counted_scene(False, patch=patch, vis=vis)
    cnt, loss = run(sc, depth_offsets)
    assert [(cnt[:, n] > 0).sum() for n in range(3)] == list(vis) and (cnt[cnt > 0] == patch * patch).all()
    assert np.isfinite(loss).all()
    assert len(batches(cnt[:, 0], True, bigp=True)) == (2 if patch == 9 else 1)


@gpu
def test_three_batches_and_the_second_64_view_block(depth_offsets):
    """V = 70, patch 7.  Point 0: every view (3 500 records: three batches in the first block, one in the second; 4 x 70 pairs
    fit).  Point 1: 20 views on both sides of view 16, 32, 48 (the cascade's flushes) and 64 (the second block), L = 4.  Point 2:
    nine views, among them 16, 64 and 69, L = 2."""
    sc = Scene(70, 32, 64, 7, 3, min_dist=2)
    v1 = [5, 15, 16, 17, 30, 31, 32, 33, 46, 47, 48, 49, 62, 63, 64, 65, 66, 67, 68, 69]
    v2 = [2, 14, 16, 33, 47, 50, 63, 64, 69]
    show_only(sc, 1, v1)
    show_only(sc, 2, v2)
    assert leftover(70) == (4, True) and leftover(len(v1)) == (4, True) and leftover(len(v2)) == (2, True)
    assert 4 * 70 <= LEFT_PAIRS
    cnt, loss = run(sc, depth_offsets)
    assert (cnt[:, 0] == 49).all() and np.isfinite(loss).all()
    assert list(np.nonzero(cnt[:, 1])[0]) == v1 and list(np.nonzero(cnt[:, 2])[0]) == v2
    assert len(batches(cnt[:64, 0], True)) == 3 and batches(cnt[:64, 0], True)[0] <= CAP
