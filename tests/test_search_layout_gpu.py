"""GPU: the odd item of a wave in the shipped search (csrc/pmvo_search.hip: mh_search_slices_lds; csrc/mh_device.h:
mh_pixel_of_fast1, mh_unit2_fast1).  A wave holds up to four item slices (slice j of wave w: the items from j * 256 + w * 64) and
projects its items two at a time (mh_pixel_of_fast2, the divisions of a pair sharing their instructions); a wave with one or
three slices has an odd item, which goes through the one-item twins of the pair forms -- the same operations in the same order,
so the same bits.  The shapes here are chosen by the slices they give the waves: 3 and 1 in waves with and without the
leftover items (mh_left_batch), next to waves of 4, 2 and 0; the largest shapes (960 and 1024 items); staging batches of fewer
lists than waves, of more, and a point that needs two batches; a batch whose last point carries trailing columns; a context of
8-bit views (the select-only kernel).

Every case compares line_ori, min_loss, high_conf, best_s and best_rank bit for bit, NaN == NaN, with oracle.forward, for the
shipped kernel by the maps, with the key body and with the select body, and for the portable kernel (search_variant 1256),
which has no pair form.  The scenes are the hand-written ones of tests/test_search_staging_gpu.py: every list complete (49 taps
of patch 7), k views see a point, so nvalid = min(nrank, ceil(k / rank_step)) ranks are usable.  Each case states the slices of
the waves it means to reach as literals and checks them against plan() of tests/test_search_shapes_gpu.py, a restatement of
the kernel's prologue.

(What this file was first written for, a workgroup of five waves x three slots, lost on the GPU and is not in the library:
profiles/search_five_waves.txt.)"""
import numpy as np
import pytest

from test_search_leftover_gpu import show_only, spread
from test_search_shapes_gpu import plan
from test_search_staging_gpu import CAP, Scene, batches, run

gpu = pytest.mark.gpu
REF_RANKS = range(0, 20, 2)
RUNS = ((0, 0), (1, 0), (2, 0), (0, 1256))       # (search_body, search_variant)
CODES = ((0, 0), (2, 0), (0, 1256))


def check(S, ranks, vis, stated, V=22, codes=False, alone=(0,), seed=1):
    """the scene of len(vis) points, point n seen by vis[n] views; the stated plan; the batch as a whole, its first three
    points, the points `alone` (a point alone is the batch's last point: its last S % 32 samples are trailing columns)"""
    ranks = list(ranks)
    runs = CODES if codes else RUNS
    assert [plan(S, ranks, k, V) for k in vis] == list(stated)
    sc = Scene(V, 32, 64, 7, len(vis), min_dist=2, codes=codes, seed=seed)
    for n, k in enumerate(vis):
        show_only(sc, n, spread(V, n, k))
    info = {}
    cnt, loss = run(sc, None, runs=runs, ranks=ranks, num_sample=S, info=info)
    assert [(cnt[:, n] > 0).sum() for n in range(len(vis))] == list(vis)
    assert (cnt[cnt > 0] == 49).all() and np.isfinite(loss).all()
    assert list(info["nvalid"]) == [p[0] for p in stated]
    if len(vis) > 3:
        run(sc, None, runs=runs, ranks=ranks, num_sample=S, pts=sc.pts[:3])
    for n in alone:
        run(sc, None, runs=runs, ranks=ranks, num_sample=S, pts=sc.pts[n:n + 1])
    return cnt, info


@gpu
def test_waves_of_three_and_of_one_slice_with_trailing_columns():
    """10 ranks x 90: 14 slices + 4 leftover items -- waves 2 and 3 hold three slices, wave 3 also the leftover pairs; 9 usable
    ranks: 810 items, the thirteenth slice partial, three waves of three; 1 usable rank: 90 items, waves 0 and 1 one slice
    (the second partial), waves 2 and 3 none; 2 usable ranks (4 views: a batch of as many lists as waves): 180 items, three
    waves of one; 3 usable ranks (6 views): 270 items, 14 leftover items next to one wave of one slice.
    Six points: 540 columns, the last 28 samples of point 5 are trailing columns and overwrite what its leftover lanes wrote;
    three points: 270 columns, 14 trailing ones in the 2-view point; a point alone: 26."""
    stated = ((10, 900, 4, True, (4, 4, 3, 3)), (9, 810, 42, False, (4, 3, 3, 3)), (1, 90, 26, False, (1, 1, 0, 0)),
              (2, 180, 52, False, (1, 1, 1, 0)), (10, 900, 4, True, (4, 4, 3, 3)), (3, 270, 14, True, (1, 1, 1, 1)))
    assert (6 * 90) % 32 == 28 and (3 * 90) % 32 == 14 and 90 % 32 == 26
    cnt, info = check(90, REF_RANKS, (22, 18, 2, 4, 22, 6), stated, alone=(0, 1, 3))
    assert (info["best_rank"] > 0).any()


@gpu
def test_960_and_1024_items():
    """15 ranks x 64 samples = 960 items: exactly 15 slices, the last wave three; 14 usable ranks: 896 items, two waves of
    three.  The same points with 16 ranks: 1024 items = MH_MAX_ITEMS, four slices everywhere."""
    stated = ((15, 960, 0, False, (4, 4, 4, 3)), (14, 896, 0, False, (4, 4, 3, 3)), (13, 832, 0, False, (4, 3, 3, 3)))
    check(64, range(15), (22, 14, 13), stated)
    stated = ((16, 1024, 0, False, (4, 4, 4, 4)), (14, 896, 0, False, (4, 4, 3, 3)), (13, 832, 0, False, (4, 3, 3, 3)))
    cnt, info = check(64, range(16), (22, 14, 13), stated)
    assert (info["best_rank"] > 0).any()


@gpu
def test_two_staging_batches():
    """30 views, every list 50 records: 25 lists fill the first batch (1250 of 1280 records), the last five are a second one;
    the odd item of waves 2 and 3 is projected in 30 views across both, and the leftover pairs of the 900 items (4 x 30) are
    evaluated per batch and added up across them.  Point 2: seven views, 360 items -- wave 0 two slices, the others one."""
    stated = ((10, 900, 4, True, (4, 4, 3, 3)),) * 2 + ((4, 360, 40, False, (2, 2, 1, 1)),)
    cnt, info = check(90, REF_RANKS, (30, 30, 7), stated, V=30, seed=5)
    assert batches(cnt[:, 0], True) == [1250, 250] and batches(cnt[:, 0], True)[0] <= CAP
    assert len(batches(cnt[:, 2], True)) == 1


@gpu
def test_an_8bit_context():
    """views uploaded as 8-bit codes: the select-only kernel, which keeps the leftover items as a slice -- 900 items are
    (4, 4, 4, 3) there, 810 (4, 3, 3, 3), 90 (1, 1, 0, 0); plan() states the key kernels' slices"""
    stated = ((10, 900, 4, True, (4, 4, 3, 3)), (9, 810, 42, False, (4, 3, 3, 3)), (1, 90, 26, False, (1, 1, 0, 0)))
    check(90, REF_RANKS, (22, 18, 2), stated, codes=True)
