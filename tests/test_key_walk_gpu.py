"""GPU: the straight-line walk of a complete 7 x 7 patch (csrc/mh_key_blocks.h: mh_key_walk<12>, taken in csrc/pmvo_search.hip
by every list of exactly 49 taps in the kernels for up to 256 views; every other length keeps the loop over blocks).  The walk is
the loop's blocks with their number, their parity and the offsets of their taps as constants, so what it could get wrong is what
a constant could be wrong in, and where the two paths meet:
  * a block under another block's number or read from another block's records: the winner in each of the 48 walked taps -- every
    place of every block -- and in the seeded last tap, as a NEGATIVE cosine, every tap with a confidence of its own;
  * the fold of a pair of blocks: the same |cos| in an earlier and a later block (the earlier wins), in the two blocks of one
    pair, in two taps of one block (the first wins), in a walked tap and the seeded one;
  * NaN taps: beside the winner in the first and in the last walked block, and a whole block of them;
  * a minimum the key cannot state: lists of 49 taps that take the bad-key route into the re-evaluation (mh_debug_key_stats [2]);
  * both paths in one workgroup: views with 49 taps beside views with 48, 45, 11 and 10 taps of the same point (the walk, the
    loop with an even and an odd number of blocks, and the select body for the short list, in one batch);
  * the instantiations: points with 10, 9, 8, 5 and 1 usable ranks -- 4, 3, 2 and 1 item slices per wave and the waves that take
    the leftover items;
  * a point whose lists need two staging batches.
Every output of forward() is compared bit for bit with oracle.forward and with the portable kernel (search_variant 1256), for the
shipped kernel's default, key and select bodies (tests/test_key_block_gpu.py: forward_all).  The scenes and the cases are those
of tests/test_key_block_max_gpu.py (build: every case is asserted on the final maps, on the numpy restatement of a tap's fp32
arithmetic, before the GPU runs)."""
import numpy as np
import pytest

import oracle
from test_key_block_gpu import P, forward_all
from test_key_block_max_gpu import bad, build, cells, cs32, place, unit32, winners32
from test_search_leftover_gpu import leftover, ranks, show_only
from test_search_leftover_gpu import spread as views_spread
from test_search_staging_gpu import CAP, THR, Scene, batches

gpu = pytest.mark.gpu

# tap t lies in block t // 4, place t % 4; a list of 49 taps walks taps 0 .. 47 in twelve blocks and seeds tap 48
PLACES = [("neg", (t,), P) for t in range(P)]
TIES = [("tie", (9, 30), P), ("tie", (2, 45), P), ("tie", (16, 21), P), ("tie", (20, 22), P), ("tie", (44, 47), P),
        ("tie", (10, 48), P), ("tie", (47, 48), P)]
NANS = [("nan", (2, (1,)), P), ("nan", (0, (3,)), P), ("nan", (46, (45,)), P), ("nan", (30, (8, 9, 10, 11)), P),
        ("nan", (5, (44, 45, 46, 47)), P)]

_cache = {}


def cached(fn):
    def get(offsets):
        if fn.__name__ not in _cache:
            _cache[fn.__name__] = fn(offsets)
        return _cache[fn.__name__]
    return get


@cached
def places_a(offsets):
    return build(offsets, [PLACES[0:12], PLACES[12:24]])


@cached
def places_b(offsets):
    return build(offsets, [PLACES[24:36], PLACES[36:48]])


@cached
def ties_nans(offsets):
    return build(offsets, [PLACES[48:] + TIES, NANS])


@cached
def bad_scene(offsets):
    """two lists of 49 taps, every tap perpendicular to the item they are built around within 2^-14 but a NaN one and a (0, 0)
    one -- in the first block and in the last walked block; asserted against that item, whose wave enters the re-evaluation"""
    plan = [[(bad(1, 2), P)], [(bad(47, 44), P)]]
    sc = Scene(22, 32, 64, 7, len(plan), min_dist=9)
    win, o0 = winners32(sc, offsets)
    placed = []
    for n, todo in enumerate(plan):
        free = [v for v in range(sc.V) if v not in win[n]["base"]]
        for v, (make, L) in zip(free, todo):
            place(sc, v, n, make, L, win[n])
            placed.append((v, n, L))
    after, o = winners32(sc, offsets)
    for v, n, L in placed:
        assert v not in after[n]["base"] and after[n]["base"] == win[n]["base"] and o["visible"][v, n] != -1.0
        el = o["Conf_patch"][v, n] > THR
        el[0] = True
        assert list(np.nonzero(el)[0]) == cells(L)
        taps = unit32(o["Ori_patch"][v, n][el])
        cs = cs32(taps, unit32(win[n]["D"][v, win[n]["s"]]))
        assert np.isnan(cs).sum() == 1 and (taps == 0).all(axis=1).sum() == 1 and np.nanmax(np.abs(cs)) < 2.0 ** -14
    return sc, {(v, n): L for v, n, L in placed}


MIXED = {3: 48, 5: 45, 8: 11, 12: 10, 17: 48, 20: 11}      # view: list length of point 0; every other list has 49 taps


@cached
def mixed_scene(offsets):
    sc = Scene(22, 32, 64, 7, 2, min_dist=9)
    for v, c in MIXED.items():
        sc.cut(v, 0, c)
    expect = {(v, 0): c for v, c in MIXED.items()}
    expect.update({(v, 0): P for v in range(22) if v not in MIXED})
    expect.update({(v, 1): P for v in range(22)})
    return sc, expect


VIS = (22, 18, 16, 10, 2)           # views that see the point: 10, 9, 8, 5 and 1 usable ranks


@cached
def rank_scene(offsets):
    sc = Scene(22, 32, 64, 7, len(VIS), min_dist=2, seed=1)
    for n, k in enumerate(VIS):
        show_only(sc, n, views_spread(22, n, k))
    return sc, VIS


def test_the_constructions_hold(depth_offsets):
    """the CPU half: every scene builds (build() asserts each case on the final maps), the oracle's losses are finite, the 49
    winner places are those of the twelve blocks and the seed, and the points of the rank scene have the ranks and leftovers meant"""
    assert sorted(a[0] for k, a, L in PLACES) == list(range(P)) and all(L == P for k, a, L in PLACES + TIES + NANS)
    assert {(a[0] // 4, a[0] % 4) for k, a, L in PLACES[:48]} == {(b, u) for b in range(12) for u in range(4)}
    for make in (places_a, places_b, ties_nans, bad_scene, mixed_scene):
        sc, expect = make(depth_offsets)
        assert np.isfinite(oracle.forward(sc.views(), sc.pts, sc.patch, THR, depth_offsets)[2]).all()
    assert [ranks(k) for k in VIS] == [10, 9, 8, 5, 1]
    # items = 90 * ranks in slices of 64: 14, 12, 11, 7 and 1 full slices over four waves (4, 3, 2 and 1 per wave all occur),
    # and leftovers of 4, 42, 16, 2 and 26 items
    assert [leftover(k) for k in VIS] == [(4, True), (42, False), (16, True), (2, True), (26, False)]


@gpu
@pytest.mark.parametrize("scene", [places_a, places_b], ids=["taps_0_23", "taps_24_47"])
def test_the_winner_in_every_place_of_every_block(scene, depth_offsets):
    sc, expect = scene(depth_offsets)
    assert len(expect) == 24 and set(expect.values()) == {P}
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_the_seeded_tap_ties_and_nan_taps(depth_offsets):
    sc, expect = ties_nans(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_lists_of_49_taps_take_the_bad_key_route(depth_offsets):
    sc, expect = bad_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert stats[(0, 0)][2] > 0 and stats[(1, 0)][2] > 0, "the key body's re-evaluation branch was not entered"
    assert stats[(2, 0)][2] == 0 and stats[(0, 1256)][2] == 0       # (the select body and the portable kernel build no keys)


@gpu
def test_the_walk_the_loop_and_short_lists_in_one_workgroup(depth_offsets):
    sc, expect = mixed_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert sorted(set(int(c) for c in cnt[:, 0])) == [10, 11, 45, 48, 49]
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_ten_nine_eight_five_and_one_usable_ranks(depth_offsets):
    sc, vis = rank_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets)
    assert [(cnt[:, n] > 0).sum() for n in range(len(vis))] == list(vis) and (cnt[cnt > 0] == P).all()


@gpu
def test_a_point_whose_lists_take_two_staging_batches(depth_offsets):
    """30 views, complete lists of 50 records each: 1 500 records do not fit the staging buffer's 1 280"""
    sc = Scene(30, 240, 160, 7, 2, min_dist=8)
    cnt, stats = forward_all(sc, depth_offsets)
    assert (cnt == P).all() and all(len(batches(cnt[:, n], True)) == 2 and batches(cnt[:, n], True)[0] <= CAP for n in range(2))
