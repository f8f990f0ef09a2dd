"""GPU: the block-key body of the one-group key kernels (csrc/pmvo_search.hip: mh_key_blockm4, mh_seed_key).  The running
minimum of a list is kept per four-tap BLOCK -- key = (min of the block's four t' << 4) | block, one accumulator per item, the
list's last tap seeding it under its own block's number -- and the winning TAP is found after the walk: the lane reads its
winning block's taps again and takes the first whose t' equals the minimum.  What can go wrong there, and no more:
  * a list length at which the walk, the padding of the last block or the seed's block is off: every length 11 .. 49 (patch 7:
    a one-group list has at most 49 taps; the 64-tap list of the issue exists only under patch 9, whose kernel keeps the per-tap
    keys -- it is run here all the same, with its neighbours 63 and 65).  The (0, 0) records behind a list must neither win nor
    send an ordinary list to the re-evaluation branch: mh_debug_key_stats stays at 0 there;
  * the order of ties: two taps of ONE block with the same loss bit for bit (the earlier one wins, first and third and first and
    fourth of the block), the same loss in two blocks (the earlier block wins), the seeded tap against a tap of an earlier block
    and against a tap of its own block;
  * where the winner sits: tap 0, the first block, the last walked block, the seeded tap (49: a block of its own; 47 and 46: inside
    the last walked block, behind which lie padding records);
  * a winner with |cos| <= 2^-14, which the key cannot state: the re-evaluation branch (asserted on mh_debug_key_stats, as
    tests/test_key_reeval_gpu.py does), with and without a NaN tap; a NaN tap beside the winner in an ordinary list;
  * a wrong block or a wrong tap inside it: a fan of taps across the directions of a rank's samples, so that the winning blocks
    differ among the lanes of a wave, every tap with a confidence of its own -- the weight of that view in the item's loss;
  * 9 usable ranks, 1 usable rank, and a point with leftover items (22 views: 900 items, four of them left over).
Every output of forward() is compared bit for bit with oracle.forward and with the portable kernel (search_variant 1256), for
the shipped kernel's default, key and select bodies.

The scenes are the hand-written ones of tests/test_search_staging_gpu.py (22 views of 32 x 64, two points a patch apart).  A
construction is built around ONE item of a point: the oracle's winner (rank, sample), the only item whose loss forward() returns.
Its direction in a view that is no base view of the point is read from the oracle, the 7 x 7 patch of that view is rewritten
(orientations 0.3 .. 0.8 rad off that direction, the taps of the case along it; the centre cell keeps its confidence, so the
ranking of the views stays), the winner is looked up again, and all of it is asserted on the final maps before the GPU runs.
A tie between taps that are no duplicates: the same orientation with the opposite sign."""
import numpy as np
import pytest

import oracle
from test_key_seed_gpu import key_stats, rot, spread
from test_search_leftover_gpu import leftover, show_only
from test_search_leftover_gpu import spread as views_spread
from test_search_staging_gpu import THR, Scene

gpu = pytest.mark.gpu
RUNS = ((0, 0), (1, 0), (2, 0), (0, 1256))      # (search_body, search_variant): default, key, select, the portable kernel
P = 49


def forward_all(sc, offsets, expect=None):
    """forward() in every run of RUNS against oracle.forward and against the portable kernel; expect = {(v, n): list length}.
    Returns the [V, N] list lengths and mh_debug_key_stats after each run."""
    pm = sc.context()
    _, o_ori, o_loss, o_hc, o_ex = oracle.forward(sc.views(), sc.pts, sc.patch, THR, offsets, extra=True)
    ref = (o_ori, o_loss, o_hc, o_ex["best_s"], o_ex["best_rank"])
    assert np.isfinite(o_loss).all()
    key_stats(pm)
    got, stats, cnt = {}, {}, None
    try:
        for body, variant in RUNS:
            pm.set_option("search_body", body)
            pm.set_option("search_variant", variant)
            _, ori, loss, hc, ex = pm.forward(sc.pts, extras=True)
            stats[(body, variant)] = key_stats(pm)
            got[(body, variant)] = tuple(x.cpu().numpy() for x in (ori, loss, hc, ex["best_s"], ex["best_rank"]))
            if cnt is None:
                cnt = pm.search_work(len(sc.pts), ex["base_val"])[0].cpu().numpy()
                for (v, n), c in (expect or {}).items():
                    assert cnt[v, n] == c, (v, n, c, int(cnt[v, n]))
    finally:
        pm.set_option("search_body", 0)
        pm.set_option("search_variant", 0)
    for run, out in got.items():
        for a, b, c in zip(out, ref, got[(0, 1256)]):
            assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), ("oracle", run)
            assert np.array_equal(a, c, equal_nan=(a.dtype.kind == "f")), ("portable", run)
    return cnt, stats


# ---------------------------------------------------------------------------------------------------------------------------
# every list length
# ---------------------------------------------------------------------------------------------------------------------------
LENGTHS7 = list(range(11, 50))
LENGTHS9 = [63, 64, 65]

_cache = {}


def cached(fn):
    def get(offsets):
        if fn.__name__ not in _cache:
            _cache[fn.__name__] = fn(offsets)
        return _cache[fn.__name__]
    return get


@cached
def length_scene7(offsets):
    sc = Scene(22, 32, 64, 7, 2, min_dist=9)
    pairs = [(v, n) for n in range(2) for v in range(22)]
    expect = {}
    for (v, n), c in zip(pairs, LENGTHS7):
        sc.cut(v, n, c)
        expect[(v, n)] = c
    return sc, expect


@cached
def length_scene9(offsets):
    sc = Scene(22, 32, 64, 9, 1, min_dist=11)
    expect = {(5, 0): 63, (9, 0): 64, (12, 0): 65}
    for (v, n), c in expect.items():
        sc.cut(v, n, c)
    return sc, expect


# ---------------------------------------------------------------------------------------------------------------------------
# constructions around the winning item
# ---------------------------------------------------------------------------------------------------------------------------
def winners(sc, offsets):
    """per point: the oracle's winner (rank, sample), the unit directions [V, S, 2] of that rank's samples, the base views"""
    views = sc.views()
    o = oracle.visible_and_ori(views, sc.pts, sc.patch)
    bidx, _ = oracle.topk_views(o["visible"], o["Conf"], 20)
    ex = oracle.forward(views, sc.pts, sc.patch, THR, offsets, extra=True)[4]
    out = []
    for n in range(len(sc.pts)):
        r, s = int(ex["best_rank"][n]), int(ex["best_s"][n])
        D = oracle.reproject_ori(views, sc.pts, oracle.sample_next(views, sc.pts, bidx[2 * r], o["Ori"], offsets))[:, n]
        D = D.astype(np.float64)
        out.append(dict(r=r, s=s, D=D / np.linalg.norm(D, axis=-1, keepdims=True), base=set(int(b) for b in bidx[0:20:2, n])))
    return out, o


def write(sc, v, n, oris, confs, count):
    hp, k = 3, 0
    r, c = sc.pix[v, n]
    for i in range(-hp, hp + 1):
        for j in range(-hp, hp + 1):
            sc.ori[v, r + i, c + j] = np.asarray(oris[k], np.float32)
            sc.conf[v, r + i, c + j] = 0.9 if k == P // 2 else (confs[k] if k < count else 0.05)
            k += 1


def base_patch(d):
    """49 distinct orientations 0.3 .. 0.8 rad off d, every tap with a confidence of its own"""
    oris, _ = spread(d, P, P)
    return oris, [0.5 + 0.008 * k for k in range(P)]


def case_win(t):
    def make(d):
        oris, confs = base_patch(d)
        oris[t] = d
        return oris, confs
    return make


def case_tie(t1, t2):
    def make(d):
        oris, confs = base_patch(d)
        first = np.asarray(d, np.float32)
        oris[t1], oris[t2] = first, -first
        return oris, confs
    return make


def case_nan_beside(t, tn):
    def make(d):
        oris, confs = base_patch(d)
        oris[t] = d
        oris[tn] = np.array([np.nan, np.nan])
        return oris, confs
    return make


def case_perp(nan_at=None):
    def make(d):
        perp = np.array([-d[1], d[0]])
        oris = [rot(perp, (k - P // 2) * 2e-6) for k in range(P)]
        if nan_at is not None:
            oris[nan_at] = np.array([np.nan, np.nan])
        return oris, [0.5 + 0.008 * k for k in range(P)]
    return make


def build_cases(offsets, cases):
    """cases[n] = [(kind, args, count)]: the cases of point n, one free view each, built around the winner of the scene as it
    stands.  Rewriting its views may make another item the winner (one of a neighbouring direction, or -- where the taps are
    all perpendicular to it -- any other): every case is asserted on the final maps against the FINAL winner's direction, with a
    margin of 0.01 in |cos| between the taps of the case and every other tap; a tie holds for every direction.  The perpendicular
    fans are asserted against the item they were built around: the wave of that item enters the re-evaluation branch."""
    sc = Scene(22, 32, 64, 7, 2, min_dist=9)
    makers = dict(win=case_win, tie=case_tie, nan=case_nan_beside, perp=case_perp)
    win, _ = winners(sc, offsets)
    placed = []
    for n, todo in enumerate(cases):
        free = [v for v in range(sc.V) if v not in win[n]["base"]]
        assert len(free) >= len(todo)
        for v, (kind, args, count) in zip(free, todo):
            write(sc, v, n, *makers[kind](*args)(win[n]["D"][v, win[n]["s"]]), count)
            placed.append((v, n, kind, args, count))
    after, o = winners(sc, offsets)
    for v, n, kind, args, count in placed:
        w = after[n]
        assert v not in w["base"] and w["base"] == win[n]["base"] and o["visible"][v, n] != -1.0
        op = o["Ori_patch"][v, n]
        taps = op.astype(np.float64)
        ok = np.isfinite(taps).all(axis=1)
        taps[ok] /= np.linalg.norm(taps[ok], axis=1, keepdims=True)
        if kind == "perp":      # (the samples of a rank do not depend on the views that are no base views)
            ac = np.abs(taps @ win[n]["D"][v, win[n]["s"]])[:count]
            assert np.nanmax(ac) < 2.0 ** -14
            assert (~ok[:count]).sum() == (0 if args[0] is None else 1)
            continue
        ac = np.abs(taps @ w["D"][v, w["s"]])[:count]
        special = list(args)
        if kind == "tie":
            assert np.array_equal(op[args[1]], -op[args[0]]) and ac[args[0]] == ac[args[1]]
        if kind == "nan":
            assert not ok[args[1]] and args[0] // 4 == args[1] // 4
            special = [args[0]]
        assert all(t < count for t in special)
        assert ac[special[0]] > np.nanmax(np.delete(ac, list(args))) + 0.01, (v, n, kind, args)
    return sc, {(v, n): count for v, n, kind, args, count in placed}


# point 0: ties; point 1: where the winner sits.  Tap t lies in block t // 4; a list of c taps seeds tap c - 1.
TIES = [("tie", (20, 22), 49), ("tie", (28, 31), 49), ("tie", (21, 20 + 3), 49), ("tie", (9, 30), 49), ("tie", (3, 4), 49),
        ("tie", (10, 48), 49), ("tie", (46, 48), 49), ("tie", (44, 45), 46), ("tie", (13, 46), 47), ("tie", (0, 47), 49)]
PLACES = [("win", (0,), 49), ("win", (2,), 49), ("win", (3,), 49), ("win", (46,), 49), ("win", (47,), 49), ("win", (48,), 49),
          ("win", (45,), 47), ("win", (46,), 47), ("win", (45,), 46), ("win", (44,), 46), ("nan", (18, 17), 49),
          ("nan", (46, 47), 49)]


@cached
def tie_scene(offsets):
    return build_cases(offsets, [TIES, PLACES])


@cached
def reeval_scene(offsets):
    return build_cases(offsets, [[("perp", (None,), 49)], [("perp", (30,), 49), ("perp", (None,), 47)]])


def winning_blocks(D, oris, count=P):
    """block of the first-index minimum-loss tap (float64) of every direction of D [S, 2]"""
    taps = np.asarray(oris, np.float64)[:count]
    taps /= np.linalg.norm(taps, axis=1, keepdims=True)
    return np.argmax(np.abs(D @ taps.T), axis=1) // 4


def fan(sc, win):
    """in every view that is no base view of a point: 49 taps fanned across the directions of the winning rank's samples, in a
    scrambled order, so that neighbouring directions win in different blocks; every tap with a confidence of its own"""
    for n, w in enumerate(win):
        for v in range(sc.V):
            if v in w["base"]:
                continue
            D = w["D"][v]
            d = D[w["s"]]
            ang = np.arcsin(np.clip(D[:, 0] * d[1] - D[:, 1] * d[0], -1, 1) * np.sign(D @ d))     # of the samples, from d
            lo, hi = ang.min(), max(ang.max(), ang.min() + 1e-3)
            oris = [rot(d, -(lo + (hi - lo) * ((k * 37) % P) / (P - 1))) for k in range(P)]
            write(sc, v, n, oris, [0.3 + 0.01 * k for k in range(P)], P)


@cached
def fan_scene(offsets):
    """the fan around the winner's rank; if that makes an item of another rank the winner, once more around that rank.  Returns
    the scene, the final winners and, per (point, rewritten view), the winning block of every sample of the winner's rank"""
    sc = Scene(22, 32, 64, 7, 2, min_dist=9)
    for _ in range(4):
        win, _ = winners(sc, offsets)
        fan(sc, win)
        after, o = winners(sc, offsets)
        if [w["r"] for w in after] == [w["r"] for w in win]:
            break
    else:
        raise AssertionError("the winner's rank does not settle")
    blocks = [(n, v, winning_blocks(w["D"][v], o["Ori_patch"][v, n])) for n, w in enumerate(after) for v in range(sc.V)
              if v not in w["base"]]
    return sc, after, blocks


@cached
def rank_scene(offsets):
    """22 views: 10 ranks, 900 items, four left over; 18 views: 9 ranks; 2 views: 1 rank"""
    vis = (22, 18, 2)
    sc = Scene(22, 32, 64, 7, len(vis), min_dist=2, seed=1)
    for n, k in enumerate(vis):
        show_only(sc, n, views_spread(22, n, k))
    return sc, vis


def test_the_constructions_hold(depth_offsets):
    """the CPU half: every scene builds (build_cases asserts its cases on the final maps), the oracle's losses are finite, the fan
    spreads the winning blocks of a rank's samples"""
    for make in (length_scene7, length_scene9, tie_scene, reeval_scene):
        sc, expect = make(depth_offsets)
        assert np.isfinite(oracle.forward(sc.views(), sc.pts, sc.patch, THR, depth_offsets)[2]).all()
    assert sorted(length_scene7(depth_offsets)[1].values()) == LENGTHS7
    sc, win, blocks = fan_scene(depth_offsets)
    assert len(blocks) == 2 * 12
    for n, v, b in blocks:
        # the 64 items of the winner's wave that belong to its rank (a wave's lanes are 64 consecutive items, item = rank * 90 + sample)
        it = win[n]["r"] * 90 + win[n]["s"]
        lo, hi = max(it // 64 * 64, win[n]["r"] * 90), min(it // 64 * 64 + 64, win[n]["r"] * 90 + 90)
        lanes = b[lo - win[n]["r"] * 90:hi - win[n]["r"] * 90]
        assert len(set(b)) >= 6, (n, v, sorted(set(b)))
        assert len(set(lanes)) >= min(len(lanes), 3), (n, v, lanes)
    sc, vis = rank_scene(depth_offsets)
    assert [leftover(k) for k in vis] == [(4, True), (42, False), (26, False)]


@gpu
def test_every_list_length_11_to_49(depth_offsets):
    sc, expect = length_scene7(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert sorted(int(cnt[v, n]) for (v, n) in expect) == LENGTHS7
    assert all(st[2] == 0 for st in stats.values()), stats          # no padding record sends a list to the re-evaluation


@gpu
def test_lists_of_63_64_65_taps_patch9(depth_offsets):
    sc, expect = length_scene9(depth_offsets)
    forward_all(sc, depth_offsets, expect)


@gpu
def test_ties_and_where_the_winner_sits(depth_offsets):
    sc, expect = tie_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_winner_within_2_to_minus_14_enters_the_reevaluation(depth_offsets):
    sc, expect = reeval_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert stats[(0, 0)][2] > 0 and stats[(1, 0)][2] > 0, "the key body's re-evaluation branch was not entered"
    assert stats[(2, 0)][2] == 0 and stats[(0, 1256)][2] == 0       # (the select body and the portable kernel build no keys)


@gpu
def test_winning_blocks_differ_lane_by_lane(depth_offsets):
    sc, win, blocks = fan_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets)
    assert (cnt == P).all()


@gpu
def test_nine_ranks_one_rank_and_leftover_items(depth_offsets):
    sc, vis = rank_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets)
    assert [(cnt[:, n] > 0).sum() for n in range(len(vis))] == list(vis)
