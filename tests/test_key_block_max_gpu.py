"""GPU: the block-key body with the MAXIMUM first (csrc/mh_key_blocks.h: mh_key_blockm4 as tools/gen_key_blocks.py writes it).
A block no longer makes the four t' = fl(C - |cs|) and takes their minimum: it takes the maximum of the four |cs| (v_max_f32,
v_max3_f32 with |.| on the sources) and subtracts once.  fl(C - x) is monotone non-increasing in x, so the block's m is the same
bits; what tests/test_key_block_gpu.py does not pin, and this block could get wrong:
  * a missing or misplaced |.|: the winning tap has a NEGATIVE cosine, in each of the four places of a block, in the first, a
    middle and the last walked block (and in the last blocks of lists of 13, 14, 15 and 16 taps, so that every padding of c - 1
    to whole blocks occurs); the confidences differ tap by tap, so the output names the tap;
  * sign ties: orientations t and -t (equal |cs|, opposite sign) in places (0, 1), (0, 3), (2, 3) of one block and in two
    different blocks: the earlier tap wins;
  * different |cs|, equal loss: two orientations whose fp32 cs differ while fl(1 - |cs|) is the same float (|cs| in [0.25, 0.5):
    the grid of cs is finer than that of the loss), in one block in both orders and in two blocks in both orders: the maximum of
    |cs| then names the LATER tap in one order of each, and the earlier tap must win all the same (the decode compares t');
  * NaN in the fold: a NaN tap in each of the four places of a block that also holds the list's winner, and a block of four NaN
    taps beside a valid winner elsewhere; mh_debug_key_stats()[2] stays 0;
  * the bad-key route: a list whose every tap is perpendicular to the item, NaN or (0, 0): the re-evaluation counter rises and
    the outputs are equal.
Shapes: patch 7, 22 views of 32 x 64, two to four points; a point all views see has 10 x 90 items (waves of 4, 4, 3, 3 slices and
four leftover items), a point two views see has 1 x 90 (a wave of one slice, waves of none).  Every output of forward() is
compared bit for bit with oracle.forward, the select body (search_body 2) and the portable kernel (search_variant 1256):
forward_all of tests/test_key_block_gpu.py.

A case is built like those of tests/test_key_block_gpu.py: around ONE item of a point, the oracle's winner, in a view that is no
base view of the point.  A list of L < 25 taps: cells 0 .. L - 2 of the patch and its centre cell (24), which keeps its
confidence; its last tap, the seeded one, is the centre cell.  The cells behind a list point almost along the item's direction:
one of them read as a tap would win.  Rewriting views can make another item the winner: every case is asserted on the final
maps against the final winner (build() says how the pair of equal loss follows it), on a numpy restatement of the fp32 arithmetic (unit vectors as
torch.cosine_similarity makes them, two rounded products, their rounded sum, fl(1 - |cs|))."""
import numpy as np
import pytest

import oracle
from test_key_block_gpu import P, forward_all, winning_blocks, write
from test_key_seed_gpu import rot
from test_search_leftover_gpu import leftover, show_only
from test_search_leftover_gpu import spread as views_spread
from test_search_staging_gpu import THR, Scene

gpu = pytest.mark.gpu
CENTRE = P // 2
F = np.float32


# ---------------------------------------------------------------------------------------------------------------------------
# the fp32 arithmetic of a tap, restated
# ---------------------------------------------------------------------------------------------------------------------------
def unit32(x):
    """x / max(|x|, 1e-8) in fp32, the norm's square as one rounded product and one fused multiply-add; a NaN norm stays NaN"""
    x = np.asarray(x, F)
    with np.errstate(all="ignore"):
        s = (x[..., 0] * x[..., 0]).astype(F)
        s = (x[..., 1].astype(np.float64) * x[..., 1].astype(np.float64) + s.astype(np.float64)).astype(F)
        nrm = np.sqrt(s).astype(F)
        nrm = np.where(nrm < F(1e-8), F(1e-8), nrm)
        return (x / nrm[..., None]).astype(F)


def cs32(taps, d):
    """fl(fl(tx * dx) + fl(ty * dy)) of unit taps [T, 2] and a unit direction d"""
    with np.errstate(all="ignore"):
        return ((taps[:, 0] * d[0]).astype(F) + (taps[:, 1] * d[1]).astype(F)).astype(F)


def loss32(cs):
    return (F(1.0) - np.abs(cs)).astype(F)


def first_min(loss):
    """index of the first-index minimum, NaN never smaller (the strict '<' of the reference; tap 0 is never NaN here)"""
    best = 0
    for t in range(1, len(loss)):
        if loss[t] < loss[best]:
            best = t
    return best


def winners32(sc, offsets):
    """per point: the oracle's winner (rank, sample), the projected directions [V, S, 2] of that rank's samples as fp32, the base views"""
    views = sc.views()
    o = oracle.visible_and_ori(views, sc.pts, sc.patch)
    bidx, _ = oracle.topk_views(o["visible"], o["Conf"], 20)
    ex = oracle.forward(views, sc.pts, sc.patch, THR, offsets, extra=True)[4]
    out = []
    for n in range(len(sc.pts)):
        r, s = int(ex["best_rank"][n]), int(ex["best_s"][n])
        D = oracle.reproject_ori(views, sc.pts, oracle.sample_next(views, sc.pts, bidx[2 * r], o["Ori"], offsets))[:, n]
        out.append(dict(r=r, s=s, D=np.ascontiguousarray(D, F), base=set(int(b) for b in bidx[0:20:2, n])))
    return out, o


# ---------------------------------------------------------------------------------------------------------------------------
# the cases: make(d, d32, L) -> the L orientations of the list's taps, in tap order (d: the item's unit direction, float64;
# d32: as the kernel has it)
# ---------------------------------------------------------------------------------------------------------------------------
def cells(L):
    """the patch cells of a list of L taps, in tap order"""
    return list(range(P)) if L == P else list(range(L - 1)) + [CENTRE]


def off_taps(d, L, a0=0.3, step=0.01):
    """L distinct orientations a0 .. a0 + 49 * step rad off d, in a scrambled order"""
    return [rot(d, a0 + step * ((k * 37) % P)) for k in range(L)]


def neg(t):
    def make(d, d32, L):
        oris = off_taps(d, L)
        oris[t] = -np.asarray(d)
        return oris
    return make


def along(t):
    def make(d, d32, L):
        oris = off_taps(d, L, a0=1.35, step=0.008)      # the other taps near the perpendicular: an item off d loses in this view
        oris[t] = np.asarray(d)
        return oris
    return make


def tie(t1, t2):
    def make(d, d32, L):
        oris = off_taps(d, L)
        first = rot(d, 0.05).astype(F)          # (not along d itself: the cosines of the two are then no +-1 of a clamp)
        oris[t1], oris[t2] = first, -first
        return oris
    return make


def equal_loss_pair(d, d32, side=1):
    """two orientations about 1.16 rad off d (to the left or to the right of it) whose fp32 cs against d32 differ while
    fl(1 - |cs|) is the same float: (larger |cs|, smaller |cs|)"""
    ang = side * (1.159 + 2e-8 * np.arange(4000))
    o = np.stack([d[0] * np.cos(ang) - d[1] * np.sin(ang), d[0] * np.sin(ang) + d[1] * np.cos(ang)], axis=1).astype(F)   # rot(d, ang)
    c = cs32(unit32(o), d32)
    loss = loss32(c)
    seen = {}
    for k in range(len(ang)):
        if not 0.25 <= abs(c[k]) < 0.5:
            continue
        k2 = seen.setdefault(loss[k].tobytes(), k)
        if abs(c[k2]) != abs(c[k]) and np.sign(c[k2]) == np.sign(c[k]):
            return (o[k2], o[k]) if abs(c[k2]) > abs(c[k]) else (o[k], o[k2])
    raise AssertionError("no two orientations of equal loss and different cosine")


def equal_loss(t1, t2, larger_first, side=1):
    def make(d, d32, L):
        oris = off_taps(d, L, a0=1.35, step=0.008)      # |cos| <= 0.22 for every other tap
        hi, lo = equal_loss_pair(d, d32, side)
        oris[t1], oris[t2] = (hi, lo) if larger_first else (lo, hi)
        return oris
    return make


NANS = [np.array([np.nan, np.nan]), np.array([np.inf, 1.0]), np.array([1.0, np.inf]), np.array([np.inf, -1.0])]   # unit vectors
#        (NaN, NaN),                  (NaN, 0),                (0, NaN),                (NaN, -0): four different records


def nan_beside(t, tn):
    def make(d, d32, L):
        oris = off_taps(d, L)
        oris[t] = np.asarray(d)
        for i, k in enumerate(tn):
            oris[k] = NANS[i]
        return oris
    return make


def bad(nan_at, zero_at):
    """every tap within 2^-14 of perpendicular to d, but a NaN one and a (0, 0) one"""
    def make(d, d32, L):
        perp = np.array([-d[1], d[0]])
        oris = [rot(perp, (k - L // 2) * 2e-6) for k in range(L)]
        oris[nan_at] = NANS[0]
        oris[zero_at] = np.zeros(2)
        return oris
    return make


def place(sc, v, n, make, L, w, exact=None, c0=0.5):
    """w: the item the patch is laid out around; exact: the item whose fp32 direction a case that needs one is made for; c0: the
    confidence of tap 0, every tap 0.001 above the one before"""
    exact = exact or w
    d32 = unit32(exact["D"][v, exact["s"]])
    d = w["D"][v, w["s"]].astype(np.float64)
    d /= np.linalg.norm(d)
    oris = [rot(d, 1e-3 * (k + 1)) for k in range(P)]           # the cells behind the list: almost along d
    for k, o in zip(cells(L), make(d, d32, L)):
        oris[k] = o
    write(sc, v, n, oris, [c0 + 0.001 * k for k in range(P)], P if L == P else L - 1)


def check(kind, args, L, op, cp, D):
    """the case on the final maps: op [P, 2], cp [P] the patch of its view, D the final winner's direction in that view"""
    el = cp > THR
    el[0] = True
    assert list(np.nonzero(el)[0]) == cells(L), (kind, args, L)
    taps = unit32(op[el])
    assert len(set(t.tobytes() for t in taps)) == L                 # no duplicates: the list has L taps
    d32 = unit32(D)
    cs = cs32(taps, d32)
    with np.errstate(all="ignore"):
        loss = loss32(cs)
        ac = np.abs(cs)
    others = np.delete(ac, [t for t in args if type(t) is int] + [k for t in args if type(t) is tuple for k in t])
    if kind == "along":
        (t,) = args
        assert cs[t] > 0.99 and first_min(loss) == t and ac[t] > others.max() + 0.01
    elif kind == "neg":
        (t,) = args
        assert cs[t] < -0.99 and first_min(loss) == t and ac[t] > others.max() + 0.01
        assert winning_blocks(d32[None].astype(np.float64), taps)[0] == t // 4
    elif kind == "tie":
        t1, t2 = args
        assert t1 < t2 and cs[t1] == -cs[t2] and loss[t1] == loss[t2] and first_min(loss) == t1 and ac[t1] > others.max() + 0.01
    elif kind == "eq":
        t1, t2, larger_first = args[:3]
        assert t1 < t2 and cs[t1] != cs[t2] and ac[t1] != ac[t2] and (ac[t1] > ac[t2]) == larger_first
        assert loss[t1] == loss[t2] and first_min(loss) == t1
        assert min(ac[t1], ac[t2]) > np.delete(ac, [t1, t2]).max() + 0.01
    elif kind == "nan":
        t, tn = args
        assert np.isnan(cs[list(tn)]).all() and np.isnan(cs).sum() == len(tn) and first_min(loss) == t
        assert ac[t] > np.nanmax(others) + 0.01
        assert all(k // 4 == tn[0] // 4 for k in tn) and (t // 4 == tn[0] // 4) == (len(tn) == 1)
    else:
        raise AssertionError(kind)


MAKERS = dict(neg=neg, along=along, tie=tie, eq=equal_loss, nan=nan_beside)
# A view of equal-loss taps gives the item it is made for a loss of 0.6 and most other items a smaller one: such views weigh little
# (confidences just above the threshold), and views with a tap along the item's direction, of full weight, stand beside them, so
# that the winner stays the item or a neighbour of its rank.
WEIGHT = dict(eq=0.16, along=0.95)


def build(offsets, plan, vis=None):
    """plan[n] = [(kind, args, L)]: the cases of point n, one free view each, laid out around the winners of the scene as it
    stands.  Rewriting its views may make another item the winner (tests/test_key_block_gpu.py: build_cases): every case is
    asserted against the FINAL winner's direction.  The pair of equal loss holds for one fp32 direction only: it is made for the
    winner of the rewritten scene, the scene written again with that pair -- a nudge of two taps by 1e-4 rad at the most --
    until the winner is the item the pairs were made for."""
    exact = None
    for _ in range(6):
        sc = Scene(22, 32, 64, 7, len(plan), min_dist=9)
        for n, k in enumerate(vis or ()):
            show_only(sc, n, views_spread(22, n, k))
        first, o0 = winners32(sc, offsets)
        made_for = exact or first
        placed = []
        for n, todo in enumerate(plan):
            free = [v for v in range(sc.V) if v not in first[n]["base"] and o0["visible"][v, n] != -1.0]
            assert len(free) >= len(todo), (n, len(free), len(todo))
            for v, (kind, args, L) in zip(free, todo):
                place(sc, v, n, MAKERS[kind](*args), L, first[n], made_for[n], c0=WEIGHT.get(kind, 0.5))
                placed.append((v, n, kind, args, L))
        after, o = winners32(sc, offsets)
        if [(w["r"], w["s"]) for w in after] == [(w["r"], w["s"]) for w in made_for]:
            break
        exact = after
    else:
        raise AssertionError("the winners do not settle")
    for v, n, kind, args, L in placed:
        w = after[n]
        assert v not in w["base"] and w["base"] == first[n]["base"] and o["visible"][v, n] != -1.0
        check(kind, args, L, o["Ori_patch"][v, n], o["Conf_patch"][v, n].copy(), w["D"][v, w["s"]])
    return sc, {(v, n): L for v, n, kind, args, L in placed}


# A tap t lies in block t // 4, place t % 4; a list of c taps seeds tap c - 1 and walks the c - 1 in front of it, padded to
# whole blocks: 49 -> 12 blocks; 13 -> 3 blocks; 14, 15, 16 -> 4 blocks with 3, 2, 1 taps in the last (the seed read again in it
# for 14 and 15).
NEG49 = [("neg", (t,), 49) for b in (0, 5, 11) for t in range(4 * b, 4 * b + 4)]
NEG_SHORT = [("neg", (9,), 13), ("neg", (12,), 14), ("neg", (13,), 15), ("neg", (14,), 16), ("neg", (15,), 16), ("neg", (2,), 14)]
SIGN_TIES = [("tie", (20, 21), 49), ("tie", (20, 23), 49), ("tie", (22, 23), 49), ("tie", (9, 30), 49), ("tie", (4, 12), 14),
             ("tie", (44, 48), 49)]
NAN_FOLD = [("nan", (21, (20,)), 49), ("nan", (20, (21,)), 49), ("nan", (20, (22,)), 49), ("nan", (20, (23,)), 49),
            ("nan", (30, (20, 21, 22, 23)), 49), ("nan", (3, (44, 45, 46, 47)), 49), ("nan", (12, (13,)), 16),
            ("nan", (1, (8, 9, 10, 11)), 15)]
EQUAL = [("eq", (20, 22, True, 1), 49), ("eq", (20, 22, False, -1), 49), ("eq", (9, 30, True, -1), 49), ("eq", (9, 30, False, 1), 49),
         ("eq", (21, 23, False, 1), 49), ("eq", (12, 13, False, -1), 16), ("eq", (8, 13, False, 1), 14), ("eq", (2, 12, True, -1), 13)]

_cache = {}


def cached(fn):
    def get(offsets):
        if fn.__name__ not in _cache:
            _cache[fn.__name__] = fn(offsets)
        return _cache[fn.__name__]
    return get


@cached
def sign_scene(offsets):
    return build(offsets, [NEG49, NEG_SHORT + SIGN_TIES])


@cached
def nan_scene(offsets):
    return build(offsets, [NAN_FOLD])


@cached
def equal_scene(offsets):
    beside = [("along", (t,), 49) for t in (5, 17, 30, 48, 0, 23, 41, 12)]
    return build(offsets, [EQUAL[:4] + beside])


@cached
def equal_scene_short(offsets):
    """the same in the last blocks of lists of 16, 14 and 13 taps (the second tap of the pair the seeded one in the last two)"""
    beside = [("along", (t,), 49) for t in (5, 17, 30, 48, 0, 23, 41, 12)]
    return build(offsets, [EQUAL[4:] + beside])


@cached
def one_rank_scene(offsets):
    """point 0: all 22 views (10 x 90 items); point 1: two views, 1 x 90 items -- its one free view holds a negative winner in
    the last place of the last walked block"""
    return build(offsets, [[("neg", (45,), 49), ("tie", (0, 47), 49)], [("neg", (47,), 49)]], vis=(22, 2))


@cached
def bad_scene(offsets):
    """lists of 49, 16 and 14 taps, every tap perpendicular to the item they are built around within 2^-14, NaN or (0, 0);
    asserted against that item (its wave enters the re-evaluation), as tests/test_key_block_gpu.py does for its fans"""
    plan = [[(bad(30, 5), 49), (bad(13, 12), 16)], [(bad(3, 11), 14), (bad(47, 44), 49)]]
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
        assert len(set(t.tobytes() for t in taps)) == L
        cs = cs32(taps, unit32(win[n]["D"][v, win[n]["s"]]))    # (the samples of a rank do not depend on views that are no base views)
        assert np.isnan(cs).sum() == 1 and (taps == 0).all(axis=1).sum() == 1
        assert np.nanmax(np.abs(cs)) < 2.0 ** -14
    return sc, {(v, n): L for v, n, L in placed}


def test_the_constructions_hold(depth_offsets):
    """the CPU half: every scene builds (build() asserts each case on the final maps, on the numpy restatement), the oracle's
    losses are finite, every list length 13, 14, 15, 16 and 49 occurs, and the pair of equal loss is what it is meant to be"""
    lengths = set()
    for make in (sign_scene, nan_scene, equal_scene, equal_scene_short, one_rank_scene, bad_scene):
        sc, expect = make(depth_offsets)
        assert np.isfinite(oracle.forward(sc.views(), sc.pts, sc.patch, THR, depth_offsets)[2]).all()
        lengths |= set(expect.values())
    assert lengths == {13, 14, 15, 16, 49}
    assert [leftover(k) for k in (22, 2)] == [(4, True), (26, False)]
    # different cs, equal loss, for a direction of its own
    d = np.array([np.cos(0.7), np.sin(0.7)])
    d32 = unit32(d.astype(F))
    hi, lo = equal_loss_pair(d, d32)
    c = cs32(unit32(np.stack([hi, lo])), d32)
    assert c[0] != c[1] and abs(c[0]) > abs(c[1]) and 0.25 <= abs(c[1]) and abs(c[0]) < 0.5
    assert loss32(c)[0] == loss32(c)[1]
    # fl(C - x) is monotone: the minimum of the t' is the t' of the maximum, on the pair and on a block's worth of values
    C = F(1.00006103515625)
    x = np.abs(np.concatenate([c, cs32(unit32(np.array(off_taps(d, 6), F)), d32)]))
    assert (C - x).astype(F).min() == (C - x.max()).astype(F)


@gpu
def test_negative_cosines_and_sign_ties(depth_offsets):
    sc, expect = sign_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_nan_taps_in_the_fold(depth_offsets):
    sc, expect = nan_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_different_cosines_of_equal_loss(depth_offsets):
    sc, expect = equal_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_different_cosines_of_equal_loss_in_short_lists(depth_offsets):
    sc, expect = equal_scene_short(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_one_rank_of_90_items(depth_offsets):
    sc, expect = one_rank_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert [(cnt[:, n] > 0).sum() for n in range(2)] == [22, 2]
    assert all(st[2] == 0 for st in stats.values()), stats


@gpu
def test_lists_of_perpendicular_nan_and_zero_taps_take_the_bad_key_route(depth_offsets):
    sc, expect = bad_scene(depth_offsets)
    cnt, stats = forward_all(sc, depth_offsets, expect)
    assert stats[(0, 0)][2] > 0 and stats[(1, 0)][2] > 0, "the key body's re-evaluation branch was not entered"
    assert stats[(2, 0)][2] == 0 and stats[(0, 1256)][2] == 0       # (the select body and the portable kernel build no keys)
