"""GPU: the key body's list walk (csrc/pmvo_search.hip: mh_key_walked) -- the blocks of four taps cover the taps in front of
a list's last tap, the last tap seeds the accumulator of its parity.  Hand-built patches whose lists have every length mod 4 on
both sides of MH_KEY_MIN_TAPS (= 10: shorter lists take the select body) and up to the complete 7 x 7 patch, a 9 x 9 scene whose
lists cross the 64-tap group border (that instantiation keeps its padded walk), a seeded list that enters the re-evaluation
branch (asserted on mh_debug_key_stats, as tests/test_key_reeval_gpu.py does), a list whose winner IS the seeded last tap, and a
list whose last tap ties in loss with an earlier one (the earlier one must win: PMVO.py:177 replaces on a strictly smaller loss
only).  Every output of every body is compared with oracle.forward, bit for bit.

How a list length is set: a tap p >= 1 is eligible iff its confidence is above the threshold (PMVO.py:162,177-182; tap 0 always
is), and taps with bit-identical unit orientations are dropped as duplicates -- so the first c cells of a patch, in tap order, get
distinct orientations and confidence 0.9, the others confidence 0.05.  A tie in loss between two taps that are NOT duplicates: the
same orientation with the opposite sign (|cos| is the same bits, the unit vectors are not)."""
import ctypes

import numpy as np
import pytest
import torch

import oracle

gpu = pytest.mark.gpu
DEV = "cuda:0"
THR = 0.15
S_REF = 45                                                   # the candidate sample whose direction the patches are built around


def key_stats(pm, reset=True):
    out = (ctypes.c_ulonglong * 4)()
    torch.cuda.synchronize()
    assert pm._L.mh_debug_key_stats(out, 1 if reset else 0) == 0
    return [int(x) for x in out]


def build(patch, V=24, H=240, W=160, seed=5):
    from monohair_amd import synth
    from monohair_amd.camera import camera_records, cameras_from_list

    scene = synth.make_scene(V, H, W, seed=seed, quantize=False, rings=2)
    cams = cameras_from_list(scene["cams"])
    rec = camera_records(cams)
    pts = synth.candidate_points(res=48, seed=seed, limit=300).astype(np.float32)
    maps = {k: scene[k].cpu().numpy().copy() for k in ("depth", "ori", "conf", "mask")}
    return rec, cams, pts, maps, (V, H, W)


def views_of(rec, m):
    return oracle.Views(rec, m["depth"], m["ori"], m["conf"], m["mask"])


def rot(d, a):
    return np.array([d[0] * np.cos(a) - d[1] * np.sin(a), d[0] * np.sin(a) + d[1] * np.cos(a)])


def usable_pairs(rec, maps, pts, patch, offsets, H, W):
    """(n, v, r, c, d): pairs whose view sees the point and is none of its base views, the patch inside the image and apart
    from the patches handed out before in that view; d = unit direction (row, col) of sample S_REF of rank 0 in that view."""
    views = views_of(rec, maps)
    o = oracle.visible_and_ori(views, pts, patch)
    bidx, bval = oracle.topk_views(o["visible"], o["Conf"], 20)
    used = bidx[0:20:2]
    D = oracle.reproject_ori(views, pts, oracle.sample_next(views, pts, bidx[0], o["Ori"], offsets))
    hp = patch // 2
    taken = []
    for n in range(len(pts)):
        for v in range(views.V):
            if o["visible"][v, n] == -1.0 or v in used[:, n] or bval[0, n] <= 0:
                continue
            rc, _, oob, _ = oracle.project_points(views.cams[v], pts[n:n + 1], H, W)
            r, c = int(rc[0, 0]), int(rc[0, 1])
            if oob[0] or not (hp <= r < H - hp and hp <= c < W - hp):
                continue
            if any(n == n2 or (v == v2 and abs(r - r2) <= 2 * patch and abs(c - c2) <= 2 * patch) for n2, v2, r2, c2 in taken):
                continue
            d = D[v, n, S_REF].astype(np.float64)
            if not np.all(np.isfinite(d)) or np.hypot(*d) < 1e-3:
                continue
            taken.append((n, v, r, c))
            yield n, v, r, c, d / np.hypot(*d)


def write_patch(maps, v, r, c, patch, oris, confs):
    hp, k = patch // 2, 0
    for i in range(-hp, hp + 1):
        for j in range(-hp, hp + 1):
            maps["ori"][v, r + i, c + j] = np.asarray(oris[k], np.float32)
            maps["conf"][v, r + i, c + j] = confs[k]
            k += 1


def spread(d, P, count, a0=0.3, step=0.01):
    """P orientations 0.3 .. 1.1 rad off d in a scrambled order (distinct losses, no duplicates); the first `count` eligible.  The
    ineligible cells point almost along d: one of them read as a tap would win."""
    oris = [rot(d, a0 + step * ((k * 37) % P)) for k in range(P)]
    for k in range(count, P):
        oris[k] = rot(d, 1e-3 * (k + 1))
    confs = [0.9 if k < count else 0.05 for k in range(P)]
    return oris, confs


def list_length(o, v, n):
    """the length the front end gives the list of (v, n): eligible taps minus later bit-identical unit orientations"""
    cp, op = o["Conf_patch"][v, n], o["Ori_patch"][v, n]
    el = np.ones(len(cp), bool) if not (cp.max() > THR) else (cp > THR)
    el[0] = True
    unit = (op / np.hypot(op[:, 0], op[:, 1])[:, None]).astype(np.float32)
    seen, c = set(), 0
    for p in np.nonzero(el)[0]:
        b = unit[p].tobytes()
        c += b not in seen
        seen.add(b)
    return c


def run_and_compare(rec, cams, pts, maps, patch, offsets, expect, bodies=(0, 1, 2), want_reeval=None):
    """forward() with the default, the key and the select body against oracle.forward; expect = {(v, n): list length}"""
    from monohair_amd.pmvo import PMVO

    views = views_of(rec, maps)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)       # noqa: E731
    pm = PMVO.from_planes(rec, t(maps["depth"]), t(maps["ori"]), t(maps["conf"]), t(maps["mask"]), device=DEV,
                          patch_size=patch, visible_threshold=1, conf_threshold=THR, camera=cams)
    _, o_ori, o_loss, o_hc, o_ex = oracle.forward(views, pts, patch, THR, offsets, extra=True)
    ref = (o_ori, o_loss, o_hc, o_ex["best_s"], o_ex["best_rank"])
    key_stats(pm)                                                    # reset
    try:
        for body in bodies:
            pm.set_option("search_body", body)
            _, ori, loss, hc, ex = pm.forward(pts, extras=True)
            st = key_stats(pm)
            cnt = pm.search_work(len(pts))[0]
            for (v, n), c in expect.items():
                assert cnt[v, n].item() == c, (v, n, c)
            if want_reeval is not None and body != 2:
                assert (st[2] > 0) == want_reeval, st
            got = tuple(x.cpu().numpy() for x in (ori, loss, hc, ex["best_s"], ex["best_rank"]))
            for a, b in zip(got, ref):
                assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), body
    finally:
        pm.set_option("search_body", 0)
    return o_loss


def scene_with_lengths(patch, lengths, offsets):
    """one scene, one hand-built patch per wanted list length; returns what run_and_compare needs + {(v, n): length}"""
    rec, cams, pts, maps, (V, H, W) = build(patch)
    P = patch * patch
    todo, placed = list(lengths), []
    for n, v, r, c, d in usable_pairs(rec, maps, pts, patch, offsets, H, W):
        if not todo:
            break
        count = todo.pop(0)
        write_patch(maps, v, r, c, patch, *spread(d, P, count))
        placed.append((v, n, count))
    assert not todo, "the scene has too few usable (point, view) pairs"
    o = oracle.visible_and_ori(views_of(rec, maps), pts, patch)     # on the FINAL maps: the lists are as long as wanted
    expect = {}
    for v, n, count in placed:
        assert o["visible"][v, n] != -1.0 and list_length(o, v, n) == count, (v, n, count)
        expect[(v, n)] = count
    return rec, cams, pts, maps, expect


LENGTHS7 = [9, 10, 11, 12, 13, 14, 15, 45, 46, 47, 48, 49]          # MH_KEY_MIN_TAPS = 10: 9 and 10 take the select body
LENGTHS9 = [61, 62, 63, 64, 65, 66, 67, 68, 69, 80, 81]             # both sides of the 64-tap group border, every length mod 4


def test_oracle_accepts_the_constructions(depth_offsets):
    """the CPU half: the inputs hold what they are built for (list lengths) and the oracle evaluates them to finite losses"""
    for patch, lengths in ((7, LENGTHS7), (9, LENGTHS9)):
        rec, cams, pts, maps, expect = scene_with_lengths(patch, lengths, depth_offsets)
        assert sorted(expect.values()) == sorted(lengths)
        _, _, loss, _ = oracle.forward(views_of(rec, maps), pts, patch, THR, depth_offsets)
        for (v, n) in expect:
            assert np.isfinite(loss[n])


@gpu
def test_every_list_length_mod_4_patch7(depth_offsets):
    rec, cams, pts, maps, expect = scene_with_lengths(7, LENGTHS7, depth_offsets)
    run_and_compare(rec, cams, pts, maps, 7, depth_offsets, expect)


@gpu
def test_lists_across_the_64_tap_group_patch9(depth_offsets):
    rec, cams, pts, maps, expect = scene_with_lengths(9, LENGTHS9, depth_offsets)
    run_and_compare(rec, cams, pts, maps, 9, depth_offsets, expect)


def special_scene(offsets, count, make):
    """one hand-built 7 x 7 patch; make(d, P, count) -> (oris, confs).  Returns the scene, the pair, and the final maps' float64
    |cos| of every tap of that pair against the direction of sample S_REF (rank 0), with the taps' eligibility."""
    patch, P = 7, 49
    rec, cams, pts, maps, (V, H, W) = build(patch)
    n, v, r, c, d = next(usable_pairs(rec, maps, pts, patch, offsets, H, W))
    write_patch(maps, v, r, c, patch, *make(d, P, count))
    views = views_of(rec, maps)
    o = oracle.visible_and_ori(views, pts, patch)
    assert o["visible"][v, n] != -1.0 and list_length(o, v, n) == count
    bidx, _ = oracle.topk_views(o["visible"], o["Conf"], 20)
    D = oracle.reproject_ori(views, pts, oracle.sample_next(views, pts, bidx[0], o["Ori"], offsets))
    dh = D[v, n, S_REF].astype(np.float64)
    dh /= np.linalg.norm(dh)
    taps = o["Ori_patch"][v, n].astype(np.float64)
    taps /= np.linalg.norm(taps, axis=1, keepdims=True)
    return (rec, cams, pts, maps), (v, n), np.abs(taps @ dh), o


def reeval_scene(count, offsets):
    """all taps within 2^-14 of perpendicular to one candidate's direction: the key cannot state the winner"""
    def make(d, P, count):
        perp = np.array([-d[1], d[0]])
        return [rot(perp, (k - P // 2) * 2e-6) for k in range(P)], [0.9 if k < count else 0.05 for k in range(P)]

    scene, pair, ac, o = special_scene(offsets, count, make)
    assert ac[:count].max() < 2.0 ** -14
    return scene, pair


def last_wins_scene(count, offsets):
    """the list's last tap lies along the candidate's direction, every other tap at least 0.3 rad off"""
    def make(d, P, count):
        oris, confs = spread(d, P, count)
        oris[count - 1] = d
        confs[count - 1] = 0.6
        return oris, confs

    scene, pair, ac, o = special_scene(offsets, count, make)
    assert np.argmax(ac[:count]) == count - 1 and ac[count - 1] > 0.9999 and ac[:count - 1].max() < 0.96
    return scene, pair


def tie_scene(count, offsets):
    """tap count // 2 lies along the candidate's direction (confidence 0.9), the last tap is the same orientation with the
    opposite sign (confidence 0.5): equal |cos| bit for bit, not duplicates; the earlier tap's confidence must be the weight"""
    def make(d, P, count):
        oris, confs = spread(d, P, count)
        first = np.asarray(d, np.float32)
        oris[count // 2] = first
        oris[count - 1] = -first
        confs[count - 1] = 0.5
        return oris, confs

    scene, (v, n), ac, o = special_scene(offsets, count, make)
    op = o["Ori_patch"][v, n]
    assert np.array_equal(op[count - 1], -op[count // 2]) and ac[count // 2] == ac[count - 1] > 0.9999
    assert np.delete(ac[:count], [count // 2, count - 1]).max() < 0.96
    return scene, (v, n)


REEVAL = [49, 47, 46, 13]
LAST_WINS = [49, 45, 13, 47, 46, 48]
TIES = [49, 46, 13]


def test_oracle_accepts_the_special_constructions(depth_offsets):
    """the CPU half of the three tests below: every construction holds on its final maps, the oracle gives a finite loss"""
    for make, counts in ((reeval_scene, REEVAL), (last_wins_scene, LAST_WINS), (tie_scene, TIES)):
        for count in counts:
            (rec, cams, pts, maps), (v, n) = make(count, depth_offsets)
            _, _, loss, _ = oracle.forward(views_of(rec, maps), pts, 7, THR, depth_offsets)
            assert np.isfinite(loss[n]), (make.__name__, count)


@gpu
@pytest.mark.parametrize("count", REEVAL)
def test_seeded_list_enters_the_reevaluation_branch(count, depth_offsets):
    scene, pair = reeval_scene(count, depth_offsets)
    run_and_compare(*scene, 7, depth_offsets, {pair: count}, want_reeval=True)


@gpu
@pytest.mark.parametrize("count", LAST_WINS)
def test_the_seeded_last_tap_wins(count, depth_offsets):
    scene, pair = last_wins_scene(count, depth_offsets)
    run_and_compare(*scene, 7, depth_offsets, {pair: count})


@gpu
@pytest.mark.parametrize("count", TIES)
def test_last_tap_ties_with_an_earlier_tap(count, depth_offsets):
    scene, pair = tie_scene(count, depth_offsets)
    run_and_compare(*scene, 7, depth_offsets, {pair: count})
