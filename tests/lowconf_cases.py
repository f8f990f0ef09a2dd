"""Shared by tools/gen_golden_lowconf.py and tests/test_lowconf_*.py: the hand-edited patches behind tests/golden/pmvo_lowconf.npz.
The search's low-confidence rule, `low_conf_index = lt(sum(positive_index), 5)` (PMVO.py:198-206), on both sides of its bound: a
point with fewer than 5 positive samples takes the smallest raw loss of all its samples, one with 5 or more the smallest loss of
its positive samples; the flag of the winner decides whether `optimize` keeps the row.

The scene is that of tests/test_key_seed_gpu.py (24 views of 240 x 160, fp32 planes, conf_threshold 0.15).  A case owns one
point n and one view v that sees the point and is none of its base views.  Over the samples s = 0 .. S - 1 of rank 0 the
projected direction D[v, n, s] turns monotonically through less than pi / 2 (theta[s], unwrapped).  The patch of v at the point's
pixel is written so that the confidence of its winning tap steps once along the sweep:

  * tap 0 (the top-left cell, which seeds the running minimum whatever its confidence, PMVO.py:173-175) and the centre cell (which
    the base-view ranking reads) get the low confidence C_LOW; tap 0 gets the orientation `alpha`;
  * the other cells get C_HIGH and the orientation `beta`, 0.2 rad outside the end of the sweep the positive samples start from
    (patch 7: one beta cell, the others distinct orientations further away from every sample than alpha or beta is);
  * the bisector of alpha and beta lies half-way between theta[k - 1] and theta[k]: on k samples a C_HIGH tap has the smaller
    loss, on the others tap 0 keeps the minimum.  k = 0: the bisector lies in front of the sweep; k = S: tap 0 is C_HIGH as well.

The other views that see the point, the rank-0 base view excepted, get one low confidence on their whole patch, chosen per case so
that `sum(weight) / sum(weight > 0)` is at least MARGIN below conf_threshold where tap 0 wins and as much above it where a
C_HIGH tap does.  `far` cases count the positive samples from s = S - 1 down.  verify() asserts all of it on the final maps.

numpy and the CPU oracle's projection only; nothing from the GPU side."""
import numpy as np

import oracle
import softmask_cases as sc

F = np.float32
V, H, W = 24, 240, 160
SEED, RES, LIMIT = 5, 48, 300
THR = 0.15
C_HIGH, C_LOW = 0.9, 0.01
MARGIN = 0.01                # every sample's ratio is at least this far from THR
ANGLE_MARGIN = 1e-3          # no D within this angle of a bisector (= 2e-3 between the two taps' angular distances)
MIN_LENGTH = 1e-3            # no projected length (pixels) below this
OFF_END = 0.2                # beta lies this far outside the sweep
MAX_SWEEP = np.pi / 2 - 0.15
RESERVE = 8                  # centres of two case points in one view are more than this many pixels apart (rows or columns)
TINY = 1e-6                  # the tiny positive base_val of the `tiny` ranking

# name, patch, S, k (wanted positive samples on rank 0), end the positive samples start from
CASES = (("k0", 3, 90, 0, "near"), ("k1", 3, 90, 1, "near"), ("k4", 3, 90, 4, "near"), ("k5", 3, 90, 5, "near"),
         ("k6", 3, 90, 6, "near"), ("k90", 3, 90, 90, "near"), ("far4", 3, 90, 4, "far"), ("far5", 3, 90, 5, "far"),
         ("p7k4", 7, 90, 4, "near"), ("p7k5", 7, 90, 5, "near"), ("s4all", 3, 4, 4, "near"), ("s5all", 3, 5, 5, "near"),
         ("s5k4", 3, 5, 4, "near"))
NAMES = tuple(c[0] for c in CASES)
RUNS = ((3, 90), (3, 4), (3, 5), (7, 90))          # (patch, S) of the forward calls; the cases of a run are those it was tuned for
RANKINGS = ("rep", "zero", "tiny")                 # base-view rankings handed to forward(), patch 3, S = 90 (rankings())


def offsets(S):
    from monohair_amd.pmvo import depth_offsets

    return depth_offsets(S)


def scene():
    """-> (camera list, maps of the unedited scene, candidate points)"""
    from monohair_amd import synth

    s = synth.make_scene(V, H, W, seed=SEED, quantize=False, rings=2)
    maps = {k: s[k].cpu().numpy().copy() for k in ("depth", "ori", "conf", "mask")}
    return s["cams"], maps, synth.candidate_points(res=RES, seed=SEED, limit=LIMIT).astype(F)


def views_of(rec, m):
    return oracle.Views(rec, m["depth"], m["ori"], m["conf"], m["mask"])


def rank0(views, pts, S, patch=3):
    """-> (visible_and_ori dict, base_idx, base_val [20,N], D [V,N,S,2] of rank 0)"""
    o = oracle.visible_and_ori(views, pts, patch)
    bidx, bval = oracle.topk_views(o["visible"], o["Conf"], 20)
    D = oracle.reproject_ori(views, pts, oracle.sample_next(views, pts, bidx[0], o["Ori"], offsets(S)))
    return o, bidx, bval, D


def angle(x):
    return np.arctan2(x[..., 1].astype(np.float64), x[..., 0].astype(np.float64))


def unit(a):
    return np.array([np.cos(a), np.sin(a)])


def line_dist(a, b):
    """angle between two sign-less directions, in [0, pi / 2]"""
    d = np.abs(np.asarray(a) - np.asarray(b)) % np.pi
    return np.minimum(d, np.pi - d)


def sweep(D_vn):
    """unwrapped angles of D[v, n, :] if they turn monotonically through less than MAX_SWEEP, every step above 4 *
    ANGLE_MARGIN and every length above MIN_LENGTH; else None"""
    if not np.all(np.isfinite(D_vn)) or np.hypot(D_vn[:, 0], D_vn[:, 1]).min() < MIN_LENGTH:
        return None
    th = np.unwrap(angle(D_vn))
    d = np.diff(th)
    if len(d) and not (np.all(d > 4 * ANGLE_MARGIN) or np.all(d < -4 * ANGLE_MARGIN)):
        return None
    return th if abs(th[-1] - th[0]) < MAX_SWEEP else None


def tuned_patch(th, patch, k, end):
    """-> (oris [P,2], confs [P]) of the tuned view's patch for k positive samples counted from `end` of the sweep th [S]"""
    P, S = patch * patch, len(th)
    t = th if end == "near" else th[::-1]
    sgn = 1.0 if t[-1] >= t[0] else -1.0
    beta = t[0] - sgn * OFF_END
    if k == 0:
        bis = t[0] - sgn * OFF_END / 4
    elif k == S:
        bis = (t[0] + t[-1]) / 2
    else:
        bis = (t[k - 1] + t[k]) / 2
    alpha = 2 * bis - beta
    oris, confs = [unit(beta)] * P, [C_HIGH] * P
    oris[0], confs[0] = unit(alpha), C_HIGH if k == S else C_LOW
    confs[P // 2] = C_LOW
    if P > 9:
        # one beta cell (the last); the others: distinct orientations, 0.3 rad and more off the sweep, each further from every
        # sample than the nearer of alpha and beta is -- the winning tap of a sample stays the one of the 3 x 3 construction
        need = np.minimum(line_dist(t, alpha), line_dist(t, beta))
        cand = [a for a in t[-1] + sgn * np.arange(0.3, np.pi - abs(t[-1] - t[0]) - 0.3, 0.004)
                if np.all(line_dist(t, a) > need + 4 * ANGLE_MARGIN)]
        assert len(cand) >= P - 3, "too few orientations off the sweep: %d" % len(cand)
        pick = [cand[(j * 37) % (P - 3)] for j in range(P - 3)]        # scrambled, as tests/test_key_seed_gpu.py: spread()
        cells = [p for p in range(1, P - 1) if p != P // 2]
        for p, a in zip(cells, pick):
            oris[p] = unit(a)
    return np.array(oris, F), np.array(confs, F)


def write_patch(maps, v, r, c, patch, oris=None, confs=None):
    hp = patch // 2
    win = (v, slice(r - hp, r + hp + 1), slice(c - hp, c + hp + 1))
    if oris is not None:
        maps["ori"][win] = np.asarray(oris, F).reshape(patch, patch, 2)
    maps["conf"][win] = np.asarray(confs, F).reshape(patch, patch) if np.ndim(confs) else F(confs)


def pixels(rec, p):
    """[V] rows, columns and out-of-bounds flags of one point"""
    res = [oracle.project_points(rec[v], p[None], H, W) for v in range(V)]
    return (np.array([x[0][0, 0] for x in res]), np.array([x[0][0, 1] for x in res]), np.array([bool(x[2][0]) for x in res]))


def point_state(views, p, patch, D_n, thr=THR, low_below=5):
    """the restated rank-0 loss of one point alone on the given views: D_n [V,S,2] -> softmask_cases.prj_loss_np's dict"""
    o = oracle.visible_and_ori(views, p[None], patch)
    return sc.prj_loss_np(D_n[:, None], o["Ori_patch"], o["Conf_patch"], o["visible"], thr, low_below=low_below), o


def build(rec):
    """-> dict(maps, points [13,3] (the case points, in CASES order), rows (their indices among the candidate points), view (the
    tuned view per case), base (the rank-0 base view per case), edits [E,6] int32 (case, view, row, col, side, tuned 1 / 0),
    edit_conf [E] (the low confidence of an untuned edit, C_LOW for a tuned one))"""
    _, maps, cand = scene()
    rec = np.ascontiguousarray(rec, F)
    views0 = views_of(rec, maps)
    o0 = oracle.visible_and_ori(views0, cand, 3)
    see = o0["visible"] != -1.0
    bidx, bval = oracle.topk_views(o0["visible"], o0["Conf"], 20)
    used = bidx[0:20:2]
    D0 = {S: oracle.reproject_ori(views0, cand, oracle.sample_next(views0, cand, bidx[0], o0["Ori"], offsets(S))) for S in (90, 4, 5)}
    order = sorted(range(len(cand)), key=lambda n: (int(see[:, n].sum()), n))       # points seen by few views first
    reserved, rows, tuned, bases, edits, edit_conf = [], [], [], [], [], []

    def free(rr, cc, sees):          # (a view that does not see a point is neither edited for it nor weighted)
        return not any((sees[v] and sees2[v] and abs(rr[v] - r2[v]) <= RESERVE and abs(cc[v] - c2[v]) <= RESERVE)
                       for r2, c2, sees2 in reserved for v in range(V))

    for ci, (name, patch, S, k, end) in enumerate(CASES):
        hp, done = patch // 2, False
        for n in order:
            m = int(see[:, n].sum())
            if n in rows or m < 2 or bval[0, n] <= 0.2:
                continue
            rr, cc, oob = pixels(rec, cand[n])
            inside = [v for v in range(V) if see[v, n] and not (hp <= rr[v] < H - hp and hp <= cc[v] < W - hp)]
            if inside or not free(rr, cc, see[:, n]):
                continue
            b = int(bidx[0, n])
            for v in range(V):
                if not see[v, n] or v in used[:, n]:
                    continue
                th = sweep(D0[S][v, n])
                if th is None:
                    continue
                others = [u for u in range(V) if see[u, n] and u not in (v, b)]
                # the base view's share of the ratio: what the restatement gives with every other seeing view at weight 0
                trial = {key: val.copy() for key, val in maps.items()}
                for u in others + [v]:
                    write_patch(trial, u, rr[u], cc[u], patch, confs=1e-6)
                share = point_state(views_of(rec, trial), cand[n], patch, D0[S][:, n])[0]["ratio"][0] * m
                if share.max() - share.min() > 1e-3:
                    continue
                B = float(share.mean())
                c_other = C_LOW if not others else float(np.clip((THR * m - B - (C_HIGH + C_LOW) / 2) / len(others), 0.004, 0.12))
                trial = {key: val.copy() for key, val in maps.items()}
                write_patch(trial, v, rr[v], cc[v], patch, *tuned_patch(th, patch, k, end))
                for u in others:
                    write_patch(trial, u, rr[u], cc[u], patch, confs=c_other)
                st, _ = point_state(views_of(rec, trial), cand[n], patch, D0[S][:, n])
                want = np.zeros(S, bool)
                want[:k] = True
                want = want if end == "near" else want[::-1]
                if not np.array_equal(st["ratio"][0] > F(THR), want) or np.abs(st["ratio"][0] - F(THR)).min() < MARGIN + 2e-3:
                    continue
                maps = trial
                reserved.append((rr, cc, see[:, n].copy()))
                rows.append(n), tuned.append(v), bases.append(b)
                edits.append((ci, v, rr[v], cc[v], patch, 1)), edit_conf.append(C_LOW)
                for u in others:
                    edits.append((ci, u, rr[u], cc[u], patch, 0)), edit_conf.append(c_other)
                done = True
                break
            if done:
                break
        assert done, "no usable (point, view) pair left for case %s: widen the point search" % name
    out = dict(maps=maps, points=np.ascontiguousarray(cand[rows]), rows=np.array(rows, np.int32), view=np.array(tuned, np.int32),
               base=np.array(bases, np.int32), edits=np.array(edits, np.int32), edit_conf=np.array(edit_conf, F))
    verify(rec, out)
    return out


def case_rows(patch, S):
    return [i for i, c in enumerate(CASES) if (c[1], c[2]) == (patch, S)]


def wanted(ci):
    name, patch, S, k, end = CASES[ci]
    w = np.zeros(S, bool)
    w[:k] = True
    return w if end == "near" else w[::-1]


def verify(rec, case):
    """on the FINAL maps and the batch of the case points: the rank-0 base views are those the patches were tuned for; per run,
    the restated ratio of every sample of the run's cases lies MARGIN off THR on the wanted side; no D of a tuned view within
    ANGLE_MARGIN of a bisector of tap 0 and an eligible tap; no projected length below MIN_LENGTH in a seeing view"""
    views, pts = views_of(np.ascontiguousarray(rec, F), case["maps"]), case["points"]
    for patch, S in RUNS:
        o, bidx, bval, D = rank0(views, pts, S, patch)
        assert np.array_equal(bidx[0], case["base"]) and (bval[0] > 0).all(), "an edit changed a rank-0 base view"
        st = sc.prj_loss_np(D, o["Ori_patch"], o["Conf_patch"], o["visible"], THR)
        for ci in case_rows(patch, S):
            v, want = int(case["view"][ci]), wanted(ci)
            assert o["visible"][v, ci] != -1.0 and v != bidx[0, ci]
            ratio = st["ratio"][ci]
            assert np.array_equal(ratio > F(THR), want) and np.abs(ratio - F(THR)).min() >= MARGIN, (CASES[ci][0], ratio)
            assert int(st["npos"][ci]) == CASES[ci][3]
            seen = o["visible"][:, ci] != -1.0
            assert np.hypot(D[seen, ci, :, 0], D[seen, ci, :, 1]).min() >= MIN_LENGTH
            if CASES[ci][3] == S:
                continue
            th = angle(D[v, ci])
            cp, taps = o["Conf_patch"][v, ci], angle(o["Ori_patch"][v, ci])
            d0 = line_dist(th, taps[0])
            for p in np.flatnonzero(cp > F(THR)):
                assert np.abs(line_dist(th, taps[p]) - d0).min() >= 2 * ANGLE_MARGIN, (CASES[ci][0], p)
    return True


def map_checksums(maps):
    return sc.map_checksums(maps)


def rankings(rec, case):
    """name -> (idx [20,N] int32, val [20,N] float32) for forward(pts, base_view=...), patch 3, S = 90, from the batch's own
    ranking:
      rep   every point's rank-0 base view again at rank 2, with its value: equal losses, the strict `lt` of PMVO.py:64 keeps
            rank 0;
      zero  for the points of k4 and k5: another seeing view u at rank 0, the tuned base view at rank 2 with base_val exactly 0
            (not taken, whatever its loss), every later rank 0 as well;
      tiny  the same with base_val TINY at rank 2: taken where its loss is the smaller.
    u is the first seeing view (ascending) whose rank loss the oracle finds larger than the tuned base view's, with the other
    flag where there is one."""
    views, pts = views_of(np.ascontiguousarray(rec, F), case["maps"]), case["points"]
    o, bidx, bval, D = rank0(views, pts, 90, 3)
    own = oracle.prj_loss(D, o["Ori_patch"], o["Conf_patch"], o["visible"], THR)
    rep = (bidx.copy(), bval.copy())
    rep[0][2], rep[1][2] = bidx[0], bval[0]
    zero = (bidx.copy(), bval.copy())
    for name in ("k4", "k5"):
        n = NAMES.index(name)
        best = None
        for u in np.flatnonzero(o["visible"][:, n] != -1.0):
            if u in (bidx[0, n], case["view"][n]):
                continue
            b2 = bidx[0].copy()
            b2[n] = u
            D2 = oracle.reproject_ori(views, pts, oracle.sample_next(views, pts, b2, o["Ori"], offsets(90)))
            l2, _, h2 = oracle.prj_loss(D2, o["Ori_patch"], o["Conf_patch"], o["visible"], THR)
            if own[0][n] < l2[n] and (best is None or (h2[n] != own[2][n] and not best[1])):
                best = (int(u), bool(h2[n] != own[2][n]))
        assert best is not None, "no other base view with a larger loss for " + name
        zero[0][0, n], zero[0][2, n] = best[0], bidx[0, n]
        zero[1][0, n], zero[1][2:, n] = bval[0, n], 0
    tiny = (zero[0].copy(), zero[1].copy())
    for name in ("k4", "k5"):
        tiny[1][2, NAMES.index(name)] = TINY
    return dict(rep=rep, zero=zero, tiny=tiny)


# ------------------------------------------------------------------------------------------------------- 8-bit code maps
CODE_HIGH, CODE_LOW = 230, 3          # confidence codes: 230 / 255 = 0.902, 3 / 255 = 0.0118
CODE_CASES = (("c8k4", 4), ("c8k5", 5))


def code_angle(code):
    """the angle (as angle() measures it) of the orientation an 8-bit code decodes to: (sin o, cos o), o = (180 - code) degrees"""
    return np.asarray(code, np.float64) * np.pi / 180 - np.pi / 2


def scene_codes():
    """-> (camera list, dict(depth float32, k8, c8, m8 uint8) of the quantised scene, candidate points)"""
    from monohair_amd import synth

    s = synth.make_scene_codes(V, H, W, seed=SEED, rings=2)
    codes = dict(depth=s["depth"].numpy().copy(), k8=s["ori_u8"].numpy().copy(), c8=s["conf_u8"].numpy().copy(), m8=s["mask_u8"].numpy().copy())
    return s["cams"], codes, synth.candidate_points(res=RES, seed=SEED, limit=LIMIT).astype(F)


def decode(codes):
    from monohair_amd.pmvo_utils import map_code_lut

    lut = map_code_lut()
    return dict(depth=codes["depth"], ori=np.ascontiguousarray(lut[codes["k8"]][..., :2]), conf=np.ascontiguousarray(lut[codes["c8"]][..., 2]),
                mask=np.ascontiguousarray(lut[codes["m8"]][..., 3]))


def code_pair(th, want):
    """orientation codes (tap 0, other cells) whose nearer one, over the sweep th, is the other cells' exactly on the samples
    `want`, no sample within ANGLE_MARGIN of their bisector; None if no pair of the 180 x 180 does (codes are 1 degree apart)"""
    dist = line_dist(th[None, :], code_angle(np.arange(180))[:, None])
    for a in range(180):
        diff = dist - dist[a]
        ok = ((diff < 0) == want).all(1) & (np.abs(diff) >= 2 * ANGLE_MARGIN).all(1)
        if ok.any():
            return a, int(np.flatnonzero(ok)[0])
    return None


def build_codes(rec):
    """the 4 / 5 pair on the quantised scene (make_scene_codes): every usable (point, view) pair is tried.  -> dict(codes, points
    [2,3], rows, view, base, edits [E,6] (case, view, row, col, orientation code of tap 0 or -1, code of the other cells or the
    confidence code of an untuned patch)) or None where no pair of codes leaves 4 and 5 positive samples"""
    _, codes, cand = scene_codes()
    rec = np.ascontiguousarray(rec, F)
    views0 = views_of(rec, decode(codes))
    o0 = oracle.visible_and_ori(views0, cand, 3)
    see = o0["visible"] != -1.0
    bidx, bval = oracle.topk_views(o0["visible"], o0["Conf"], 20)
    used = bidx[0:20:2]
    D0 = oracle.reproject_ori(views0, cand, oracle.sample_next(views0, cand, bidx[0], o0["Ori"], offsets(90)))
    order = sorted(range(len(cand)), key=lambda n: (int(see[:, n].sum()), n))
    reserved, rows, tuned, bases, edits = [], [], [], [], []

    def put(c, v, r, col, k=None, conf=None):
        win = (v, slice(r - 1, r + 2), slice(col - 1, col + 2))
        if k is not None:
            c["k8"][win] = np.asarray(k, np.uint8).reshape(3, 3)
        c["c8"][win] = np.asarray(conf, np.uint8).reshape(3, 3) if np.ndim(conf) else np.uint8(conf)

    for ci, (name, k) in enumerate(CODE_CASES):
        done = False
        want = np.arange(90) < k
        for n in order:
            m = int(see[:, n].sum())
            if n in rows or m < 2 or bval[0, n] <= 0.2:
                continue
            rr, cc, oob = pixels(rec, cand[n])
            if any(see[v, n] and not (1 <= rr[v] < H - 1 and 1 <= cc[v] < W - 1) for v in range(V)):
                continue
            if any(see[v, n] and s2[v] and abs(rr[v] - r2[v]) <= RESERVE and abs(cc[v] - c2[v]) <= RESERVE for r2, c2, s2 in reserved for v in range(V)):
                continue
            b = int(bidx[0, n])
            for v in range(V):
                if not see[v, n] or v in used[:, n]:
                    continue
                th = sweep(D0[v, n])
                pair = None if th is None else code_pair(th, want)
                if pair is None:
                    continue
                others = [u for u in range(V) if see[u, n] and u not in (v, b)]
                trial = {key: val.copy() for key, val in codes.items()}
                for u in others + [v]:
                    put(trial, u, rr[u], cc[u], conf=0)
                share = point_state(views_of(rec, decode(trial)), cand[n], 3, D0[:, n])[0]["ratio"][0] * m
                if share.max() - share.min() > 1e-3:
                    continue
                c_other = CODE_LOW if not others else int(np.clip(np.rint(255 * (THR * m - float(share.mean()) - (CODE_HIGH + CODE_LOW) / 510) / len(others)), 1, 30))
                trial = {key: val.copy() for key, val in codes.items()}
                kk, cf = [pair[1]] * 9, [CODE_HIGH] * 9
                kk[0], cf[0], cf[4] = pair[0], CODE_LOW, CODE_LOW
                put(trial, v, rr[v], cc[v], kk, cf)
                for u in others:
                    put(trial, u, rr[u], cc[u], conf=c_other)
                st, _ = point_state(views_of(rec, decode(trial)), cand[n], 3, D0[:, n])
                if not np.array_equal(st["ratio"][0] > F(THR), want) or np.abs(st["ratio"][0] - F(THR)).min() < MARGIN + 2e-3:
                    continue
                alt = point_state(views_of(rec, decode(trial)), cand[n], 3, D0[:, n], low_below=4 if k == 4 else 6)[0]
                if alt["idx"][0] == st["idx"][0] and alt["hc"][0] == st["hc"][0]:          # (the two regimes must differ on it)
                    continue
                codes = trial
                reserved.append((rr, cc, see[:, n].copy()))
                rows.append(n), tuned.append(v), bases.append(b)
                edits.append((ci, v, rr[v], cc[v], pair[0], pair[1]))
                edits += [(ci, u, rr[u], cc[u], -1, c_other) for u in others]
                done = True
                break
            if done:
                break
        if not done:
            return None
    out = dict(codes=codes, points=np.ascontiguousarray(cand[rows]), rows=np.array(rows, np.int32), view=np.array(tuned, np.int32),
               base=np.array(bases, np.int32), edits=np.array(edits, np.int32))
    # on the final maps and the batch of the two points
    views = views_of(rec, decode(codes))
    o, bi, bv, D = rank0(views, out["points"], 90, 3)
    assert np.array_equal(bi[0], out["base"])
    st = sc.prj_loss_np(D, o["Ori_patch"], o["Conf_patch"], o["visible"], THR)
    for ci, (name, k) in enumerate(CODE_CASES):
        assert np.array_equal(st["ratio"][ci] > F(THR), np.arange(90) < k) and np.abs(st["ratio"][ci] - F(THR)).min() >= MARGIN
        seen = o["visible"][:, ci] != -1.0
        assert np.hypot(D[seen, ci, :, 0], D[seen, ci, :, 1]).min() >= MIN_LENGTH
        th, taps = angle(D[out["view"][ci], ci]), angle(o["Ori_patch"][out["view"][ci], ci])
        assert np.abs(line_dist(th, taps[1]) - line_dist(th, taps[0])).min() >= 2 * ANGLE_MARGIN
    return out


# ------------------------------------------------------------------------------------------------- reading the fixture
def load():
    import ast
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pmvo_lowconf.npz"), allow_pickle=False)
    return ast.literal_eval(str(z["meta"])), z


def records(z):
    rec = np.zeros((V, 48), F)
    rec[:, 0:16] = z["cam_pose"].reshape(V, 16)
    rec[:, 16:32] = z["cam_proj"].reshape(V, 16)
    rec[:, 32:41] = z["cam_rinv"].reshape(V, 9)
    return rec


_cache = {}


def case_of(z):
    """(case, [V,48] records) regenerated from the fixture's camera records and checked against the file"""
    if "case" not in _cache:
        rec = records(z)
        case = build(rec)
        assert np.array_equal(case["points"], z["points"]) and np.array_equal(case["edits"], z["edits"]), "the cases do not regenerate"
        assert np.array_equal(case["edit_conf"], z["edit_conf"]) and np.array_equal(case["view"], z["view"])
        assert np.array_equal(map_checksums(case["maps"]), z["map_sums"]), "the maps do not regenerate"
        _cache["case"] = (case, rec)
    return _cache["case"]


def codes_case_of(z):
    """the 4 / 5 pair on 8-bit code maps, regenerated and checked against the file"""
    if "codes" not in _cache:
        cc = build_codes(records(z))
        assert cc is not None and np.array_equal(cc["points"], z["c8_points"]) and np.array_equal(cc["edits"], z["c8_edits"])
        assert np.array_equal(np.array([cc["codes"][k].astype(np.float64).sum() for k in ("depth", "k8", "c8", "m8")]), z["c8_map_sums"])
        _cache["codes"] = cc
    return _cache["codes"]
