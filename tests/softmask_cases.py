"""Shared by tools/gen_golden_softmask.py and tests/test_soft_mask_*.py: the seeded case behind tests/golden/pmvo_softmask.npz.
Soft hair masks and compared quantities that sit exactly on their thresholds -- what a real capture has and no other fixture:

  * mask codes drawn from {0, 49, 50, 51, 52, 255}: the loader zeroes codes below 50 and divides by 255, the votes set m > 0.2 to
    1, float32(51 / 255.0) IS float32(0.2) and stays a fraction, so codes 50 and 51 enter the votes' sums over the views as
    0.196... and 0.2 and the order of those sums decides rows; a second palette for PMVO.from_planes puts 0.1f, the two
    neighbours of 0.2f and 0.2f itself on the same pixels;
  * confidence codes with 51 and 102 (float32 0.2 and 0.4, the two recorded conf_threshold values) common;
  * designed points whose pixels are painted so that a vote is a tie in the reals (class m), a patch maximum equals the threshold
    (c), one view's weight equals it (w), two views see the point over taps on both sides of the code (p), and -- in the hand-made view with a dyadic z' * 255 -- the depth gap equals 0.1f, 0.9f
    or 1.0 exactly and one ulp either side (g);
  * two view counts: 24 (23 ring cameras + the hand-made one) and 272 (view v has camera v % 24 and maps of its own): level 1
    of ATen's cascade flushes every 16 views, level 2 at 256.

Plain numpy restatements of the votes (PMVO.py:110-137, :402-480) on the per-pair terms, with the summation order and every
comparison operator as switches -- what the generator and the host test use to prove that the fixture can tell a wrong order or
operator from the right one.  numpy Generator streams and IEEE arithmetic only; nothing from the GPU side."""
import numpy as np

import border_cases as bc
import cascade_cases as cc

H, W = bc.H, bc.W            # 32 x 64
NCAM, HAND = 24, 23          # the cameras of border_cases: 23 ring cameras + the hand-made one (pure translation, ndc_prj 2, 2)
VIEW_COUNTS = (24, 272)
THRS = (0.4, 0.2)            # conf_threshold: the reference's default and code 51
VIS_THR = 1.0
PATCHES = (3, 5)
SEED = 32                    # chosen by `tools/gen_golden_softmask.py --search`: every order family of both view counts occurs
TILE = 14                    # vote launches of TILE * N >= 4096 points take the lane-per-point kernel
F = np.float32
CODES = np.array([0, 49, 50, 51, 52, 255], np.uint8)
CODE_WEIGHTS = (0.2, 0.1, 0.2, 0.2, 0.1, 0.2)
LO2, HI2 = np.nextafter(F(0.2), F(0)), np.nextafter(F(0.2), F(1))
PLANE_PALETTE = np.array([0, 0.1, LO2, 0.2, HI2, 1], F)     # the float-plane variant: the value each of CODES stands for
PALETTES = ("u8", "planes")
SINGLES = 10                 # rows handed over one at a time (batches of one point)
GAP_SEEN, GAP_NEAR, GAP_HIDDEN = -0.5, 0.5, 3.0             # painted depth gaps far from 0.1 / 0.9 / 1.0

# class m: (codes 49, 50, 51, ones, zeros) under the views that see the point -- a tie of `seen - sum(seen * m) < seen / 2` in
# the reals for the 8-bit palette (51 / 255 = 0.2, 51 * 50 / 255 = 10), for the float palette (0.1f, 0.2f-, 0.2f) or for both
DESIGNS_24 = ((0, 0, 5, 3, 0), (0, 0, 5, 4, 1), (0, 0, 10, 6, 0), (0, 0, 5, 5, 2), (0, 0, 10, 7, 1), (0, 0, 15, 9, 0),
              (0, 5, 0, 3, 0), (0, 5, 5, 6, 0), (10, 0, 0, 8, 0), (10, 0, 5, 9, 0), (0, 10, 0, 6, 0), (0, 5, 0, 4, 1))
DESIGNS_272 = ((0, 51, 0, 31, 0), (0, 51, 5, 34, 0), (0, 51, 10, 38, 1), (0, 102, 0, 62, 0), (0, 0, 50, 30, 0),
               (0, 0, 100, 60, 0), (0, 50, 50, 60, 0), (10, 0, 45, 35, 0), (0, 51, 0, 33, 2), (0, 0, 85, 53, 2),
               (0, 153, 0, 93, 0), (20, 40, 40, 56, 0)) + DESIGNS_24[:4]
# class g: (k, t): the point lies at camera-space z = -2^-k of the hand-made view (z' * 255 = 255 * 2^-(k+1), dyadic) and the
# depth under it is z' * 255 - t.  z' * 255 = 63.75 (k = 1) holds t = 1.0 only; 1.9921875 (k = 6) holds 1.0 and its neighbours;
# 0.12451171875 (k = 10) holds 0.1f, 0.9f and theirs
G_T = {"1.0": F(1.0), "0.1": F(0.1), "0.9": F(0.9)}


def _nb(t, s):
    return np.nextafter(F(t), F(t) + F(s))


G_FAMILIES = [(1, "1.0", 0)] + [(6, "1.0", s) for s in (0, -1, 1)] + [(10, n, s) for n in ("0.1", "0.9") for s in (0, -1, 1)]
N_R, N_M, N_C, N_W, N_P, N_G = 192, 64, 10, 6, 10, 3 * len(G_FAMILIES)


def view_records(rec24, V):
    return np.ascontiguousarray(rec24[np.arange(V) % NCAM])


def camera_list(V):
    base = bc.cameras()
    return [dict(base[v % NCAM], file="view_%03d" % v) for v in range(V)]


def thr_code(thr):
    return int(round(thr * 255))            # 102 / 51: float32(code / 255.0) == float32(thr)


def _unproject(rec, fx, fy, rowf, colf, z255):
    """float64 world point that the camera of record `rec` sees at the unrounded pixel (rowf, colf) with z' * 255 = z255
    (plain sums of products of the stored float32 record: the same value wherever it is computed)"""
    t, rinv = rec[[3, 7, 11]].astype(np.float64), rec[32:41].astype(np.float64).reshape(3, 3)
    zc = -z255 / 127.5
    q = np.array([(1.0 - 2.0 * colf / W) * zc / fx, (2.0 * rowf / H - 1.0) * zc / fy, zc]) - t
    return np.array([rinv[i, 0] * q[0] + rinv[i, 1] * q[1] + rinv[i, 2] * q[2] for i in range(3)])


def _project24(rec24, pts):
    import oracle

    res = [oracle.project_points(rec24[v], pts, H, W) for v in range(NCAM)]
    rc, zp, oob = (np.stack([r[k] for r in res]) for k in range(3))
    return rc, (zp * F(255.0)).astype(F), oob


def build(rec24, V, seed=SEED):
    """-> dict(k8, c8, m8 [V,H,W] uint8, depth [V,H,W] float32, points [N,3] float32, tags [N] class letters, info [N,3] int32
    (class-specific: m = target (0 surface, 1 filter), design; c / w = threshold code; g = family), singles [SINGLES] rows)"""
    assert V % NCAM in (0, 8) and V >= NCAM
    cams = bc.cameras()
    rng = np.random.default_rng([seed, V, 1])
    k8 = rng.integers(0, 256, (V, H, W), dtype=np.uint8)
    c8 = rng.integers(0, 256, (V, H, W), dtype=np.uint8)
    u = rng.random((V, H, W))
    c8[u < 0.15] = 51
    c8[(u >= 0.15) & (u < 0.30)] = 102
    m8 = CODES[rng.choice(len(CODES), (V, H, W), p=CODE_WEIGHTS)]
    depth = (F(102.0) + (rng.random((V, H, W), dtype=F) - F(0.5)) * F(24.0)).astype(F)
    hands = np.flatnonzero(np.arange(V) % NCAM == HAND)
    depth[hands] = (F(bc.HAND_Z255) - (rng.random((len(hands), H, W), dtype=F) * F(0.6) - F(0.2))).astype(F)
    copies = [np.flatnonzero(np.arange(V) % NCAM == b) for b in range(NCAM)]
    claimed = np.zeros((NCAM, H, W), bool)
    pts, tags, info = [], [], []
    rng = np.random.default_rng([seed, V, 2])
    designs = DESIGNS_24 if V == 24 else DESIGNS_272
    scalp = cc.toy_head()[1]             # (designed points stay 5 cm away: the head filter's scalp test leaves them alone)
    ring_views = np.flatnonzero(np.arange(V) % NCAM != HAND)

    def candidate(halo, bases=()):
        """a point 5 cm or more from the toy scalp that all 24 cameras see, on pixels no designed point owns"""
        for _ in range(20000):
            p = (rng.uniform(-1, 1, 3) * (0.35, 0.2, 0.35)).astype(F)
            if np.hypot(p[0], p[2]) > 0.35 or np.sqrt(((scalp - p.astype(np.float64)) ** 2).sum(1)).min() < 0.05:
                continue
            rc, z255, oob = _project24(rec24, p[None])
            rc = rc[:, 0]
            if oob.any() or (rc[:, 0] < 1).any() or (rc[:, 0] > H - 2).any() or (rc[:, 1] < 1).any() or (rc[:, 1] > W - 2).any():
                continue
            hb = [halo if b in bases else 0 for b in range(NCAM)]       # (a window only in the views that will see the point)
            win = [(b, slice(rc[b, 0] - hb[b], rc[b, 0] + hb[b] + 1), slice(rc[b, 1] - hb[b], rc[b, 1] + hb[b] + 1)) for b in range(NCAM)]
            if any(claimed[w].any() for w in win):
                continue
            for w in win:
                claimed[w] = True
            return p, rc, z255[:, 0]
        raise AssertionError("no free pixels left for a designed point")

    def view_pixels(rc, z255):
        """per view of the case: (row, col, z' * 255)"""
        b = np.arange(V) % NCAM
        return rc[b, 0], rc[b, 1], z255[b]

    def set_gap(v, r, c, z, gap):
        depth[v, r, c] = F(z - F(gap))

    # ---- c: in 4 of the views that see the point every tap lies below the threshold code, in one the patch maximum IS the
    # code, in the others one tap is 255 and the rest lie on, above and below the code; w: one view sees the point and every tap
    # of it is the code; p: two views see it, taps on both sides of the code
    for cls, count in (("c", N_C), ("w", N_W), ("p", N_P)):
        for i in range(count):
            T = thr_code(THRS[i % 2])
            nseen = dict(c=6, w=1, p=2)[cls]
            bases = rng.permutation(NCAM - 1)[:nseen]          # ring cameras; one copy of each sees the point
            p, rc, z255 = candidate(1, set(bases.tolist()))
            r, c, z = view_pixels(rc, z255)
            seen = np.array([int(rng.choice(copies[b])) for b in bases])
            gaps = np.full(V, GAP_HIDDEN)
            gaps[seen] = GAP_SEEN
            for v in range(V):
                set_gap(v, r[v], c[v], z[v], gaps[v])
            for j, v in enumerate(seen):
                if cls == "c" and j < 4:
                    tap = rng.integers(0, T, (3, 3))
                elif cls == "c" and j == 4:
                    tap = rng.integers(0, T, (3, 3))
                    tap[tuple(rng.integers(0, 3, 2))] = T
                elif cls == "w":
                    tap = np.full((3, 3), T)
                else:
                    tap = rng.choice([T - 20, T, T, T + 1, T + 30, 255], (3, 3))
                    if cls == "c":
                        tap[tuple(rng.integers(0, 3, 2))] = 255
                c8[v, r[v] - 1:r[v] + 2, c[v] - 1:c[v] + 2] = tap.astype(np.uint8)
                m8[v, r[v], c[v]] = 255
            pts.append(p), tags.append(cls), info.append((T, nseen, 0))
    # ---- m: ties of the mask vote
    for i in range(N_M):
        target, d = i % 2, (i // 2) % len(designs)
        n49, n50, n51, ones, zeros = designs[d]
        p, rc, z255 = candidate(0)
        r, c, z = view_pixels(rc, z255)
        seen = rng.permutation(V)[:n49 + n50 + n51 + ones + zeros]
        code = np.repeat(np.array([49, 50, 51, 255, 0], np.uint8), (n49, n50, n51, ones, zeros))
        gaps = np.full(V, GAP_HIDDEN)
        gaps[seen] = GAP_NEAR if target else GAP_SEEN
        m8[seen, r[seen], c[seen]] = code          # (seen is in random order: so is the placement of the fractions)
        for v in range(V):
            set_gap(v, r[v], c[v], z[v], gaps[v])
        pts.append(p), tags.append("m"), info.append((target, d, 0))
    # ---- g: exact depth gaps in the hand-made view (every copy of it paints its own depth: the first holds the tie, the next
    # one or two see the point plainly, the others do not)
    hand_px = set()
    for fam, (k, name, s) in enumerate(G_FAMILIES):
        for rep in range(3):
            while True:
                row, col = int(rng.integers(2, H - 2)), int(rng.integers(2, W - 2))
                if (row, col) not in hand_px and not claimed[HAND, row, col]:
                    break
            hand_px.add((row, col))
            claimed[HAND, row, col] = True
            zc = -(2.0 ** -k)
            p = _unproject(rec24[HAND], 2.0, 2.0, row + 0.25, col + 0.25, -zc * 127.5).astype(F)
            z = F(255.0 * 2.0 ** -(k + 1))
            t = G_T[name] if s == 0 else _nb(G_T[name], s)
            plain = 2 if name == "0.9" else 1        # with the tie pair: 3 seeing views for `> 2`, 2 for `> 1`
            for j, v in enumerate(hands):
                depth[v, row, col] = F(z - t) if j == 0 else F(z - F(GAP_SEEN if j <= plain else GAP_HIDDEN))
                m8[v, row, col] = (255, 0, 255, 51)[(rep + j) % 4] if j else 255
            # the ring views that have the point in bounds do not see it -- but for `plain` of them where there is one hand-made
            # view only -- so that the tie pair decides the count of seeing views
            rc, zr, oob = _project24(rec24, p[None])
            need = plain if len(hands) == 1 else 0
            for b in range(NCAM - 1):
                rb, cb = rc[b, 0]
                if oob[b, 0] or claimed[b, rb, cb]:
                    continue
                claimed[b, rb, cb] = True
                for v in copies[b]:
                    set_gap(v, rb, cb, zr[b, 0], GAP_SEEN if need else GAP_HIDDEN)
                    m8[v, rb, cb] = 255
                need = max(need - 1, 0)
            pts.append(p), tags.append("g"), info.append((fam, rep, 0))
    # ---- r: ordinary points over the unpainted and painted maps alike
    for i in range(N_R):
        b = int(rng.integers(0, NCAM))
        v = int(rng.choice(copies[b]))
        rowf, colf = rng.integers(2, H - 2) + rng.uniform(-0.3, 0.3), rng.integers(2, W - 2) + rng.uniform(-0.3, 0.3)
        z255 = float(depth[v, int(np.rint(rowf)), int(np.rint(colf))]) + float(rng.choice([-0.4, 0.05, 0.2, 0.6, 0.95]))
        pts.append(_unproject(rec24[b], float(F(cams[b]['ndc_prj'][0])), float(F(cams[b]['ndc_prj'][1])), rowf, colf, z255).astype(F)), tags.append("r"), info.append((v, 0, 0))
    # the trailing N mod 32 rows (ATen's row_sum order) are all ties of the mask vote; the other classes mix over the blocks
    is_m = np.flatnonzero(np.array(tags) == "m")
    tail = is_m[rng.permutation(len(is_m))[:len(pts) % 32]]
    rest = np.setdiff1d(np.arange(len(pts)), tail)
    order = np.concatenate([rest[rng.permutation(len(rest))], tail])
    tags, info = np.array(tags)[order], np.array(info, np.int32)[order]
    singles = np.concatenate([np.flatnonzero(tags == t)[:n] for t, n in (("m", 4), ("g", 2), ("c", 2), ("w", 1), ("r", 1))])
    assert len(singles) == SINGLES
    return dict(k8=k8, c8=c8, m8=m8, depth=depth, points=np.array(pts, F)[order], tags=tags, info=info, singles=singles)


def mask_plane(lut, m8, palette):
    if palette == "u8":
        return np.ascontiguousarray(lut[m8][..., 3])
    table = np.zeros(256, F)
    table[CODES] = PLANE_PALETTE
    return table[m8]


def decode(lut, case, palette):
    """the float planes of a case under one palette (lut = pmvo_utils.map_code_lut())"""
    return dict(depth=case["depth"], ori=np.ascontiguousarray(lut[case["k8"]][..., :2]),
                conf=np.ascontiguousarray(lut[case["c8"]][..., 2]), mask=mask_plane(lut, case["m8"], palette))


def map_checksums(maps):
    return np.array([maps[k].astype(np.float64).sum() for k in ("depth", "ori", "conf", "mask")])


def compositions(case):
    """name -> points: the batch, the batch tiled to the size of the lane-per-point vote kernel, and batches of one point"""
    pts = case["points"]
    out = {"batch": pts, "tiled": np.tile(pts, (TILE, 1))}
    for j, n in enumerate(case["singles"]):
        out["one%d" % j] = pts[n:n + 1]
    return out


# --------------------------------------------------------------------------------------------- per-pair terms and the votes
def pair_terms(rec, pts, case, maps, patch):
    """what the votes read per (view, point) pair, from the oracle's projection: dict of [V,N] arrays -- oob, gap = z' * 255 -
    depth, m (mask value), code (mask code), cmax (maximum of the raw patch confidences), ccode / kcode [V,N,P] (the patch's
    confidence and orientation codes in tap order)"""
    rc, zp, oob, _ = bc.project(rec, pts)
    V = len(rec)
    vi = np.arange(V)[:, None]
    r, c = rc[..., 0], rc[..., 1]
    hp = bc.side(patch) // 2
    taps = [case["c8"][vi, np.clip(r + i, 0, H - 1), np.clip(c + j, 0, W - 1)] for i in range(-hp, hp + 1) for j in range(-hp, hp + 1)]
    ccode = np.stack(taps, -1)
    kcode = np.stack([case["k8"][vi, np.clip(r + i, 0, H - 1), np.clip(c + j, 0, W - 1)] for i in range(-hp, hp + 1)
                      for j in range(-hp, hp + 1)], -1)
    return dict(oob=oob, gap=(zp * F(255.0)).astype(F) - maps["depth"][vi, r, c], m=maps["mask"][vi, r, c], code=case["m8"][vi, r, c],
                ccode=ccode, kcode=kcode, cmax=(ccode.max(-1) / 255.0).astype(F), cconf=(case["c8"][vi, r, c] / 255.0).astype(F))


OPS = {">": np.greater, ">=": np.greater_equal, "<": np.less, "<=": np.less_equal}
RULES = dict(gap01=">", gap_vis=">", gap09=">", gap_head=">=", cmax="<", mask=">")      # PMVO.py:422, 424, 470, 121, 426, 427/124
OPPOSITE = {">": ">=", ">=": ">", "<": "<=", "<=": "<"}


def vote_terms(t, thr, vis_thr=VIS_THR, flip=None):
    """the eight [V,N] float32 summands of the votes; flip = the name of one rule of RULES to evaluate with the opposite operator"""
    op = {k: OPS[OPPOSITE[o] if k == flip else o] for k, o in RULES.items()}
    one = lambda b: b.astype(F)          # noqa: E731
    unv = one(t["oob"] | op["gap01"](t["gap"], F(0.1)))
    unv1 = one(t["oob"] | op["gap_vis"](t["gap"], F(vis_thr)))
    unv9 = one(t["oob"] | op["gap09"](t["gap"], F(0.9)))
    unvh = one(op["gap_head"](t["gap"], F(vis_thr)))
    lowc = one(op["cmax"](np.where(t["oob"], F(0), t["cmax"]), F(thr)))
    m = np.where(op["mask"](t["m"], F(0.2)), F(1), t["m"])
    return [(1 - unv) * lowc, 1 - unv, (1 - unv) * m, 1 - unv1, (1 - unv1) * m, 1 - unv9, 1 - unvh, (1 - unvh) * m]


def sum_aten(x):
    """torch.sum(x, dim=0) of [V,N]: blocks of 32 points in cascade order, the trailing N mod 32 in row_sum order; [V,1] in the
    order of a sum over the inner dimension"""
    if x.shape[1] == 1:
        return cc.inner_sum(np.ascontiguousarray(x.T))
    return cc.outer_sum(x)


def sum_left_to_right(x):
    acc = np.zeros(x.shape[1], F)
    for row in x:
        acc = acc + row
    return acc


def sum_cascade_everywhere(x):
    return cc._multi_row_sum(np.ascontiguousarray(x, F), 4)


def votes(terms, total=sum_aten):
    """-> (surface_index, filter_index, unvisible_index, head vote before the scalp test) from the eight summands"""
    s = [total(np.ascontiguousarray(x, F)) for x in terms]
    low = s[0] > 4
    hair, hair1 = (s[1] - s[2]) < s[1] * F(1) / F(2), (s[3] - s[4]) < s[3] * F(1) / F(2)
    surf0 = s[1] > 1
    filt0 = (s[3] > 1) & ~surf0
    return surf0 & ~low & hair, filt0 & ~low & hair1, ~(s[5] > 2), ~((s[6] - s[7]) < s[6] * F(1) / F(2))


VOTE_NAMES = ("surface", "filter", "unvisible", "head")


def families(t, vis, thr):
    """counts of the tie pairs among the in-bounds pairs that pass the soft depth test (vis = visible [V,N] > -1): mask codes
    50 and 51, patch maximum on the threshold, a tap on the threshold inside a high-confidence patch"""
    T = thr_code(thr)
    ok = ~t["oob"] & (vis > -1)
    mx = t["ccode"].max(-1)
    return dict(mask50=int((ok & (t["code"] == 50)).sum()), mask51=int((ok & (t["code"] == 51)).sum()),
                cmax_on_thr=int((ok & (mx == T)).sum()), tap_on_thr_in_high_patch=int((ok & (mx > T) & (t["ccode"] == T).any(-1)).sum()))


def gap_families(t, tags, info, hand_views):
    """family name -> pairs of the hand-made views whose gap IS the tie value or its neighbour, by the case's own arithmetic"""
    out = {}
    g = np.flatnonzero(tags == "g")
    for fam, (k, name, s) in enumerate(G_FAMILIES):
        want = G_T[name] if s == 0 else _nb(G_T[name], s)
        rows = g[info[g, 0] == fam]
        key = "gap%s%s_z%d" % (name, {0: "", -1: "-", 1: "+"}[s], k)
        out[key] = int((~t["oob"][hand_views[0], rows] & (t["gap"][hand_views[0], rows] == want)).sum())
    return out


def sensitivity(t, thr, n_rows):
    """rows whose recorded decision would change: per vote output, under a plain left-to-right sum (rows of whole blocks),
    under cascade order (trailing rows), and under the opposite operator of each rule -> dict of counts"""
    base = votes(vote_terms(t, thr))
    N = n_rows
    main = np.arange(N) < N - N % 32
    rep = {}
    ltr, casc = votes(vote_terms(t, thr), sum_left_to_right), votes(vote_terms(t, thr), sum_cascade_everywhere)
    for name, b, a, c in zip(VOTE_NAMES, base, ltr, casc):
        rep["order_main_" + name] = int(((a != b) & main).sum())
        rep["order_tail_" + name] = int(((c != b) & ~main).sum())
    for rule in RULES:
        alt = votes(vote_terms(t, thr, flip=rule))
        rep["op_" + rule] = {n: int((x != y).sum()) for n, x, y in zip(VOTE_NAMES, alt, base) if (x != y).any()}
    return rep


def eligible_taps(t, thr):
    """the taps that can ever hold the running minimum of a (view, point) pair (PMVO.py:162, 174-182): tap 0 always; every tap of
    a patch whose maximum is not above the threshold; else the taps above it -> (eligible [V,N,P] bool, number of distinct
    orientation codes among them [V,N])"""
    T = thr_code(thr)
    high = (t["ccode"].max(-1) > T)[..., None]
    el = np.where(high, t["ccode"] > T, True)
    el[..., 0] = True
    k = np.sort(np.where(el, t["kcode"].astype(np.int32), -1), -1)
    distinct = ((k[..., 1:] != k[..., :-1]) & (k[..., 1:] >= 0)).sum(-1) + (k[..., 0] >= 0)
    return el, distinct


# ------------------------------------------------------------------------------------- the search's loss (PMVO.py:151-209)
SEARCH_RULES = ("cmax", "tap", "weight")      # cmax > thr (:162), conf_p > thr (:178), sum(weight) / sum(weight > 0) > thr (:198)


def prj_loss_np(D, op, cp, vis, thr, flip=None, low_below=5):
    """compute_prj_loss in numpy float32 on D [V,N,S,2], Ori_patch [V,N,P,2], Conf_patch [V,N,P], visible [V,N], the sums over
    the views in ATen's order; flip = one of SEARCH_RULES to evaluate with `>=`; low_below = the bound of the low-confidence rule
    (PMVO.py:199: 5) -> dict(loss, idx, hc [N], npos [N] = positive samples, ratio [N,S] = sum(weight) / sum(weight > 0),
    all [N,S] = the losses the minimum is taken of)"""
    o = {k: OPS[">=" if k == flip else ">"] for k in SEARCH_RULES}
    V, N, S, _ = D.shape
    thr = F(thr)
    high = o["cmax"](cp.max(-1), thr)[..., None]
    nd = np.sqrt(D[..., 0] * D[..., 0] + D[..., 1] * D[..., 1])
    ml = bcf = None
    with np.errstate(invalid="ignore", divide="ignore"):
        for i in range(cp.shape[-1]):
            a = op[:, :, i, None, :]
            na = np.sqrt(a[..., 0] * a[..., 0] + a[..., 1] * a[..., 1])
            sim = np.abs((a[..., 0] * D[..., 0] + a[..., 1] * D[..., 1]) / np.maximum(na * nd, F(1e-8)))
            l, c = F(1) - sim, np.broadcast_to(cp[:, :, i, None], (V, N, S))
            if ml is None:
                ml, bcf = l, c
            else:
                idx = l < ml
                take = (idx & o["tap"](c, thr) & high) | (idx & ~high)
                ml, bcf = np.where(take, l, ml), np.where(take, c, bcf)
        w = np.where(vis[..., None] == -1, F(0), F(1)) * bcf
        tot = lambda x: cc.outer_sum(np.ascontiguousarray(x, F).reshape(V, N * S)).reshape(N, S)      # noqa: E731
        sw = tot(w)
        ratio = sw / tot((w > 0).astype(F))
        pos = o["weight"](ratio, thr)
        loss = tot(ml * w) / sw
    l2 = np.where(pos, loss, F(1))
    low = pos.sum(-1) < low_below
    l2[low] = loss[low]
    nan = np.isnan(l2)
    idx = np.where(nan.any(-1), nan.argmax(-1), np.argmin(np.where(nan, np.inf, l2), -1))
    rows = np.arange(N)
    return dict(loss=l2[rows, idx], idx=idx, hc=pos[rows, idx], npos=pos.sum(-1), ratio=ratio, all=l2)


def search_sensitivity(D, op, cp, vis, thr, ref_idx, ref_hc):
    """on the reference's own tensors of one compute_prj_loss call: the restatement gives the reference's (index, flag) on
    `agree` rows; among those, rows whose (index, flag) change under `>=` in place of `>` per rule; the families the issue names"""
    base = prj_loss_np(D, op, cp, vis, thr)
    agree = (base["idx"] == ref_idx) & (base["hc"] == ref_hc)
    rep = dict(rows=int(len(ref_idx)), agree=int(agree.sum()))
    for rule in SEARCH_RULES:
        alt = prj_loss_np(D, op, cp, vis, thr, flip=rule)
        rep["op_search_" + rule] = int((agree & ((alt["idx"] != base["idx"]) | (alt["hc"] != base["hc"]))).sum())
    rep["weight_on_thr"] = int((base["ratio"] == F(thr)).any(-1).sum())
    rep["positive_4"], rep["positive_5"] = int((base["npos"] == 4).sum()), int((base["npos"] == 5).sum())
    return rep


# ------------------------------------------------------------------------------------------------- reading the fixture
def load():
    import ast
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "pmvo_softmask.npz"), allow_pickle=False)
    return ast.literal_eval(str(z["meta"])), z


def records24(z):
    rec = np.zeros((NCAM, 48), F)
    rec[:, 0:16] = z["cam_pose"].reshape(NCAM, 16)
    rec[:, 16:32] = z["cam_proj"].reshape(NCAM, 16)
    rec[:, 32:41] = z["cam_rinv"].reshape(NCAM, 9)
    return rec


def case_of(z, V):
    """(case, {palette: maps}, [V,48] records) of one view count, regenerated and checked against the file"""
    rec24 = records24(z)
    case = build(rec24, V, int(z["seed"]))
    assert np.array_equal(case["tags"], z["v%d_tags" % V]) and np.array_equal(case["points"], z["v%d_points" % V]), \
        "the points of V=%d do not regenerate" % V
    maps = {p: decode(z["lut"], case, p) for p in PALETTES}
    for p in PALETTES:
        assert np.array_equal(map_checksums(maps[p]), z["v%d_%s_map_sums" % (V, p)]), "the maps do not regenerate"
    return case, maps, view_records(rec24, V)
