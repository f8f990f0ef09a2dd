"""CPU only: the scalp attachment (HairGrow.py:606-812, random_move_strands of Utils/PMVO_utils.py:618-658) restated in
plain numpy -- one pass and the driver loop, per strand and per point, no grid and no wave -- and held to the reference's
own run (tests/golden/hair_scalp.npz, tools/gen_golden_scalp.py) on every recorded quantity, exact.  The fact the
restatement and the kernels rest on is held too: KDTree.query_ball_point of one point returns the points with float64
distance <= r in ascending position in tree.indices.  tests/test_hair_scalp_gpu.py uses the restatement as the comparator
of its sweep."""
import collections
import os

import numpy as np
import pytest
from scipy.spatial import KDTree

from conftest import GOLDEN

F32 = np.float32


def split(pts, lens):
    return [np.ascontiguousarray(a) for a in np.split(pts, np.cumsum(lens)[:-1])] if len(lens) else []


def ball_by_rank(core64, rank, q, r):
    """members of the ball, float64 ((d0*d0 + d1*d1) + d2*d2) <= r*r, in ascending rank"""
    d = q.astype(np.float64) - core64
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    m = np.flatnonzero(dd <= r * r)
    return m[np.argsort(rank[m], kind="stable")]


def nearest(p, s64, stats):
    """KDTree(s).query(p, 1) -> (distance, index), float64; an exact tie is counted (scipy's answer there follows its tree)"""
    d = p.astype(np.float64) - s64
    dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    k = int(np.argmin(dd))
    stats["nearest_ties"] += int((dd == dd[k]).sum() > 1)
    return np.sqrt(dd[k]), k


def similar32(a, b):
    """compute_similar on float32 vectors, every operation rounded to float32 in numpy's order"""
    a, b = a.astype(F32), b.astype(F32)
    dot = F32(F32(a[0] * b[0] + a[1] * b[1]) + a[2] * b[2])
    na = np.sqrt(F32(F32(a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]))
    nb = np.sqrt(F32(F32(b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]))
    return F32(dot / np.maximum(F32(na * nb), F32(1e-4)))


def occupancy_test(ss, vox, ratio_thr, stats):
    """random_move_strands on ss = strand[:index] -> (check, out_ratio as float64, similar).  vox [Z,H,W,4]: the solver's
    orientation (y/z negated) and occupancy."""
    Z, H, W = vox.shape[:3]
    idx = np.rint(ss).astype(np.int64)
    if idx[:, 2].max() >= 192 or (idx[:, 1] >= 256).any() or (idx[:, 0] >= 256).any():
        stats["left_box"] += 1
        return False, 0.0, F32(0)
    if (idx < -np.array([W, H, Z])).any() or (idx >= np.array([W, H, Z])).any():
        raise IndexError("a joined strand indexes outside the occupancy volume")
    v = vox[idx[:, 2], idx[:, 1], idx[:, 0]]
    ori = np.concatenate([ss[1:] - ss[:-1], ss[-1:] - ss[-2:-1]], 0).astype(np.float64)
    a = v[:, :3].astype(np.float64)
    na = np.maximum(np.sqrt((a * a).sum(1)), 1e-8)
    nb = np.maximum(np.sqrt((ori * ori).sum(1)), 1e-8)
    cos = np.abs(((a / na[:, None]) * (ori / nb[:, None])).sum(1))
    s = F32(v[:, 3].sum(dtype=np.float64))
    ratio = F32(s / F32(len(ss)))
    with np.errstate(divide="ignore", invalid="ignore"):
        sim = F32(F32(cos.sum()) / s)
    if ratio > F32(ratio_thr):
        stats["similar_near_0.3"] += int(abs(float(sim) - 0.3) < 1e-4)
    return bool(ratio > F32(ratio_thr) and sim > F32(0.3)), float(F32(1) - ratio), sim


def rs_pass(strands, root, out, out_ratio, flips, choice, sims, vox, thr_dist, thr_dot, ratio_thr, stats):
    """one pass of the while loop, in place on the state; returns the number of strands newly rooted"""
    n = len(strands)
    core_ids = [i for i in range(n) if root[i]]
    core = np.concatenate([strands[i] for i in core_ids], 0)          # raises on an empty list, like the reference
    info = np.concatenate([[i] * len(strands[i]) for i in core_ids])
    core64 = core.astype(np.float64)
    tree = KDTree(core)
    rank = np.empty(len(core), np.int64)
    rank[tree.indices] = np.arange(len(core))
    s64 = {}

    def pts64(j):
        if j not in s64:
            s64[j] = strands[j].astype(np.float64)
        return s64[j]

    new = {}
    for i in range(n):
        if root[i] or out[i]:
            continue
        s = strands[i]
        ball = ball_by_rank(core64, rank, s[0], thr_dist)
        nei = info[ball]
        distinct = list(dict.fromkeys(nei.tolist()))
        stats["ball_distinct_%s" % (len(distinct) if len(distinct) in (0, 1, 30) else (">30" if len(distinct) > 30 else "n"))] += 1
        stats["ball_gt64"] += len(ball) > 64
        if len(ball):
            d = (s[0].astype(np.float64) - core64[ball])
            stats["on_radius"] += int((((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]) == thr_dist * thr_dist).any())
            c = int(nei[0])
            ss = strands[c]
            nd = [nearest(p, pts64(c), stats) for p in s]
            b, e = nd[0][1], nd[-1][1]
            tan1 = ss[b] - ss[b - 1] if b == len(ss) - 1 else ss[b + 1] - ss[b]
            mean = np.mean(np.array([x[0] for x in nd]))
            stats["mean_near_5"] += int(abs(mean - 5) < 1e-9)
            if similar32(tan1, s[1] - s[0]) < 0 and b > e and mean < 5:
                s = s[::-1].copy()
                flips[i] += 1
                stats["flipped"] += 1
        min_loss, best = np.inf, None
        count = 0
        losses = []
        for j in distinct:
            count += 1
            ns = strands[j]
            _, pi = nearest(s[0], pts64(j), stats)
            if np.mean(np.array([nearest(p, pts64(j), stats)[0] for p in s[:5]])) < 1:
                stats["refused_mean"] += 1
                continue
            if len(s) > 60 and len(s) + pi > 150:
                stats["refused_long"] += 1
                continue
            stats["nearest_index_%s" % (pi if pi <= 2 else "n")] += 1
            if pi <= 1:
                continue
            tan = s[1] - s[0]
            e3 = (ns[pi] - s[0]).astype(np.float64)
            dist = np.sqrt(F32((e3[0] * e3[0] + e3[1] * e3[1]) + e3[2] * e3[2]))
            stats["dist_near_thr"] += int(dist != F32(thr_dist) and abs(float(dist) - thr_dist) < 1e-5 * thr_dist)
            loss = np.inf
            if similar32(ns[pi] - ns[pi - 1], tan) > F32(thr_dot) and dist < F32(thr_dist):
                loss = float(F32(F32(1) - similar32(s[0] - ns[pi], tan)) + F32(0.1 * thr_dist))
            loss = loss + out_ratio[j]
            losses.append(loss)
            if loss < min_loss:
                min_loss, best = loss, (j, pi)
            if count >= 30:
                stats["stopped_at_30"] += 1
                break
        fin = sorted(x for x in losses if np.isfinite(x))
        stats["loss_ties"] += int(len(fin) >= 2 and fin[0] == fin[1])
        strands_i = s
        if best is not None:
            j, m = best
            ss = strands[j]
            seed = (s[0] * F32(0.95) + ss[m] * F32(0.05)).astype(F32)
            chain = []
            cur = seed
            for t in range(m):
                nx = (cur + (ss[m - 1 - t] - ss[m - t])).astype(F32)
                nx = (nx * F32(1) + ss[m - 1 - t] * F32(0)).astype(F32)
                chain.append(nx)
                cur = nx
            joined = np.concatenate([np.array(chain, F32)[::-1], seed[None], s], 0)
            check, orat, sim = occupancy_test(joined[:m + 1], vox, ratio_thr, stats)
            strands_i = joined
            new[i] = (check, orat, sim, j, m)
            stats["len_%d_joined" % len(s) if len(s) in (2, 4) else "joined"] += 1
        strands[i] = strands_i
    for i, (check, orat, sim, j, m) in new.items():
        out_ratio[i] = orat
        sims[i] = sim
        choice[i] = (j, m)
        if check:
            root[i] = True
        else:
            out[i] = True
    return sum(1 for v in new.values() if v[0])


def rs_connect(strands, num_root, vox, ratio_thr, stats=None):
    """connect_to_scalp -> dict(passes, root, out, out_ratio, flips, choice, similar, strands (all), returned)"""
    stats = collections.defaultdict(int) if stats is None else stats
    strands = [np.ascontiguousarray(s, F32) for s in strands]
    n = len(strands)
    root = np.zeros(n, bool)
    root[:num_root] = True
    out = np.zeros(n, bool)
    out_ratio = np.zeros(n)
    flips = np.zeros(n, np.int32)
    choice = np.full((n, 2), -1, np.int32)
    sims = np.zeros(n, F32)
    thr_dist, thr_dot = 0.5, 0.9
    passes = []
    while True:
        got = rs_pass(strands, root, out, out_ratio, flips, choice, sims, vox, thr_dist, thr_dot, ratio_thr, stats)
        passes.append((thr_dist, thr_dot, int(root.sum()), int(out.sum())))
        stats["progress_floor_%d" % ((n - num_root) // 500)] += 1
        if not got > (n - num_root) // 500:
            if thr_dist == 2.0 and thr_dot == 0.6:
                break
            thr_dist = min(thr_dist + 0.25, 2.0)
            thr_dot = max(thr_dot - 0.075, 0.6)
    return dict(passes=passes, root=root, out=out, out_ratio=out_ratio, flips=flips, choice=choice, similar=sims,
                strands=strands, returned=[strands[i] for i in range(n) if root[i] or out[i]], stats=stats)


def similar_close(got, ref):
    """random_move_strands' score is float32 torch in the reference (x/0 where no voxel is occupied): equal to 1e-4 where
    the reference's is finite.  The decisions it feeds are pinned exactly by the flags."""
    ok = np.isfinite(ref)
    return np.allclose(got[ok], ref[ok], rtol=1e-4, atol=1e-5)


def load_volume(z):
    """[Z,H,W,4] float32: what HairGrowing packs (orientation with y/z negated, occupancy)"""
    G = tuple(int(g) for g in z["vol_shape"])
    occ = np.zeros(G, np.float32)
    occ[tuple(z["occ_nz"].T.astype(np.int64))] = 1
    ori = np.zeros(G + (3,), np.float32)
    ori[tuple(z["ori_nz"].T.astype(np.int64))] = z["ori_nz_val"]
    occ = occ.transpose(2, 1, 0)[..., None]
    ori = ori.transpose(2, 1, 0, 3)
    vox = np.concatenate([ori * np.array([1, -1, -1], np.float32), occ], -1)
    return occ, ori, np.ascontiguousarray(vox)


def check_recorded(z, tag, res):
    """every recorded quantity of one case against a run's result (restatement or HairGrowing), exact"""
    assert np.array_equal(np.array(res["passes"], np.float64), z[tag + "_passes"])
    assert np.array_equal(res["root"], z[tag + "_root"]) and np.array_equal(res["out"], z[tag + "_out"])
    assert np.array_equal(res["out_ratio"], z[tag + "_out_ratio"])
    assert np.array_equal(res["flips"] % 2, z[tag + "_flipped"])
    assert np.array_equal(res["choice"], z[tag + "_choice"])
    ref = split(z[tag + "_ret_pts"], z[tag + "_ret_len"])
    assert len(ref) == len(res["returned"])
    for a, b in zip(res["returned"], ref):
        assert a.dtype == np.float32 and np.array_equal(a, b)


def case_inputs(z, zc, tag):
    """the float32 voxel-space strands a case starts from; "shell": the strands.hair recorded in hair_connect.npz, taken
    to voxel space as WorldToVoxel does (HairGrow.py:826-835)"""
    if tag == "edge":
        return split(z["edge_in_pts"], z["edge_in_len"])
    import torch

    from monohair_amd.pmvo_utils import points_to_voxel

    b = zc["strands_hair"].tobytes()
    n = int(np.frombuffer(b[:4], "<u4")[0])
    lens = np.frombuffer(b[8:8 + 2 * n], "<u2").astype(int)
    pts = np.frombuffer(b[8 + 2 * n:], "<f4").astype(np.float64).reshape(-1, 3) + zc["bust"]
    return split(points_to_voxel(torch.from_numpy(pts).type(torch.float)).numpy(), lens)


@pytest.fixture(scope="module")
def golden():
    z = np.load(os.path.join(GOLDEN, "hair_scalp.npz"))
    zc = np.load(os.path.join(GOLDEN, "hair_connect.npz"))      # the volume of both cases and the input of "shell"
    return z, zc, load_volume(zc)[2]


@pytest.mark.parametrize("tag", ["shell", "edge"])
def test_restatement_matches_reference(golden, tag):
    z, zc, vox = golden
    strands = case_inputs(z, zc, tag)
    res = rs_connect(strands, int(z[tag + "_num_root"]), vox, float(z[tag + "_ratio_thr"]))
    check_recorded(z, tag, res)
    st = res["stats"]
    assert st["nearest_ties"] == 0 and st["loss_ties"] == 0 and st["similar_near_0.3"] == 0
    joined = z[tag + "_choice"][:, 0] >= 0
    assert similar_close(res["similar"][joined], z[tag + "_similar"][joined])


def test_edge_case_reaches_every_family(golden):
    z, zc, vox = golden
    res = rs_connect(case_inputs(z, zc, "edge"), int(z["edge_num_root"]), vox, float(z["edge_ratio_thr"]))
    st = res["stats"]
    for k in ("ball_distinct_0", "ball_distinct_1", "ball_distinct_30", "ball_distinct_>30", "on_radius", "len_2_joined",
              "len_4_joined", "refused_long", "nearest_index_0", "nearest_index_1", "nearest_index_2", "flipped",
              "left_box", "stopped_at_30", "refused_mean"):
        assert st[k] > 0, k
    assert res["passes"][-1][:2] == (2.0, 0.6) and st["progress_floor_0"] > 0
    assert (len(z["shell_root"]) - int(z["shell_num_root"])) // 500 == 1


def test_query_ball_point_returns_the_radius_set_in_tree_order():
    rng = np.random.default_rng(3)
    for n, r in ((37, 0.5), (500, 1.0), (4000, 2.0)):
        pts = (rng.random((n, 3)) * (6 if n < 1000 else 20)).astype(np.float32)
        pts[n // 2:n // 2 + n // 10] = pts[:n // 10]          # duplicates
        tree = KDTree(pts)
        rank = np.empty(n, np.int64)
        rank[tree.indices] = np.arange(n)
        p64 = pts.astype(np.float64)
        for q in np.concatenate([pts[:40], (rng.random((40, 3)) * 6).astype(np.float32)]):
            got = tree.query_ball_point(q, r)
            assert np.array_equal(np.asarray(got, np.int64), ball_by_rank(p64, rank, q, r))
