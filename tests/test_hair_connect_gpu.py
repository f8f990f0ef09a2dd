"""GPU: segment connection and smoothing (csrc/hairconnect.hip, HairGrowing.find_connect_info, strand_smooth,
connect_segments) against the reference's own run (tests/golden/hair_connect.npz, tools/gen_golden_connect.py) and a
float64 numpy restatement kept here."""
import collections
import math
import os
from fractions import Fraction

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _split(pts, lens):
    return [a for a in np.split(pts, np.cumsum(lens)[:-1])]


@pytest.fixture(scope="module")
def setup():
    from monohair_amd.hairgrow import HairGrowing

    z = np.load(os.path.join(GOLDEN, "hair_connect.npz"))
    G = tuple(int(g) for g in z["vol_shape"])
    occ = np.zeros(G, np.float32)
    occ[tuple(z["occ_nz"].T.astype(np.int64))] = 1
    ori = np.zeros(G + (3,), np.float32)
    ori[tuple(z["ori_nz"].T.astype(np.int64))] = z["ori_nz_val"]
    occ = occ.transpose(2, 1, 0)[..., None]           # [Z,Y,X,1] as get_ground_truth_3D_occ returns
    ori = ori.transpose(2, 1, 0, 3)                   # [Z,Y,X,3]
    hg = HairGrowing(None, None, device=DEV, occ=occ, ori=ori)
    return z, hg, occ, ori


def _shell_segments(z):
    """the non-root segments of the recorded scalp_segment.hair, shifted by bust_to_origin (HairGrow.py:929-939)"""
    b = z["seg_hair"].tobytes()
    n = int(np.frombuffer(b[:4], "<u4")[0])
    lens = np.frombuffer(b[8:8 + 2 * n], "<u2").astype(int)
    pts = np.frombuffer(b[8 + 2 * n:], "<f4").astype(np.float64).reshape(-1, 3)
    segs = _split(pts, lens)
    nr = int(z["num_root"])
    return [s + z["bust"] for s in segs[nr:]], segs[:nr]


def _long_case(z):
    """case "long" of strands_long.npz: (segments, occupancy [Z,Y,X] of the 256 x 256 x 192 box, thr, dot)"""
    segs = _split(z["long_in_pts"].astype(np.float64), z["long_in_len"])
    occ = np.zeros((192, 256, 256), np.float32)
    for x0, x1, y0, y1, z0, z1 in z["long_occ_boxes"].astype(int):
        occ[z0:z1, y0:y1, x0:x1] = 1
    return segs, occ, float(z["connect_thr"]), float(z["connect_dot"])


def _check_case(z, hg, tag, segs, seed, occ=None, thr=None, dot=None):
    np.random.seed(seed)
    out = hg.find_connect_info([s.copy() for s in segs], float(z["thr"]) if thr is None else thr,
                               float(z["dot"]) if dot is None else dot, occ)
    nxt = np.random.random()
    table = np.stack([hg.connect_best, hg.connect_best_type], -1)
    assert np.array_equal(table, z[tag + "_table"])
    ref = _split(z[tag + "_out_pts"], z[tag + "_out_len"])
    assert len(out) == len(ref)
    for a, b in zip(out, ref):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    assert hg.connect_fail == int(z[tag + "_fail"])
    assert nxt == float(z[tag + "_next_random"])
    return out


def test_end_tables_match_reference(setup):
    z, hg, _, _ = setup
    zl = np.load(os.path.join(GOLDEN, "strands_long.npz"))
    lsegs, locc, lthr, ldot = _long_case(zl)
    for tag, segs in (("shell", _shell_segments(z)[0]), ("edge", _split(z["edge_in_pts"], z["edge_in_len"])),
                      ("long", lsegs)):
        if tag == "long":
            z = zl
            hg.find_connect_info(segs, lthr, ldot, locc[None])
        else:
            hg.find_connect_info(segs, float(z["thr"]), float(z["dot"]))
        ends = (np.stack([s[0] for s in segs]), np.stack([s[-1] for s in segs]))
        for k, name in enumerate(("rr", "rt", "tr", "tt")):
            idx, dist, cnt = (t.cpu().numpy() for t in hg._end_lists[k])
            ref_idx = z["%s_%s_idx" % (tag, name)].astype(np.int64)
            assert np.array_equal(cnt, (ref_idx >= 0).sum(1))
            q, d = ends[k // 2], ends[k % 2]
            for i in range(len(segs)):
                r = ref_idx[i, :cnt[i]]
                assert np.array_equal(idx[i, :cnt[i]], r), (tag, name, i)
                df = q[i] - d[r]      # the distance scipy reports: sqrt((d0*d0 + d1*d1) + d2*d2)
                assert np.array_equal(dist[i, :cnt[i]], np.sqrt((df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) +
                                                                df[:, 2] * df[:, 2])), (tag, name, i)


def test_shell_case_matches_reference(setup):
    z, hg, _, _ = setup
    _check_case(z, hg, "shell", _shell_segments(z)[0], 1234)


def test_edge_case_matches_reference(setup):
    z, hg, _, _ = setup
    edge = _split(z["edge_in_pts"], z["edge_in_len"])
    assert (z["edge_rr_idx"] >= 0).sum(1).max() >= 49          # a full row of the k = 50 query
    assert (z["edge_draws"] == 50).any() and ((z["edge_draws"] > 0) & (z["edge_draws"] < 50)).any()
    _check_case(z, hg, "edge", edge, 99)


def test_long_case_matches_reference(setup, tmp_path):
    """case "long" (tools/gen_golden_strands_long.py): segments of 2..513 points, so that mh_best_of_list takes several
    64-point passes, with close counts of 6 and 7 and the end rule decided by points of a later pass; a strand of 1028
    points through chains, occupancy test and smoothing.  Table, float64 strands, fail count, np.random's next value
    and the bytes of the smoothed .hair file are the reference's."""
    from monohair_amd.pmvo_utils import save_hair_strands
    from monohair_amd.strand_smooth import smooth_strands

    _, hg, _, _ = setup
    z = np.load(os.path.join(GOLDEN, "strands_long.npz"))
    segs, occ, thr, dot = _long_case(z)
    L = z["long_in_len"]
    assert {2, 5, 6, 20, 21, 63, 64, 65, 127, 128, 129, 192, 193, 513} <= set(L.tolist())
    t = z["long_table"]
    for e in range(2):
        for ty in range(2):
            m = (t[:, e, 0] >= 0) & (t[:, e, 1] == ty)
            assert (m & (L > 64) & (L <= 128)).any() and (m & (L > 128)).any()
    assert (z["long_out_len"] > 1000).any() and (z["long_draws"] == 50).any()
    assert ((z["long_draws"] > 0) & (z["long_draws"] < 50)).any()
    out = _check_case(z, hg, "long", segs, 4321, occ[None], thr, dot)
    sm = smooth_strands([c - z["bust"] for c in out], 4.0, 2.0, device=DEV)
    save_hair_strands(str(tmp_path / "strands.hair"), sm, z["bust"], translate=False)
    assert (tmp_path / "strands.hair").read_bytes() == z["long_strands_hair"].tobytes()


def test_connect_segments_writes_reference_strands_hair(setup, tmp_path):
    from monohair_amd.hairgrow import connect_segments

    z, _, occ, ori = setup
    (tmp_path / "scalp_segment.hair").write_bytes(z["seg_hair"].tobytes())
    np.save(tmp_path / "num_root.npy", np.array(int(z["num_root"])))
    np.random.seed(1234)
    connect_segments(str(tmp_path), z["bust"], float(z["thr"]), float(z["dot"]), device=DEV, occ=occ, ori=ori)
    assert np.random.random() == float(z["shell_next_random"])
    assert (tmp_path / "strands.hair").read_bytes() == z["strands_hair"].tobytes()


def test_smooth_strands_writes_reference_hair(setup, tmp_path):
    from monohair_amd.pmvo_utils import save_hair_strands
    from monohair_amd.strand_smooth import smooth_strands

    z, _, _, _ = setup
    b = z["seg_hair"].tobytes()
    n = int(np.frombuffer(b[:4], "<u4")[0])
    lens = np.frombuffer(b[8:8 + 2 * n], "<u2").astype(int)
    segs = _split(np.frombuffer(b[8 + 2 * n:], "<f4").reshape(-1, 3).copy(), lens)   # float32, as VoxelToWorld gives
    sm = smooth_strands(segs, 4.0, 2.0, device=DEV)
    save_hair_strands(str(tmp_path / "s.hair"), sm, None, translate=False)
    assert (tmp_path / "s.hair").read_bytes() == z["seg_smooth_hair"].tobytes()


def test_generate_segments_write_smooth(setup, tmp_path):
    from monohair_amd.hairgrow import generate_segments

    z, _, occ, ori = setup
    torch.manual_seed(77)
    generate_segments(None, None, torch.from_numpy(z["scalp_points"].copy()), torch.from_numpy(z["scalp_normals"].copy()),
                      str(tmp_path), z["bust"], 0.8, device=DEV, write_smooth=True, occ=occ, ori=ori)
    assert (tmp_path / "scalp_segment.hair").read_bytes() == z["seg_hair"].tobytes()
    assert (tmp_path / "scalp_segment_smooth.hair").read_bytes() == z["seg_smooth_hair"].tobytes()


# ------------------------------------------------------------------ seeded sweep against a numpy restatement
def _np_lists(segs, thr):
    roots = np.stack([s[0] for s in segs])
    tips = np.stack([s[-1] for s in segs])
    out = []
    for q, d in ((roots, roots), (roots, tips), (tips, roots), (tips, tips)):
        rows = []
        for i, p in enumerate(q):
            df = p - d
            dd = (df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]
            c = np.flatnonzero(dd < thr * thr)
            c = c[np.lexsort((c, dd[c]))][:50]
            c = c[c != i]
            rows.append((c, np.sqrt(dd[c])))
        out.append(rows)
    return out


def _np_nearest(a, b):
    df = a[:, None, :] - b[None, :, :]
    return np.sqrt(((df[..., 0] * df[..., 0] + df[..., 1] * df[..., 1]) + df[..., 2] * df[..., 2]).min(1))


def _np_smooth(s, lap, pos):
    from scipy.linalg import solveh_banded

    n = s.shape[0]
    A = np.zeros((2 * n, n))
    A[0, :2] = [lap, -lap]
    for k in range(1, n - 1):
        A[k, k - 1:k + 2] = [-lap, 2 * lap, -lap]
    A[n - 1, n - 2:] = [-lap, lap]
    A[n:] = np.eye(n) * pos
    M = A.T @ A
    ab = np.zeros((3, n))
    for u in range(3):
        ab[2 - u, u:] = np.diagonal(M, u)
    return solveh_banded(ab, (s * pos) * pos)


# ------------------------------------------------------------------ the connection, restated in plain float64 numpy
# Written from HairGrow.py:303-420 (connect_segments, connect_strands with add_mid), :514-544 (the occupancy loop) and
# :550-590 (find_best_connect_strands): per-point loops and a Python visited list; no wave, no passes, no replayed prefix.
# tests/test_hair_connect_host.py holds it to the reference's recorded tables and strands, which is what licenses it as
# the comparator of the sweep below.
def _fma(a, b, c):
    """correctly rounded a*b + c, independent of the host's BLAS"""
    if hasattr(math, "fma"):
        return math.fma(a, b, c)
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def _rs_nearest(si, sj):
    out = np.empty(len(si))
    for k, p in enumerate(si):
        d = p - sj
        out[k] = np.sqrt(((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).min())
    return out


def _rs_ori(s, tip):
    return s[-1] - s[-2] if tip else s[1] - s[0]


def _rs_best(segs, i, tip_end, nb, nd, nb_tip, same_type, thr, stats):
    s = segs[i]
    a = _rs_ori(s, tip_end)
    na = np.sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2])
    v = s[0] - s[-1]
    slen = math.sqrt(_fma(float(v[2]), float(v[2]), _fma(float(v[1]), float(v[1]), float(v[0]) * float(v[0]))))
    lim = slen * 2 / 3
    best, best_loss, kept = None, None, []
    for j, dj in zip(nb, nd):
        b = _rs_ori(segs[j], nb_tip)
        cs = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) / (na * np.sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]))
        if not (cs < -thr if same_type else cs > thr):
            continue
        dist = _rs_nearest(s, segs[j])
        if len(s) < 6:
            close = dist < 0.005
            ok = close.sum() < 4
        else:
            close = dist < 0.01
            ok = close.sum() <= 6
        late = len(s) > 64 and close[:64].sum() <= 3 and close[64:].any()
        if len(s) >= 6 and late and close.sum() in (6, 7):      # a count of the first pass alone (<= 3) would accept both
            stats["count%d_late" % close.sum()] += 1
            stats["count%d_block%d" % (close.sum(), np.flatnonzero(close)[-1] // 64)] += 1
        if len(s) < 6 and close.sum() in (3, 4):
            stats["short_count%d" % close.sum()] += 1
        if len(s) > 20:
            if dist[0] < lim and dist[-1] < lim:
                if ok and len(s) > 64:
                    stats["end_rule_only_late"] += 1
                ok = False
            elif ok and dist[0] < lim and len(s) > 64:
                stats["kept_by_dlast"] += 1
        if not ok:
            continue
        loss = dj * (1 - abs(cs))
        kept.append((dj, loss))
        if best is None or loss < best_loss:
            best, best_loss = int(j), loss
    if len(kept) >= 2 and np.argmin([k[0] for k in kept]) != np.argmin([k[1] for k in kept]):
        stats["loss_order_differs"] += 1
    if len(kept) >= 2 and sorted(k[1] for k in kept)[0] == sorted(k[1] for k in kept)[1]:
        stats["loss_tie"] += 1
    return best


def _rs_table(segs, lists, thr, stats):
    """[N,2,2]: (neighbour, 0 joined at its root / 1 at its tip) per end, -1 where there is none"""
    t = np.full((len(segs), 2, 2), -1, np.int64)
    for i in range(len(segs)):
        for e in range(2):
            j = _rs_best(segs, i, e, lists[2 * e][i][0], lists[2 * e][i][1], 0, e == 0, thr, stats)
            ty = 0
            if j is None:
                j = _rs_best(segs, i, e, lists[2 * e + 1][i][0], lists[2 * e + 1][i][1], 1, e == 1, thr, stats)
                ty = 1
                stats["fallback"] += j is not None
            if j is not None:
                t[i, e] = (j, ty)
                L = len(segs[i])
                stats["join_gt64"] += L > 64
                stats["join_gt128_%d%d" % (e, ty)] += L > 128
                stats["join_both_long"] += L > 64 and len(segs[j]) > 64
    return t


def _rs_chain(segs, table, i, stats=None):
    pieces, visited = [segs[i]], [i]
    for root_side in (True, False):
        j, ty = table[i, 0 if root_side else 1]
        while j >= 0:
            visited.append(int(j))
            s = segs[j]
            s2 = s[::-1] if (ty == 0) == root_side else s
            new = []
            if root_side:
                seed = pieces[0][0] * 0.5 + s2[-1] * 0.5
                new.append(seed)
                for k in range(len(s2) - 1):
                    seed = (seed + (s2[-2 - k] - s2[-1 - k])) * (1 - 0) + s2[-2 - k] * 0
                    new.append(seed)
                pieces.insert(0, np.array(new)[::-1])
            else:
                seed = pieces[-1][-1] * 0.5 + s2[0] * 0.5
                new.append(seed)
                for k in range(len(s2) - 1):
                    seed = (seed + (s2[k + 1] - s2[k])) * (1 - 0) + s2[k + 1] * 0
                    new.append(seed)
                pieces.append(np.array(new))
            nj, nty = table[j, 1 - ty]
            if nj < 0:
                break
            if nj in visited:
                if stats is not None:
                    stats["cycle"] += 1
                break
            j, ty = nj, nty
    if stats is not None:
        stats["chain_ge4"] += len(visited) >= 4
    return np.concatenate(pieces, 0)


_VMIN = np.array([-0.32, -0.32, -0.24], np.float32).astype(np.float64)


def _rs_occupancy(strand, occ_zyx, stats):
    """the acceptance loop of HairGrow.py:514-544 with np.random's global generator -> (strand, accepted)"""
    ss, count = strand.copy(), 0
    while True:
        idx = np.rint((ss * np.array([1.0, -1.0, -1.0]) - _VMIN) / 0.0025).astype(np.int64)
        if idx[:, 2].max() >= 192 or (idx[:, 1] >= 256).any() or (idx[:, 0] >= 256).any():
            return strand, False
        v = occ_zyx[idx[:, 2], idx[:, 1], idx[:, 0]].astype(np.float32)
        if v.sum(dtype=np.float32) / np.float32(len(v)) > np.float32(0.8):
            stats["retried_ok"] += count > 0
            return ss, True
        ss = strand.copy()
        ss += np.random.random((3)) * 0.005
        count += 1
        if count >= 50:
            stats["exhausted"] += 1
            return strand, False


def _rs_connect(segs, thr, dot, occ_zyx, stats):
    table = _rs_table(segs, _np_lists(segs, thr), dot, stats)
    pre = [_rs_chain(segs, table, i, stats) for i in range(len(segs))]
    out, fail = [], 0
    for s in pre:
        o, ok = _rs_occupancy(s, occ_zyx, stats)
        fail += not ok
        out.append(o)
    return table, pre, out, fail


def _stats():
    return collections.defaultdict(int)


# ------------------------------------------------------------------ the sweep's inputs
_SWEEP_LENS = (2, 3, 5, 6, 7, 20, 21, 22, 63, 64, 65, 66, 127, 128, 129, 200, 513)


def _arc(c, R, a0, n, step, axis_seed):
    """n points `step` apart on a circle of radius R in a plane through c"""
    r = np.random.default_rng(axis_seed)
    u = r.normal(size=3)
    u /= np.linalg.norm(u)
    w = np.cross(u, r.normal(size=3))
    w /= np.linalg.norm(w)
    t = a0 + np.arange(n) * (step / R)
    return c + R * (np.outer(np.cos(t), u) + np.outer(np.sin(t), w))


def _sweep_segments(rng, trial):
    """short random segments as before; long arcs (two 64-point passes and more) with partners laid alongside their
    ends so that 5, 6 or 7 of their points are close; a spiral cut into consecutive pieces of every length of
    _SWEEP_LENS, some reversed (chains of mixed orientation, strands of more than 1000 points); segments sharing exactly
    equal end coordinates.  Everything stays inside the 256 x 256 x 192 box the occupancy test hard-codes."""
    segs = []
    c = rng.random((300, 3)) * 0.03 + np.array([0.0, -0.02, 0.0])
    for i in range(300):
        L = int(rng.integers(3, 40))
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        segs.append(c[i] + np.cumsum(d * 0.0025 + rng.normal(scale=4e-4, size=(L, 3)), 0))
    # long arcs; a partner at the tip whose root lies q points back along the arc, one at the root likewise
    k = 0
    for L in (65, 66, 127, 128, 129, 200, 513, 22, 21, 7, 6):
        for q in (0, 1, 2):
            R = L * 0.00205 / (2 * np.pi) * (1.02 if L > 100 and q == 0 else 4.0)      # nearly closed or a quarter turn
            R = max(R, 0.004)
            ctr = np.array([0.05, 0.0, 0.0]) * rng.normal(size=3) * 0.4 + np.array([0.0, -0.02, 0.0])
            arc = _arc(ctr, R, rng.random() * 6, L, 0.00205, 1000 * trial + k)
            k += 1
            segs.append(arc)
            for end in (1, 0):
                p = arc[-1 - q] if end else arc[q]
                d = (arc[-1] - arc[-2]) if end else (arc[0] - arc[1])
                d /= np.linalg.norm(d)
                n = np.cross(d, rng.normal(size=3))
                n /= np.linalg.norm(n)
                Lp = int(rng.choice((5, 6, 21, 65, 129)))
                part = p + 0.0003 * n + np.outer(np.arange(Lp), d) * 0.0025 + np.outer(np.arange(Lp) ** 2, n) * 2e-5
                segs.append(part if end else part[::-1])       # at the root the partner ends there: root -> tips' list
    # a wide spiral cut into consecutive pieces, long ones between short ones (a long piece next to a long one comes
    # round to its neighbour's far end and is refused by the end rule)
    lens = [513, 2, 200, 3, 129, 5, 128, 6, 127, 7, 66, 20, 65, 21, 64, 22, 63, 2, 200, 6, 64]
    total = sum(lens)
    t = np.arange(total) * (0.0025 / 0.2) + rng.random()
    sp = np.stack([0.2 * np.cos(t), 0.2 * np.sin(t) - 0.02, t * (0.012 / (2 * np.pi)) - 0.02], 1)
    o = 0
    for m, L in enumerate(lens):
        piece = sp[o:o + L]
        segs.append(piece[::-1].copy() if m % 3 == 1 else piece.copy())
        o += L
    # a closed ring of four pieces (a cycle)
    t = np.arange(80) * (2 * np.pi / 80)
    ring = np.stack([0.06 + 0.0025 * 80 / (2 * np.pi) * np.cos(t), -0.05 + 0 * t, 0.0025 * 80 / (2 * np.pi) * np.sin(t)], 1)
    for m in range(4):
        segs.append(ring[20 * m:20 * m + 20].copy())
    # exactly equal end coordinates: fans of segments leaving one point, and a pair of identical partners
    for f in range(6):
        p0 = rng.random(3) * 0.03 + np.array([0.0, -0.02, 0.0])
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        n = np.cross(d, rng.normal(size=3))
        n /= np.linalg.norm(n)
        L = int(rng.choice((5, 6, 7, 20)))
        base = p0 - np.outer(np.arange(L)[::-1], d) * 0.0025             # ends at p0
        segs.append(base)
        for sgn in (1.0, -1.0, 1.0):                                     # the third repeats the first exactly
            segs.append(p0 + np.outer(np.arange(L), d * 0.0025 + sgn * n * 0.0004))
    return segs


def test_seeded_sweep(setup):
    """The whole connection against the restatement above, per trial: end lists, the table of joins, the connected
    strands before the occupancy loop (where no retry happened the returned strand; elsewhere the draws are replayed
    with the same np.random.seed), the fail count and np.random's next value, all exact; smoothing of every connected
    strand within 1 float32 ulp of solveh_banded.  No (segment, end) item is left out: sqrt and divide are correctly
    rounded on both sides and the one fused operation is stated as an exact fma."""
    z, hg, occ, _ = setup
    from monohair_amd.strand_smooth import smooth_strands

    occ_zyx = np.ascontiguousarray(occ[..., 0])
    rng = np.random.default_rng(2024)
    worst, longest = 0, 0
    stats = _stats()
    for trial in range(3):
        segs = _sweep_segments(rng, trial)
        n = len(segs)
        np.random.seed(500 + trial)
        out = hg.find_connect_info([s.copy() for s in segs], 0.005, 0.7)
        nxt = np.random.random()
        lists = _np_lists(segs, 0.005)
        for k in range(4):
            idx, dist, cnt = (t.cpu().numpy() for t in hg._end_lists[k])
            for i in range(n):
                assert np.array_equal(idx[i, :cnt[i]], lists[k][i][0]) and np.array_equal(dist[i, :cnt[i]], lists[k][i][1])
            stats["end_ties"] += sum(len(np.unique(r[1])) < len(r[1]) for r in lists[k])
        # every join passes the nearest-distance rule
        for i in range(n):
            for e in range(2):
                j = int(hg.connect_best[i, e])
                if j < 0:
                    continue
                dd = _np_nearest(segs[i], segs[j])
                ok = (dd < 0.005).sum() < 4 if len(segs[i]) < 6 else (dd < 0.01).sum() <= 6
                assert ok
        np.random.seed(500 + trial)
        table, pre, ref, fail = _rs_connect(segs, 0.005, 0.7, occ_zyx, stats)
        got = np.stack([hg.connect_best, hg.connect_best_type], -1)
        bad = np.argwhere((got != table).any(-1))
        assert len(bad) == 0, "trial %d: joins differ at (segment, end) %s: kernel %s, restatement %s" % (
            trial, bad[:5].tolist(), got[tuple(bad[:5].T)].tolist(), table[tuple(bad[:5].T)].tolist())
        assert len(out) == n
        for i, (o, p, r) in enumerate(zip(out, pre, ref)):
            assert o.dtype == np.float64 and o.shape == p.shape, (trial, i)
            if np.array_equal(r, p):          # accepted at once, or never: returned as connected
                assert np.array_equal(o, p), (trial, i)
            assert np.array_equal(o, r), (trial, i)
        assert hg.connect_fail == fail and nxt == np.random.random()
        assert all(o.shape[0] >= s.shape[0] for o, s in zip(out, segs))
        longest = max(longest, max(o.shape[0] for o in out))
        stats["strand_gt513"] += sum(o.shape[0] > 513 for o in out)
        stats["strand_gt1000"] += sum(o.shape[0] > 1000 for o in out)
        sm = smooth_strands([o.copy() for o in out], 4.0, 2.0, device=DEV)
        for o, s in zip(out, sm):
            ref = _np_smooth(o, 4.0, 2.0).astype(np.float32)
            got = s.astype(np.float32)
            ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
            worst = max(worst, int(ulp.max()))
    print("sweep:", dict(stats), "longest strand", longest)
    print("smoothing: largest float32 difference from solveh_banded: %d ulp" % worst)
    _assert_sweep_reaches(stats)
    assert worst <= 1


_SWEEP_MUST_OCCUR = ("join_gt64", "join_gt128_00", "join_gt128_01", "join_gt128_10", "join_gt128_11", "join_both_long",
                     "count6_late", "count7_late", "short_count3", "short_count4", "end_rule_only_late", "kept_by_dlast",
                     "fallback", "loss_order_differs", "loss_tie", "end_ties", "chain_ge4", "cycle", "strand_gt513",
                     "strand_gt1000", "retried_ok", "exhausted",
                     # the counts of 6 and 7 made by points of the 2nd, 3rd, 4th and 9th 64-point block
                     "count6_block1", "count6_block2", "count6_block3", "count6_block8",
                     "count7_block1", "count7_block2", "count7_block3", "count7_block8")


def _assert_sweep_reaches(stats):
    """every situation the sweep exists for occurred: joins of segments of more than 64 / 128 points in all four end
    pairings, close-point counts of 6 and 7 (3 and 4 for short segments) made by points of a later 64-point block, a
    candidate refused by the end rule alone and one kept because dist[-1] >= lim, a join taken from the tips' list, two
    admissible candidates ordered differently by loss and by distance, equal losses, equal end distances, chains of at
    least four segments, a cycle, strands of more than 513 and 1000 points, retries that succeed and that run out"""
    missing = [k for k in _SWEEP_MUST_OCCUR if stats[k] <= 0]
    assert not missing, missing


# ------------------------------------------------------------------ the end grid, coarsened
def _two_clusters(gap):
    """16 two-point segments in two clusters of 8, the second `gap` away from the first: chains along the diagonal, a tip
    a fifth of the threshold from the next root, every other segment reversed.  All coordinates are multiples of 2^-20,
    so every difference and squared distance is exact and moving a cluster changes no distance inside it."""
    rng = np.random.default_rng(8)
    u = np.ones(3) / np.sqrt(3.0)
    segs = []
    for c in range(2):
        org = np.array([0.0, -0.02, 0.0]) + c * np.asarray(gap)
        for k in range(8):
            a = org + u * (0.004 * k) + rng.normal(scale=1e-4, size=3)
            s = np.stack([a, a + u * 0.003 + rng.normal(scale=1e-4, size=3)])
            segs.append(np.round((s[::-1] if k % 2 else s) * 2.0 ** 20) / 2.0 ** 20)
    return segs


def test_end_tables_on_a_doubled_grid(setup):
    """The doubling branch of grid_dims under mh_end_knn64: with the clusters 1.2 apart the ends' grid would have more
    than 2^20 cells of the threshold's size and is coarsened; 0.02 apart it is not.  On the coarsened grid the end
    tables equal the brute-force float64 k-NN (neighbours in adjacent cells among them), and tables and joins are those
    of the uncoarsened run (same segment order, so the index map is the identity).  The far cluster lies outside the
    reference's 256 x 256 x 192 box: its strands fail the occupancy test without a retry, which no assertion reads."""
    from monohair_amd.hairgrow import grid_dims

    _, hg, _, _ = setup
    thr = 0.005
    far = np.round(np.array([1.0, -1.0, -1.0]) * (1.2 / np.sqrt(3.0)) * 2.0 ** 20) / 2.0 ** 20
    near = np.round(np.array([1.0, -1.0, 0.0]) * (0.02 / np.sqrt(2.0)) * 2.0 ** 20) / 2.0 ** 20
    runs = []
    for gap in (far, near):
        segs = _two_clusters(gap)
        ends = np.concatenate([np.stack([s[0] for s in segs]), np.stack([s[-1] for s in segs])])
        h, dims = grid_dims(ends.max(0) - ends.min(0), thr, 1.0001, len(ends))
        cell = np.floor((ends - ends.min(0)) / h).astype(np.int64)
        np.random.seed(3)
        hg.find_connect_info([s.copy() for s in segs], thr, 0.7)
        lists = _np_lists(segs, thr)
        got, apart = [], 0
        for k in range(4):
            idx, dist, cnt = (t.cpu().numpy() for t in hg._end_lists[k])
            for i in range(16):
                assert np.array_equal(idx[i, :cnt[i]], lists[k][i][0]) and np.array_equal(dist[i, :cnt[i]], lists[k][i][1])
                got.append((idx[i, :cnt[i]].tolist(), dist[i, :cnt[i]].tolist()))
                apart += sum(np.abs(cell[(k // 2) * 16 + i] - cell[(k % 2) * 16 + j]).max() == 1 for j in lists[k][i][0])
        assert all(((r[0] >= 8) == (i >= 8)).all() for k in range(4) for i, r in enumerate(lists[k]))   # inside a cluster
        runs.append((h, apart, got, hg.connect_best.copy(), hg.connect_best_type.copy()))
    (h0, apart0, got0, best0, type0), (h1, _, got1, best1, type1) = runs
    assert h0 >= 2 * thr * 1.0001 and h1 == thr * 1.0001                 # at least one doubling; none
    assert apart0 > 0                                                     # neighbours found in an adjacent coarse cell
    assert sum(len(g[0]) for g in got0) >= 32 and (best0 >= 0).sum() >= 12
    assert got0 == got1 and np.array_equal(best0, best1) and np.array_equal(type0, type1)
