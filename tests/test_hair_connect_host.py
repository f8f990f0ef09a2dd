"""CPU-only: the segment-connection fixture (tests/golden/hair_connect.npz) is consistent with the stage it records --
strands.hair is write_strand of the recorded connected strands after the float64 subtraction of bust_to_origin and the
Laplacian smoothing (restated with scipy's banded solver, whose float32 rounding is what the file pins)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN


def _smooth(s, lap, pos):
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


def _hair(b):
    n = int(np.frombuffer(b[:4], "<u4")[0])
    lens = np.frombuffer(b[8:8 + 2 * n], "<u2").astype(int)
    pts = np.frombuffer(b[8 + 2 * n:], "<f4").reshape(-1, 3)
    assert int(np.frombuffer(b[4:8], "<u4")[0]) == lens.sum() == pts.shape[0]
    return lens, pts


def test_fixture_strands_hair_is_smoothed_recorded_strands(tmp_path):
    pytest.importorskip("scipy")
    from monohair_amd.pmvo_utils import write_strand

    z = np.load(os.path.join(GOLDEN, "hair_connect.npz"))
    lens, pts = _hair(z["seg_hair"].tobytes())
    segs = np.split(pts.astype(np.float64), np.cumsum(lens)[:-1])
    nr = int(z["num_root"])
    out = np.split(z["shell_out_pts"], np.cumsum(z["shell_out_len"])[:-1])
    assert len(out) == len(segs) - nr
    strands = segs[:nr] + [c - z["bust"] for c in out]
    sm = [_smooth(s, 4.0, 2.0) for s in strands]
    write_strand(np.concatenate(sm, 0), str(tmp_path / "strands.hair"), [s.shape[0] for s in sm])
    assert (tmp_path / "strands.hair").read_bytes() == z["strands_hair"].tobytes()


def test_fixture_covers_the_edge_cases():
    z = np.load(os.path.join(GOLDEN, "hair_connect.npz"))
    assert (z["edge_rr_idx"] >= 0).sum(1).max() >= 49                      # a full k = 50 row (self dropped)
    assert ((z["edge_rr_idx"] < 0).all(1) & (z["edge_rt_idx"] < 0).all(1)).any()   # empty lists
    d = z["edge_draws"]
    assert (d == 50).any() and ((d > 0) & (d < 50)).any()                # exhausted and successful retries
    assert int(z["edge_fail"]) > int((d == 50).sum())                     # failures without retries: outside the box
    table = z["edge_table"]
    ring = range(60, 68)
    assert all(table[i, 1, 0] >= 0 for i in ring)                         # the ring joins into a cycle


# ------------------------------------------------------------------ the restatement the GPU sweep compares against
def _occ_zyx(z):
    G = tuple(int(g) for g in z["vol_shape"])
    occ = np.zeros(G, np.float32)
    occ[tuple(z["occ_nz"].T.astype(np.int64))] = 1
    return np.ascontiguousarray(occ.transpose(2, 1, 0))


@pytest.mark.parametrize("tag,seed", [("shell", 1234), ("edge", 99), ("long", 4321)])
def test_numpy_restatement_reproduces_the_reference(tag, seed):
    """The float64 numpy restatement of find_best_connect_strands / connect_segments / the occupancy loop kept in
    test_hair_connect_gpu.py gives the reference's recorded table, connected strands, fail count and next np.random
    value exactly, on the two cases of hair_connect.npz and on the "long" case of strands_long.npz (segments of up to
    513 points, strands of more than 1000); that licenses it as the comparator of the GPU sweep."""
    import test_hair_connect_gpu as T

    if tag == "long":
        z = np.load(os.path.join(GOLDEN, "strands_long.npz"))
        segs, occ, thr, dot = T._long_case(z)
    else:
        z = np.load(os.path.join(GOLDEN, "hair_connect.npz"))
        segs = T._shell_segments(z)[0] if tag == "shell" else T._split(z["edge_in_pts"], z["edge_in_len"])
        occ, thr, dot = _occ_zyx(z), float(z["thr"]), float(z["dot"])
    np.random.seed(seed)
    table, _, out, fail = T._rs_connect(segs, thr, dot, occ, T._stats())
    assert np.random.random() == float(z[tag + "_next_random"])
    assert np.array_equal(table, z[tag + "_table"])
    ref = T._split(z[tag + "_out_pts"], z[tag + "_out_len"])
    assert len(out) == len(ref) and all(np.array_equal(a, b) for a, b in zip(out, ref))
    assert fail == int(z[tag + "_fail"])


def test_sweep_inputs_reach_every_situation():
    """the inputs of the GPU sweep, judged by the restatement alone: every situation the sweep exists for occurs"""
    import test_hair_connect_gpu as T

    z = np.load(os.path.join(GOLDEN, "hair_connect.npz"))
    occ = _occ_zyx(z)
    rng = np.random.default_rng(2024)
    stats = T._stats()
    for trial in range(3):
        segs = T._sweep_segments(rng, trial)
        assert {len(s) for s in segs} >= set(T._SWEEP_LENS)
        np.random.seed(500 + trial)
        _, _, out, _ = T._rs_connect(segs, 0.005, 0.7, occ, stats)
        lists = T._np_lists(segs, 0.005)
        stats["end_ties"] += sum(len(np.unique(r[1])) < len(r[1]) for k in range(4) for r in lists[k])
        stats["strand_gt513"] += sum(o.shape[0] > 513 for o in out)
        stats["strand_gt1000"] += sum(o.shape[0] > 1000 for o in out)
    T._assert_sweep_reaches(stats)


# ------------------------------------------------------------------ the grid under both neighbour searches
def _end_cells_rule(ends, bound):
    """find_connect_info's rule as it stood before grid_dims: float64 ends, slack 1.0001 -> (h, dims)"""
    lo = ends.min(0)
    h = bound * 1.0001
    cap = max(4 * ends.shape[0], 1 << 20)
    while True:
        cell = np.floor((ends - lo) / h).astype(np.int64)
        dims = cell.max(0) + 1
        if int(np.prod(dims)) <= cap:
            return h, [int(d) for d in dims]
        h *= 2.0


def _scalp_rule(lo, hi, thr_dist, M):
    """connect_to_scalp's rule as it stood before grid_dims: float32 extent, slack 1.01 -> (h, dims)"""
    h = thr_dist * 1.01
    while True:
        dims = np.floor((hi - lo).astype(np.float64) / h).astype(np.int64) + 1
        if int(np.prod(dims)) <= max(4 * M, 1 << 20):
            break
        h *= 2.0
    return h, [int(d) for d in dims]


# (extent per axis in units of the radius, number of points, doublings): 2^20 is the cap up to 262144 points, 4n above
_GRID_CASES = [((90.0, 100.0, 80.0), 1000, 0), ((101.7, 103.2, 102.9), 1000, 1), ((700.0, 650.3, 810.9), 1000, 3),
               ((256 / 0.505,) * 3, 200000, 3), ((170.2, 160.0, 150.0), 300000, 1), ((105.0, 104.0, 103.0), 300000, 0)]


@pytest.mark.parametrize("ext,n,doublings", _GRID_CASES)
def test_grid_dims_is_both_former_rules(ext, n, doublings):
    from monohair_amd.hairgrow import grid_dims

    rng = np.random.default_rng(n + doublings)
    cap = max(4 * n, 1 << 20)
    # the segment connection: float64 ends (the box corners among them), slack 1.0001
    r = 0.005
    ends = np.array([-0.31, 0.07, 0.2]) + rng.random((n, 3)) * (np.array(ext) * r)
    ends[0], ends[1] = ends.min(0), np.array([-0.31, 0.07, 0.2]) + np.array(ext) * r
    h, dims = grid_dims(ends.max(0) - ends.min(0), r, 1.0001, n)
    assert (h, dims) == _end_cells_rule(ends, r)
    assert h == r * 1.0001 * 2 ** doublings and h >= r * 1.0001 and int(np.prod(dims)) <= cap
    assert doublings == 0 or int(np.prod(np.floor((ends.max(0) - ends.min(0)) / (h / 2)) + 1)) > cap
    # the scalp attachment: float32 extent widened, slack 1.01
    for r in (0.5, 0.75, 2.0):
        lo = np.array([3.25, 100.1, 17.0], np.float32)
        hi = (lo + np.array(ext) * r).astype(np.float32)
        h, dims = grid_dims((hi - lo).astype(np.float64), r, 1.01, n)
        assert (h, dims) == _scalp_rule(lo, hi, r, n)
        assert h >= r * 1.01 and int(np.prod(dims)) <= cap and h == r * 1.01 * 2 ** round(np.log2(h / (r * 1.01)))
    # the production volume at the first radius: 256 voxels / 0.505 per axis is always coarsened
    assert grid_dims(np.full(3, 256.0), 0.5, 1.01, 1000)[0] > 0.5 * 1.01


def test_pack_strands_round_trip_and_refusals():
    from monohair_amd._lib import MhError
    from monohair_amd.strand_smooth import pack_strands, split_strands

    rng = np.random.default_rng(3)
    strands = [rng.random((L, 3)) for L in (2, 7, 3, 64)]
    for dtype in (np.float64, np.float32):
        pts, offs = pack_strands(strands, dtype, "caller", finite=True)
        assert pts.dtype == dtype and pts.flags["C_CONTIGUOUS"] and pts.shape == (76, 3)
        assert offs.dtype == np.int64 and offs.tolist() == [0, 2, 9, 12, 76]
        back = split_strands(pts, offs)
        assert len(back) == 4 and all(np.array_equal(b, s.astype(dtype)) for b, s in zip(back, strands))
        assert [b.shape[0] for b in split_strands(pts, offs, [3, 1])] == [64, 7]
    pts, offs = pack_strands([], np.float32, "caller")
    assert pts.shape == (0, 3) and offs.tolist() == [0] and split_strands(pts, offs) == []
    for bad in (strands[:1] + [rng.random((1, 3))], strands[:1] + [rng.random((5, 2))], [rng.random(3)]):
        with pytest.raises(MhError, match="^caller: every strand must be"):
            pack_strands(bad, np.float64, "caller")
    nan = [s.copy() for s in strands]
    nan[2][1, 0] = np.nan
    with pytest.raises(MhError, match="^caller: non-finite"):
        pack_strands(nan, np.float64, "caller", finite=True)
    pts, offs = pack_strands(nan, np.float64, "caller")            # smooth_strands' use: no finite check
    assert np.isnan(pts[offs[2] + 1, 0]) and np.isfinite(np.delete(pts, offs[2] + 1, 0)).all()
