"""GPU: segment connection and smoothing (csrc/hairconnect.hip, HairGrowing.find_connect_info, strand_smooth,
connect_segments) against the reference's own run (tests/golden/hair_connect.npz, tools/gen_golden_connect.py) and a
float64 numpy restatement kept here."""
import os

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


def _check_case(z, hg, tag, segs, seed):
    np.random.seed(seed)
    out = hg.find_connect_info([s.copy() for s in segs], float(z["thr"]), float(z["dot"]))
    nxt = np.random.random()
    table = np.stack([hg.connect_best, hg.connect_best_type], -1)
    assert np.array_equal(table, z[tag + "_table"])
    ref = _split(z[tag + "_out_pts"], z[tag + "_out_len"])
    assert len(out) == len(ref)
    for a, b in zip(out, ref):
        assert a.dtype == np.float64 and np.array_equal(a, b)
    assert hg.connect_fail == int(z[tag + "_fail"])
    assert nxt == float(z[tag + "_next_random"])


def test_end_tables_match_reference(setup):
    z, hg, _, _ = setup
    for tag, segs in (("shell", _shell_segments(z)[0]), ("edge", _split(z["edge_in_pts"], z["edge_in_len"]))):
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


def test_seeded_sweep(setup):
    z, hg, _, _ = setup
    from monohair_amd.strand_smooth import smooth_strands

    rng = np.random.default_rng(2024)
    worst = 0
    for trial in range(3):
        n = 300
        c = rng.random((n, 3)) * 0.03 + np.array([0.0, -0.02, 0.0])
        segs = []
        for i in range(n):
            L = int(rng.integers(3, 40))
            d = rng.normal(size=3)
            d /= np.linalg.norm(d)
            segs.append(c[i] + np.cumsum(d * 0.0025 + rng.normal(scale=4e-4, size=(L, 3)), 0))
        out = hg.find_connect_info(segs, 0.005, 0.7)
        lists = _np_lists(segs, 0.005)
        for k in range(4):
            idx, dist, cnt = (t.cpu().numpy() for t in hg._end_lists[k])
            for i in range(n):
                assert np.array_equal(idx[i, :cnt[i]], lists[k][i][0]) and np.array_equal(dist[i, :cnt[i]], lists[k][i][1])
        # every join passes the nearest-distance rule, and chain lengths add up
        for i in range(n):
            for e in range(2):
                j = int(hg.connect_best[i, e])
                if j < 0:
                    continue
                dd = _np_nearest(segs[i], segs[j])
                ok = (dd < 0.005).sum() < 4 if len(segs[i]) < 6 else (dd < 0.01).sum() <= 6
                assert ok
        assert len(out) == n and all(o.shape[0] >= s.shape[0] for o, s in zip(out, segs))
        sm = smooth_strands([o.copy() for o in out], 4.0, 2.0, device=DEV)
        for o, s in zip(out, sm):
            ref = _np_smooth(o, 4.0, 2.0).astype(np.float32)
            got = s.astype(np.float32)
            ulp = np.abs(got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
            worst = max(worst, int(ulp.max()))
    print("smoothing: largest float32 difference from solveh_banded: %d ulp" % worst)
    assert worst <= 1
