"""GPU: the scalp attachment (csrc/hairscalp.hip, HairGrowing.connect_to_scalp, hairgrow.connect_scalp) against the
reference's own run (tests/golden/hair_scalp.npz, tools/gen_golden_scalp.py) and, on a seeded sweep, against the numpy
restatement of tests/test_hair_scalp_host.py (which that file holds to the same recorded run)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN
from test_hair_scalp_host import case_inputs, check_recorded, load_volume, rs_connect, similar_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def setup():
    from monohair_amd.hairgrow import HairGrowing

    z = np.load(os.path.join(GOLDEN, "hair_scalp.npz"))
    zc = np.load(os.path.join(GOLDEN, "hair_connect.npz"))
    occ, ori, vox = load_volume(zc)
    return z, zc, HairGrowing(None, None, device=DEV, occ=occ, ori=ori), occ, ori, vox


def _run(hg, strands, num_root, ratio):
    ret = hg.connect_to_scalp([s.copy() for s in strands], num_root, ratio)
    return dict(passes=hg.scalp_passes, root=hg.scalp_root_flag, out=hg.scalp_out_flag, out_ratio=hg.scalp_out_ratio,
                flips=hg.scalp_flips, choice=hg.scalp_choice, similar=hg.scalp_similar, returned=ret)


@pytest.mark.parametrize("tag", ["shell", "edge"])
def test_connect_to_scalp_matches_reference(setup, tag):
    z, zc, hg, _, _, _ = setup
    res = _run(hg, case_inputs(z, zc, tag), int(z[tag + "_num_root"]), float(z[tag + "_ratio_thr"]))
    check_recorded(z, tag, res)
    joined = z[tag + "_choice"][:, 0] >= 0
    assert similar_close(res["similar"][joined], z[tag + "_similar"][joined])


def test_connect_scalp_writes_reference_connected_strands_hair(setup, tmp_path):
    from monohair_amd.hairgrow import connect_scalp

    z, zc, _, occ, ori, _ = setup
    (tmp_path / "strands.hair").write_bytes(zc["strands_hair"].tobytes())
    np.save(tmp_path / "num_root.npy", np.array(int(zc["num_root"])))
    connect_scalp(str(tmp_path), zc["bust"], float(z["shell_ratio_thr"]), device=DEV, occ=occ, ori=ori)
    assert (tmp_path / "connected_strands.hair").read_bytes() == z["connected_strands_hair"].tobytes()


# ------------------------------------------------------------------ seeded sweep against the restatement
def _line(p0, d, n, rng, step=1.0):
    d = np.asarray(d, np.float64)
    p = np.asarray(p0, np.float64) + np.outer(np.arange(n) * step, d / np.linalg.norm(d))
    return (p + rng.normal(scale=2e-3, size=p.shape)).astype(np.float32)


def _sweep_strands(rng):
    """rooted and floating strands of 2, 64, 65 and 513 points around the occupied shell (centre (128, 128, 96), radius
    10) and away from it; a bundle of 40 rooted strands within 0.4 of one axis, so that a floating start sees more than 30
    distinct strands and, at the wider radii, more than 64 core points."""
    roots, floats = [], []
    c = np.array([128.0, 128.0, 96.0])
    for n in (2, 64, 65, 513, 30, 30, 30, 30):
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        t = np.cross(u, rng.normal(size=3))
        t /= np.linalg.norm(t)
        p0 = c + u * 10.0 - t * min(n, 40) / 2       # tangent to the shell
        r = _line(p0, t, n, rng, 1.0 if n > 2 else 3.0)
        roots.append(r)
        for m in (2, 64, 65, 513):
            k = int(rng.integers(0, n))
            w = np.cross(t, rng.normal(size=3))
            w /= np.linalg.norm(w)
            d = t * 3.0 + w * rng.uniform(0.5, 2.5)
            floats.append(_line(r[k].astype(np.float64) + w * rng.uniform(0.1, 1.8), d, m, rng, 0.25 * np.linalg.norm(d)))
    for a in range(40):
        ang = 2 * np.pi * a / 40
        roots.append(_line([60.0, 60.0 + 0.4 * np.cos(ang), 60.0 + 0.4 * np.sin(ang)], [1, 0, 0], 14, rng))
    for k in range(6):
        floats.append(_line([63.0 + k, 60.0 + 0.2 * k, 60.0], [3.0, 1.0 + 0.3 * k, 0.2], 5 + k, rng, 3.3))
    # runs against its neighbour with its start further along it than its end: reversed by the flip test
    roots.append(_line([60.0, 90.0, 60.0], [1, 0, 0], 14, rng))
    floats.append(_line([68.0, 90.3, 60.0], [-3.0, 1.0, 0.0], 4, rng, 3.2))
    # at too wide an angle to join: still floating at the widest radius, where its ball holds more than 64 core points
    floats.append(_line([66.0, 60.9, 60.0], [3.0, 5.0, 0.0], 6, rng, 5.8))
    return roots + floats, len(roots)


def _compare(hg, vox, strands, num_root, ratio):
    ref = rs_connect(strands, num_root, vox, ratio)
    st = ref["stats"]
    for k in ("nearest_ties", "loss_ties", "similar_near_0.3", "mean_near_5", "dist_near_thr"):
        assert st[k] == 0, k                       # no exact tie, no decision within rounding of its threshold
    got = _run(hg, strands, num_root, ratio)
    assert got["passes"] == ref["passes"]
    for k in ("root", "out", "out_ratio", "flips", "choice"):
        assert np.array_equal(got[k], ref[k]), k
    assert len(got["returned"]) == len(ref["returned"])
    for a, b in zip(got["returned"], ref["returned"]):
        assert a.dtype == np.float32 and np.array_equal(a, b)
    return st


def test_seeded_sweep_matches_restatement(setup):
    _, _, hg, _, _, vox = setup
    rng = np.random.default_rng(77)
    strands, num_root = _sweep_strands(rng)
    lens = {len(s) for s in strands[:num_root]}, {len(s) for s in strands[num_root:]}
    assert {2, 64, 65, 513} <= lens[0] and {2, 64, 65, 513} <= lens[1]
    st = _compare(hg, vox, strands, num_root, 0.1)
    assert st["ball_distinct_>30"] > 0 and st["ball_gt64"] > 0 and st["stopped_at_30"] > 0 and st["joined"] > 0
    assert st["flipped"] > 0


def test_one_cell_grid_and_no_floating_strand(setup):
    _, _, hg, _, _, vox = setup
    rng = np.random.default_rng(5)
    root = [np.array([[100.0, 100.0, 100.0], [100.2, 100.1, 100.0]], np.float32)]     # extent below one cell
    floats = [_line([100.1, 100.3, 100.0], [3.0, 1.0, 0.0], 4, rng, 3.2), _line([140.0, 100.0, 100.0], [1, 0, 0], 3, rng)]
    _compare(hg, vox, root + floats, 1, 0.0)
    got = _run(hg, root, 1, 0.0)                   # nothing floats: every pass is empty, the thresholds widen to the end
    assert len(got["returned"]) == 1 and got["passes"][-1][:2] == (2.0, 0.6) and len(got["passes"]) == 7


def test_no_rooted_strand_raises(setup):
    from monohair_amd._lib import MhError

    _, _, hg, _, _, _ = setup
    with pytest.raises(MhError):
        hg.connect_to_scalp([np.zeros((3, 3), np.float32) + np.arange(3, dtype=np.float32)[:, None]], 0, 0.0)
    with pytest.raises(MhError):
        hg.connect_to_scalp([], 0, 0.0)


def _face_case(cells):
    """a rooted strand whose grid at radius 0.5 has `cells` cells along x (1: the extent is below one cell), and floating
    strands that start exactly on a face of its cells, one float32 below it, and at the grid's origin"""
    from test_knn_paths_gpu import _first_in_cell

    rng = np.random.default_rng(6)
    root = (np.array([[100.0, 100.0, 100.0], [100.2, 100.1, 100.0]], np.float32) if cells == 1 else
            _line([100.0, 100.0, 100.0], [1, 0, 0], 40, rng, 0.25))
    lo = root.min(0)
    starts = [lo.copy()]
    for k in (1,) if cells == 1 else (1, 2, 7):
        on = np.array([_first_in_cell(lo[0], np.float32(0.505), k), lo[1] + np.float32(0.05), lo[2]], np.float32)
        starts += [on, np.array([np.nextafter(on[0], np.float32(-np.inf)), on[1], on[2]], np.float32)]
    floats = []
    for p in starts:
        s = _line(p, [3.0, 1.0, 0.2], 4, rng, 3.2)
        s[0] = p
        floats.append(s)
    return [root] + floats, starts


@pytest.mark.parametrize("cells", [20, 1])
def test_ball_of_a_start_on_a_cell_face(setup, cells):
    """The cell formula under the scalp balls (mh_grid_cell): for strands that start on a cell face of the core grid --
    in the one-cell grid its far face, where the clamp decides -- one float32 below it and at the origin, the first
    pass's balls have the size of scipy's query_ball_point, and the attachment (which orders and uses the balls' members)
    equals the restatement."""
    import torch
    import types
    from scipy.spatial import KDTree

    from monohair_amd import _lib
    from monohair_amd._lib import host_ptr as _hp
    from monohair_amd.hairgrow import grid_dims
    from monohair_amd.strand_smooth import pack_strands

    _, _, hg, _, _, vox = setup
    strands, starts = _face_case(cells)
    core = strands[0]
    h, dims = grid_dims((core.max(0) - core.min(0)).astype(np.float64), 0.5, 1.01, len(core))
    assert np.float32(h) == np.float32(0.505) and dims == [cells, 1, 1]
    q = np.floor((np.stack(starts)[:, 0] - core.min(0)[0]) / np.float32(h))              # in float32, as the kernel
    assert q.tolist() == ([0, 1, 0] if cells == 1 else [0, 1, 0, 2, 1, 7, 6])
    pts, offs = pack_strands(strands, np.float32, "test")
    flags = np.zeros(len(strands), np.uint8)
    flags[0] = 1
    s = types.SimpleNamespace(P=torch.from_numpy(pts).to(DEV), offs=torch.from_numpy(offs).to(DEV),
                              flags=torch.from_numpy(flags).to(DEV))
    c = hg._scalp_core(s)
    hg._scalp_grid(c, 0.5)
    assert c.dims.tolist() == dims
    act = torch.arange(1, len(strands), dtype=torch.int32, device=DEV)
    bcnt = torch.empty(len(starts), dtype=torch.int64, device=DEV)
    _lib.check(_lib.lib().mh_scalp_ball_count(hg._ctx, _lib.ptr(s.P), _lib.ptr(s.offs), _lib.ptr(act), len(starts),
                                              _lib.ptr(c.pts), c.M, _lib.ptr(c.order), _lib.ptr(c.cstart), _hp(c.grid),
                                              _hp(c.dims), 0.5, _lib.ptr(bcnt), _lib.stream_ptr()), "mh_scalp_ball_count")
    tree = KDTree(core.astype(np.float64))
    ref = [len(tree.query_ball_point(p.astype(np.float64), 0.5)) for p in starts]
    assert bcnt.cpu().tolist() == ref and min(ref) >= 1
    _compare(hg, vox, strands, 1, 0.0)
