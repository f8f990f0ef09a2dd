"""CPU only: the numpy restatement of the scalp diffusion (tests/scalp_diffusion_np.py) held to the reference's own run of
diffusion_scalp (tests/golden/scalp_diffusion.npz, tools/gen_golden_diffusion.py) on every recorded quantity, all exact:
status, step and restarts per sample, end points and end normals, the float64 rows (scipy's Hermite evaluation and the
forward differences), the voxel of every row, and the returned volumes -- the voxels the reference changed with their
values, and nothing else changed."""
import collections
import os

import numpy as np
import pytest

import scalp_diffusion_np as rs
from conftest import GOLDEN

CASES = ("shell", "edge", "one")


def load_case(z, tag):
    """(points, normals, ori [3,Z,Y,X], occ [1,Z,Y,X]) float32 from the compact record"""
    Z, Y, X = (int(v) for v in z[tag + "_shape"])
    nz = z[tag + "_occ_nz"].astype(np.int64)
    occ = np.zeros((1, Z, Y, X), np.float32)
    ori = np.zeros((3, Z, Y, X), np.float32)
    occ[0, nz[:, 0], nz[:, 1], nz[:, 2]] = 1
    ori[:, nz[:, 0], nz[:, 1], nz[:, 2]] = z[tag + "_ori_nz"].T
    return z[tag + "_points"], z[tag + "_normals"], ori, occ


def expected_volumes(z, tag, ori, occ):
    """the reference's returned volumes: the input with the recorded changed voxels replaced"""
    ch = z[tag + "_changed"].astype(np.int64)
    o, c = ori.copy(), occ.copy()
    o[:, ch[:, 0], ch[:, 1], ch[:, 2]] = z[tag + "_changed_ori"].T
    c[0, ch[:, 0], ch[:, 1], ch[:, 2]] = z[tag + "_changed_occ"]
    return o, c


def check_details(z, tag, det):
    """per-sample and per-row quantities of a run (restatement or kernels) against the record, exact"""
    assert np.array_equal(det["status"], z[tag + "_status"]) and np.array_equal(det["step"], z[tag + "_step"])
    acc = z[tag + "_status"] == 0
    for k in ("end_point", "first_normal", "last_normal"):
        got = np.asarray(det[k])
        assert got.dtype == np.float32 and np.array_equal(got[acc], z["%s_%s" % (tag, k)][acc]), k
    assert np.array_equal(np.asarray(det["voxel"], np.int64), z[tag + "_voxel"])
    for k in ("total_sample", "total_normal"):
        got = np.asarray(det[k])
        assert got.dtype == np.float64 and np.array_equal(got, z["%s_%s" % (tag, k)]), k


def check_case(z, tag, case, res=None):
    stats = collections.defaultdict(int)
    pts, nrm, ori, occ = case
    if res is None:
        res = rs.diffusion_scalp(pts, nrm, ori, occ, stats)
        assert np.array_equal(res[2]["restarts"], z[tag + "_restarts"])
    o, c, det = res
    check_details(z, tag, det)
    eo, ec = expected_volumes(z, tag, ori, occ)
    assert o.dtype == np.float32 and c.dtype == np.float32
    assert np.array_equal(c, ec), "occ"
    assert np.array_equal(o, eo), "ori"
    return res, stats


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "scalp_diffusion.npz"))


@pytest.mark.parametrize("tag", CASES)
def test_restatement_matches_reference(golden, tag):
    _, stats = check_case(golden, tag, load_case(golden, tag))
    for k in ("cos_near", "boundary_near", "zero_tangent", "rows_outside"):
        assert stats[k] == 0, k


def test_cases_reach_every_family(golden):
    z = golden
    st = z["shell_status"]
    assert all((st == s).any() for s in (0, 1, 2, 3)) and len(st) > 256
    r = z["shell_restarts"][st == 0]
    assert r.min() == 0 and r.max() >= 2
    stats = collections.defaultdict(int)
    rs.diffusion_scalp(*load_case(z, "shell"), stats)
    assert all(stats[k] > 0 for k in ("accept_pos_first", "accept_neg_first", "accept_pos_restarted"))
    e = {k[len("edge_expect_"):]: z[k] for k in z.files if k.startswith("edge_expect_")}
    st, sp = z["edge_status"], z["edge_step"]
    assert sp[e["step1"][0]] == 1 and sp[e["step9"][0]] == 9 and st[e["ten_steps"][0]] == 2
    assert st[e["zero_orientation"][0]] == 3 and st[e["inside"][0]] == 1 and st[e["minus_grow_dir"][0]] == 0
    assert (z["edge_voxel"][:, 0] == 0).any() and (z["edge_total_sample"][:, 0] < -0.32).any()   # (-1, 0) truncates to 0
    _, cnt = np.unique(z["edge_voxel"], axis=0, return_counts=True)
    assert cnt.max() > 64 and (cnt >= 3).sum() >= 2
    assert len(z["one_points"]) == 1 and z["one_status"][0] == 0


def test_no_accepted_sample_returns_the_volumes_unchanged(golden):
    pts, nrm, ori, occ = load_case(golden, "edge")
    keep = golden["edge_status"] != 0
    o, c, det = rs.diffusion_scalp(pts[keep], nrm[keep], ori, occ)
    assert keep.sum() >= 3 and (det["status"] != 0).all() and len(det["total_sample"]) == 0
    assert np.array_equal(o, ori) and np.array_equal(c, occ)
