"""GPU: the scalp diffusion kernels (csrc/hairdiffuse.hip, driven by hairgrow.diffusion_scalp) against the numpy restatement
(tests/scalp_diffusion_np.py, which tests/test_scalp_diffusion_host.py holds to the reference's own run) -- on the golden
cases and on a seeded sweep of small volumes, everything exact, details included: status and step per sample, end points
and end normals, the float64 rows, their unit tangents and voxels, and every element of the returned volumes."""
import os

import numpy as np
import pytest

import scalp_diffusion_np as rs
from conftest import GOLDEN
from test_scalp_diffusion_host import CASES, check_details, expected_volumes, load_case

pytestmark = pytest.mark.gpu


def run_gpu(pts, nrm, ori, occ):
    import torch

    from monohair_amd.hairgrow import diffusion_scalp

    o, c, det = diffusion_scalp(torch.from_numpy(pts), torch.from_numpy(nrm), torch.from_numpy(ori), torch.from_numpy(occ),
                                return_details=True)
    assert o.dtype == torch.float32 and c.dtype == torch.float32 and o.shape == ori.shape and c.shape == occ.shape
    return o.cpu().numpy(), c.cpu().numpy(), {k: (v.cpu().numpy() if hasattr(v, "cpu") else v) for k, v in det.items()}


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


def check_against_restatement(pts, nrm, ori, occ):
    o, c, det = run_gpu(pts, nrm, ori, occ)
    ro, rc, rdet = rs.diffusion_scalp(pts, nrm, ori, occ)
    for k in ("status", "step", "end_point", "first_normal", "last_normal", "total_sample", "total_normal",
              "total_normal_unit"):
        assert same_bits(det[k], rdet[k]), k
    assert np.array_equal(det["voxel"], rdet["voxel"])
    assert det["left_volume"] == int((rdet["status"] == rs.LEFT).sum())
    assert same_bits(c, rc), "occ"
    assert same_bits(o, ro), "ori"
    return rdet


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "scalp_diffusion.npz"))


@pytest.mark.parametrize("tag", CASES)
def test_kernels_match_reference_and_restatement(golden, tag):
    pts, nrm, ori, occ = load_case(golden, tag)
    o, c, det = run_gpu(pts, nrm, ori, occ)
    check_details(golden, tag, det)
    eo, ec = expected_volumes(golden, tag, ori, occ)
    assert np.array_equal(c, ec) and np.array_equal(o, eo)
    check_against_restatement(pts, nrm, ori, occ)


def small_volume(seed, n):
    """a 12x14x16 (Z,Y,X) volume, a third of it hair with random orientations (some of them zero), and n samples anywhere
    in it with random normals: walks end in every way, leaving the volume included"""
    rng = np.random.default_rng(seed)
    Z, Y, X = 12, 14, 16
    hair = rng.random((Z, Y, X)) < (0.1, 0.35)[seed % 2]
    o = rng.normal(size=(3, Z, Y, X))
    o /= np.linalg.norm(o, axis=0, keepdims=True)
    o[:, rng.random((Z, Y, X)) < 0.05] = 0
    occ = hair.astype(np.float32)[None]
    ori = (o * hair[None]).astype(np.float32)
    pts = rs.to_world(rng.random((n, 3)) * np.array([X, Y, Z]) * 0.98 + 0.01)
    d = rng.normal(size=(n, 3))
    nrm = (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(np.float32)
    return pts, nrm, ori, occ


@pytest.mark.parametrize("seed,n", [(0, 1), (1, 64), (2, 65), (3, 257)])
def test_sweep_of_small_volumes(seed, n):
    rdet = check_against_restatement(*small_volume(seed, n))
    if n == 257:
        assert all((rdet["status"] == s).any() for s in range(5))


def test_walk_out_of_a_face_is_a_status_not_a_fault():
    Z, Y, X = 6, 7, 8
    occ = np.zeros((1, Z, Y, X), np.float32)
    ori = np.zeros((3, Z, Y, X), np.float32)
    occ[0, 3, 3, 2] = 1
    ori[:, 3, 3, 2] = (-1, 0, 0)
    pts = rs.to_world(np.array([[6.5, 3.5, 3.5], [4.5, 3.5, 3.5], [6.5, 0.5, 3.5], [6.5, 3.5, 5.5], [0.5, 6.5, 0.5]]))
    nrm = np.array([[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, 0, -1], [-1, 0, 0]], np.float32)   # world y, z point the other way
    rdet = check_against_restatement(pts, nrm, ori, occ)
    assert rdet["status"].tolist() == [rs.LEFT, rs.ACCEPTED, rs.LEFT, rs.LEFT, rs.LEFT]
    assert rdet["step"].tolist() == [2, 2, 2, 1, 2]        # a coordinate in (-1, 0) is still voxel 0


def test_no_accepted_sample_returns_the_volumes_unchanged(golden):
    pts, nrm, ori, occ = load_case(golden, "edge")
    keep = golden["edge_status"] != 0
    o, c, det = run_gpu(pts[keep], nrm[keep], ori, occ)
    assert (det["status"] != 0).all() and det["total_sample"].shape == (0, 3) and det["voxel"].shape == (0, 3)
    assert same_bits(o, ori) and same_bits(c, occ)
    o, c, det = run_gpu(pts[:0], nrm[:0], ori, occ)
    assert same_bits(o, ori) and same_bits(c, occ) and det["status"].shape == (0,)


def test_stage_writes_mat_files_that_read_back_the_result(golden, tmp_path):
    import torch

    from monohair_amd.hairgrow import diffuse_scalp, diffusion_scalp
    from monohair_amd.pmvo_utils import (get_ground_truth_3D_occ, get_ground_truth_3D_ori, points_to_voxel,
                                         save_volume_mat_sparse, voxel_to_points)

    pts, nrm, ori, occ = load_case(golden, "edge")
    save_volume_mat_sparse(str(tmp_path / "Occ3D.mat"), str(tmp_path / "Ori3D.mat"), occ[0], ori.transpose(1, 2, 3, 0))
    assert np.array_equal(get_ground_truth_3D_occ(str(tmp_path / "Occ3D.mat"))[..., 0], occ[0])
    assert np.array_equal(get_ground_truth_3D_ori(str(tmp_path / "Ori3D.mat")), ori.transpose(1, 2, 3, 0))
    # the samples as scalp_samples.npz holds them: voxel units, normals with y and z negated
    pv = points_to_voxel(torch.from_numpy(pts.copy())).type(torch.float)
    nv = torch.from_numpy(nrm * np.array([1, -1, -1], np.float32))
    o, c = diffuse_scalp(str(tmp_path), pv, nv)
    world = voxel_to_points(pv.clone())
    eo, ec, det = diffusion_scalp(world, torch.from_numpy(nrm), torch.from_numpy(ori), torch.from_numpy(occ),
                                  return_details=True)
    assert int((det["status"] == 0).sum()) >= 70
    assert torch.equal(o, eo) and torch.equal(c, ec) and not torch.equal(c.cpu(), torch.from_numpy(occ))
    back_occ = get_ground_truth_3D_occ(str(tmp_path / "Occ3D_diffusion.mat"))
    back_ori = get_ground_truth_3D_ori(str(tmp_path / "Ori3D_diffusion.mat"))
    assert back_occ.dtype == np.float32 and np.array_equal(back_occ[..., 0], c[0].cpu().numpy())
    assert back_ori.dtype == np.float32 and np.array_equal(back_ori, o.permute(1, 2, 3, 0).cpu().numpy())
    import scipy.io

    m = scipy.io.loadmat(str(tmp_path / "Ori3D_diffusion.mat"))["Ori"]
    assert m.dtype == np.float64 and m.shape == (occ.shape[2], occ.shape[3], 3 * occ.shape[1])
