"""GPU: the scalp diffusion kernels (csrc/hairdiffuse.hip through hairgrow.diffusion_scalp(return_details=True)) with
every decision ON its bound: the hand-written cases of tests/scalp_diffusion_bound_cases.py against the reference's own
record (tests/golden/scalp_diffusion_bounds.npz: the cases and the cases tiled to 257 samples), and against the numpy
restatement, which tests/test_scalp_diffusion_bounds_host.py holds to that record, at other batch sizes: every case
sample alone, and the batch tiled to 63, 64, 65 and 600 samples, so that case boundaries fall inside a wave and across
blocks.  Compared: status, step, end point, first and last normal, the float64 rows, tangents, unit tangents, voxels and
every element of both returned volumes -- bit for bit, NaN == NaN where a NaN occupancy makes elements NaN."""
import os

import numpy as np
import pytest

import scalp_diffusion_bound_cases as bc
import scalp_diffusion_np as rs
from conftest import GOLDEN
from test_scalp_diffusion_gpu import run_gpu

pytestmark = pytest.mark.gpu
QUANTITIES = ("status", "step", "end_point", "first_normal", "last_normal", "total_sample", "total_normal", "total_normal_unit")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "scalp_diffusion_bounds.npz"))


def check_against_restatement(pts, nrm, ori, occ):
    o, c, det = run_gpu(pts, nrm, ori, occ)
    ro, rc, rdet = rs.diffusion_scalp(pts, nrm, ori, occ)
    acc = rdet["status"] == rs.ACCEPTED
    for k in QUANTITIES:
        got, want = det[k], rdet[k]
        assert bc.same_bits(got, want), k
    assert np.array_equal(det["voxel"], rdet["voxel"]) and det["left_volume"] == 0 and not (rdet["status"] == rs.LEFT).any()
    assert bc.same_bits(c, rc), "occ"
    assert bc.same_bits(o, ro), "ori"
    return acc


@pytest.mark.parametrize("tag", ("cases", "tiled"))
def test_recorded_batches_equal_the_reference(golden, tag):
    pts, nrm, ori, occ = bc.load(golden, tag)
    res = run_gpu(pts, nrm, ori, occ)
    bc.check_record(golden, tag, res)
    assert np.isnan(res[1]).sum() == 1 and np.isnan(res[0]).sum() == 3          # the one voxel whose occupancy is NaN
    check_against_restatement(pts, nrm, ori, occ)


def test_every_case_sample_alone(golden):
    pts, nrm, ori, occ = bc.load(golden, "cases")
    accepted = 0
    for i in range(len(pts)):
        accepted += int(check_against_restatement(pts[i:i + 1], nrm[i:i + 1], ori, occ)[0])
    assert accepted == int((golden["cases_status"] == 0).sum())


@pytest.mark.parametrize("n", (63, 64, 65, 600))
def test_batch_tiled_to_other_sizes(golden, n):
    pts, nrm, ori, occ = bc.load(golden, "cases")
    idx = np.arange(n) % len(pts)
    acc = check_against_restatement(pts[idx], nrm[idx], ori, occ)
    assert acc.sum() > n // 2
