"""Pin the strand-tracing oracle (oracle/hairgrow_oracle.c) against the reference's HairGrowing run on a small
synthetic fitted volume (tools/gen_golden_more.py hairgrow).  CPU only."""
import os

import numpy as np
import torch

import oracle
from conftest import GOLDEN


def load():
    z = np.load(os.path.join(GOLDEN, "hairgrow.npz"))
    occ_xyz, ori_xyz = z["occ"], z["ori"]
    # the readers hand HairGrowing [Z,Y,X] arrays (PMVO_utils.py:86-113)
    vol = oracle.Volume(occ_xyz.transpose(2, 1, 0), ori_xyz.transpose(2, 1, 0, 3))
    assert np.array_equal(vol.vox[..., 3], z["vol_occ_zyx"])
    return z, vol


def jitter(n_calls, seed=77):
    torch.manual_seed(seed)
    return torch.rand(n_calls, 3).numpy()       # == n_calls consecutive torch.rand_like(seedPos) draws


def split(pts, lens):
    o = np.concatenate([[0], np.cumsum(lens)])
    return [pts[o[i]:o[i + 1]] for i in range(len(lens))]


def test_guide_strands_match_reference():
    z, vol = load()
    n_occ = int((vol.vox[..., 3] != 0).sum())
    strands, num_root, flag = oracle.generate_guide_strands(vol, z["scalp_points"], z["scalp_normals"], float(z["thr"]),
                                                            jitter(2 * n_occ))
    assert num_root == int(z["guide_num_root"])
    ref = split(z["guide_pts"], z["guide_len"])
    assert len(strands) == len(ref)
    assert np.array_equal(np.array([len(s) for s in strands]), z["guide_len"])
    assert np.array_equal(np.concatenate(strands), z["guide_pts"])
    assert max(len(s) for s in strands) > 25 and flag.max() >= 3      # long strands and the flag gate are exercised


def test_random_segments_match_reference():
    z, vol = load()
    n_occ = int((vol.vox[..., 3] != 0).sum())
    strands, flag = oracle.randomly_generate_segments(vol, float(z["thr"]), jitter(3 * n_occ))
    assert np.array_equal(np.array([len(s) for s in strands]), z["random_len"])
    assert np.array_equal(np.concatenate(strands), z["random_pts"])


# ---------------------------------------------------------------- long strands, volume borders, W != H != Z
def load_long():
    """tests/golden/strands_long.npz (tools/gen_golden_strands_long.py): the reference's per-seed walks and driver
    outputs on a 64 x 24 x 56 volume whose walks reach both 256-step caps and leave through every face."""
    z = np.load(os.path.join(GOLDEN, "strands_long.npz"))
    G = tuple(int(g) for g in z["trace_shape"])
    occ = np.zeros(G, np.float32)
    occ[tuple(z["trace_occ_nz"].T.astype(np.int64))] = 1
    ori = np.zeros(G + (3,), np.float32)
    ori[tuple(z["trace_ori_nz"].T.astype(np.int64))] = z["trace_ori_nz_val"]
    vol = oracle.Volume(occ.transpose(2, 1, 0), ori.transpose(2, 1, 0, 3))
    assert len({vol.W, vol.H, vol.Z}) == 3
    return z, vol


def test_long_fixture_reaches_caps_and_faces():
    """what the fixture is for, restated on the recorded data so that a regenerated file cannot lose it silently"""
    z, vol = load_long()
    ln, first = z["trace_len"], z["trace_first"]
    nb, nf = 256 - first, first + ln - 257
    assert (ln == 513).any() and ((ln > 0) & (nf == 256) & (nb < 256)).any()
    assert ((ln >= 65) & (ln <= 128)).any() and ((ln >= 129) & (ln <= 192)).any() and ((ln > 256) & (ln < 513)).any()
    dims = np.array([vol.W, vol.H, vol.Z])
    for a in range(3):
        assert (z["trace_pts"][:, a] < 0).any() and (z["trace_pts"][:, a] >= dims[a]).any()
    assert ((z["trace_pts"] > -1) & (z["trace_pts"] < 0)).any()
    assert ((z["trace_seeds"] < 0) | (z["trace_seeds"] >= dims)).any()
    assert (z["scalp_len"] == 257).any() and (z["scalp_len"] == 0).any()
    assert z["guide_len"].max() == 513 and z["random_len"].max() == 513


def test_long_per_seed_walks_match_reference():
    """oracle.trace_seeds / trace_scalp == HairGrowing.trace / traceFromScalp called seed by seed: length, first slot,
    every point, and the seeds the reference answers with False (fewer than 5 points) or None."""
    z, vol = load_long()
    thr = float(z["grow_thr"])
    out, first, ln = oracle.trace_seeds(vol, z["trace_seeds"], thr)
    ref = split(z["trace_pts"], z["trace_len"])
    for i in range(len(ln)):
        if z["trace_len"][i] == 0:
            assert ln[i] < 5, i
            continue
        assert ln[i] == z["trace_len"][i] and first[i] == z["trace_first"][i], i
        assert np.array_equal(out[i, first[i]:first[i] + ln[i]], ref[i]), i
        assert np.array_equal(out[i, 256], z["trace_seeds"][i])
    sp, sl = oracle.trace_scalp(vol, z["scalp_points"], z["scalp_normals"], thr)
    assert np.array_equal(sl, z["scalp_len"])
    ref = split(z["scalp_pts"], z["scalp_len"])
    for i in range(len(sl)):
        assert np.array_equal(sp[i, :sl[i]], ref[i]), i


def test_long_drivers_match_reference():
    z, vol = load_long()
    thr = float(z["grow_thr"])
    n_occ = int((vol.vox[..., 3] != 0).sum())
    strands, num_root, _ = oracle.generate_guide_strands(vol, z["scalp_points"], z["scalp_normals"], thr, jitter(2 * n_occ))
    assert num_root == int(z["guide_num_root"])
    assert np.array_equal(np.array([len(s) for s in strands]), z["guide_len"])
    assert np.array_equal(np.concatenate(strands), z["guide_pts"])
    strands, _ = oracle.randomly_generate_segments(vol, thr, jitter(3 * n_occ))
    assert np.array_equal(np.array([len(s) for s in strands]), z["random_len"])
    assert np.array_equal(np.concatenate(strands), z["random_pts"])


def test_long_index_conversion_truncates():
    """The C oracle's (int)x and the kernels' (int)x agree with the reference's .type(torch.long) on every recorded
    coordinate, the negative ones included: both truncate towards zero.  Out-of-range conversions (|x| >= 2^31, NaN)
    are undefined in C and differ between x86 and the GPU; they cannot occur after <= 256 unit steps from a finite
    seed and are outside the pinned domain, so they are not tested.  This test pins the recorded data's meaning (torch
    against numpy and the C cast); it cannot fail on a change of a kernel or of the oracle, and floor in place of
    truncation would not show after the clamp to 0 either: the walks of the tests above are what hold the kernels."""
    z, _ = load_long()
    for key in ("trace_pts", "scalp_pts", "guide_pts", "random_pts", "trace_seeds"):
        p = z[key]
        assert np.isfinite(p).all() and np.abs(p).max() < 2 ** 20
        t = torch.from_numpy(p).type(torch.long).numpy()
        assert np.array_equal(t, np.trunc(p).astype(np.int64))
        assert np.array_equal(t, p.astype(np.int32))             # the C cast
    assert (z["trace_pts"] < 0).any() and np.any((z["trace_pts"] > -1) & (z["trace_pts"] < 0))
