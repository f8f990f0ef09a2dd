"""GPU: the one strand lookup of the strand tools (csrc/mh_strands.h: mh_strand_of) on strand sets that sit on its edges,
through the three tools whose kernels use it -- strand_tangents (csrc/hairmetrics.hip), voxelize_strands on an 8 x 8 x 8 grid
(csrc/hairvolume.hip) and capture_planes at 16 x 16 with one view (csrc/haircapture.hip) -- against the numpy restatements
the suite already has (tests/hair_metrics_np.py, tests/hair_volume_np.py, tests/hair_capture_np.py): every quantity EQUAL.
All three restatements accept empty strands and the empty set (checked on the CPU), so no input is dropped from any tool."""
import functools

import numpy as np
import pytest

import hair_capture_np
import hair_metrics_np
import hair_volume_np

pytestmark = pytest.mark.gpu

H = W = 16
DIMS, VS, VMIN, BUST = (8, 8, 8), 0.02, (-0.08, -0.08, -0.08), (0.0, 0.0, 0.0)      # the grid covers the head: |x| <= 0.08


def _curve(n, seed):
    """n points of a seeded curve around the synthetic head (radius 0.1), float32 [n,3]: steps of a few millimetres"""
    rng = np.random.default_rng(seed)
    t = np.linspace(0.0, 1.0, n)[:, None] if n > 1 else np.zeros((1, 1))
    a, b = rng.uniform(-0.06, 0.06, 3), rng.uniform(-0.06, 0.06, 3)
    swing = 0.015 * np.concatenate([np.cos(9.0 * t), np.sin(7.0 * t), np.cos(5.0 * t + 1.0)], 1)
    return (a[None, :] * (1.0 - t) + b[None, :] * t + swing).astype(np.float32)


SETS = {
    # empty strands in front of, between and behind the others, and a strand of one point
    "empty strands": [1, 0, 0, 2, 1, 0, 3, 0],
    # one strand across the border between two workgroups of the kernels with one lane per point
    "257 points": [257],
    "nothing": [],
}


@functools.lru_cache(maxsize=None)
def _set(name):
    counts = np.array(SETS[name], np.int64)
    pts = [_curve(int(c), 10 + i) for i, c in enumerate(counts) if c]
    return counts, np.concatenate(pts) if pts else np.zeros((0, 3), np.float32)


@pytest.mark.parametrize("name", list(SETS))
def test_tangents(name):
    from monohair_amd import hairmetrics

    counts, pts = _set(name)
    want_t, want_v = hair_metrics_np.tangents(counts, pts)
    got_t, got_v = hairmetrics.strand_tangents(counts, pts)
    assert got_t.dtype == np.float64 and got_v.dtype == np.uint8 and got_t.shape == want_t.shape
    assert np.array_equal(got_v, want_v)
    assert got_t.tobytes() == want_t.tobytes()
    if name == "empty strands":
        assert list(got_v) == [0, 1, 1, 0, 1, 1, 1]       # the strands of one point have no direction


@pytest.mark.parametrize("name", list(SETS))
def test_volume(name):
    from monohair_amd import hairvolume

    counts, pts = _set(name)
    want = hair_volume_np.voxelize(counts, pts, BUST, VMIN, VS, DIMS, 2)
    got = hairvolume.voxelize_strands((counts, pts), BUST, VMIN, VS, DIMS, 2, return_details=True)
    assert got["dropped_segments"] == want["dropped_segments"] == 0 and got["outside_samples"] == want["outside_samples"]
    for k in ("voxels", "cnt", "sums", "coh", "ori"):
        assert got[k].dtype == want[k].dtype and got[k].tobytes() == want[k].tobytes(), k
    # a segment from the last point of a strand to the first of the next would add samples: the counts are the strands' own
    assert got["samples"] == int(want["cnt"].sum()) and (got["samples"] > 0) == (len(pts) > 1)


@pytest.mark.parametrize("name", list(SETS))
def test_capture(name):
    from monohair_amd import synth, synth_hair
    from monohair_amd.camera import cameras_from_list

    counts, pts = _set(name)
    cams = cameras_from_list(synth.make_cameras(1, H, W))
    depth, ori, conf, mask, details = synth_hair.capture_planes((counts, pts), cams, H, W, return_details=True)
    fused = synth_hair.capture_planes((counts, pts), cams, H, W)
    got = dict(depth=depth, ori_u8=ori, conf_u8=conf, mask_u8=mask)
    for k, f in zip(got, fused):
        assert got[k].cpu().numpy().tobytes() == f.cpu().numpy().tobytes(), k      # the one-call form is the four steps
    det = details[0]
    vert, valid = det["vert"].cpu().numpy(), det["valid"].cpu().numpy()
    assert valid.all() and vert.shape == (len(pts), 3)
    want = hair_capture_np.capture(vert, valid, counts, H, W)
    got.update({k: det[k] for k in ("zmin", "cnt", "c2", "s2")})
    assert det["dropped"] == want["dropped"] == 0
    for k, g in got.items():
        g = g.cpu().numpy()[0] if k in ("depth", "ori_u8", "conf_u8", "mask_u8") else g.cpu().numpy()
        assert g.dtype == want[k].dtype and g.shape == want[k].shape and g.tobytes() == want[k].tobytes(), k
    assert want["mask_u8"].any() == (len(pts) > 1)
