"""CPU: the strand-volume and volume-score rules (include/mh_pmvo.h, "Strand volume" / "Volume scores") as
tests/hair_volume_np.py restates them, against cases worked out by hand.  The grid of these cases has voxel_min 0 and voxel
size 1, so a world point (x, y, z) has the voxel coordinate (x, -y, -z) and every number below is exact."""
import numpy as np
import pytest

import hair_volume_np as hv

VMIN, VS, ZERO = (0.0, 0.0, 0.0), 1.0, (0.0, 0.0, 0.0)
Q2 = 4096 * 4096


def _vox(counts, pts, dims=(8, 9, 10), sub=2, bust=ZERO):
    return hv.voxelize(counts, np.array(pts, np.float32), bust, VMIN, VS, dims, sub)


def test_strand_along_x_through_voxel_centres():
    r = _vox([2], [[1, -2, -3], [5, -2, -3]])
    # n = 8 samples at x = 1.25, 1.75, ..., 4.75
    assert r["voxels"].tolist() == [[1, 2, 3], [2, 2, 3], [3, 2, 3], [4, 2, 3], [5, 2, 3]]
    assert r["cnt"].tolist() == [1, 2, 2, 2, 1]
    assert r["sums"].tolist() == [[c * Q2, 0, 0, 0, 0, 0] for c in (1, 2, 2, 2, 1)]
    assert r["ori"].tolist() == [[1.0, 0.0, 0.0]] * 5 and r["ori"].dtype == np.float32
    assert r["coh"].tolist() == [1.0] * 5
    assert (r["dropped_segments"], r["outside_samples"]) == (0, 0)


def test_world_plus_y_is_stored_with_negative_y_and_the_voxel_y_falls():
    r = _vox([2], [[2, -5, -3], [2, -1, -3]], sub=1)          # along world +y: voxel y runs from 5 down to 1
    # n = 4 samples at voxel y = 4.5, 3.5, 2.5, 1.5 -> 4, 4, 2, 2 (half to even)
    assert r["voxels"].tolist() == [[2, 2, 3], [2, 4, 3]] and r["cnt"].tolist() == [2, 2]
    assert r["sums"].tolist() == [[0, 2 * Q2, 0, 0, 0, 0]] * 2
    assert np.array_equal(r["ori"], np.array([[0, -1, 0]] * 2, np.float32))
    w, g, valid = hv.voxel_coords(np.array([[2, -5, -3], [2, -1, -3]], np.float32), ZERO, VMIN, VS)
    assert g[:, 1].tolist() == [5.0, 1.0] and valid.all()


def test_two_perpendicular_strands_keep_the_first_largest_diagonal():
    r = _vox([2, 2], [[2.5, -2, -3], [3.5, -2, -3], [3, -2, -2.5], [3, -2, -3.5]], sub=1)
    assert r["voxels"].tolist() == [[3, 2, 3]] and r["cnt"].tolist() == [2]
    assert r["sums"].tolist() == [[Q2, 0, Q2, 0, 0, 0]]
    assert r["ori"].tolist() == [[1.0, 0.0, 0.0]] and r["coh"].tolist() == [0.5]


def test_sample_on_a_half_goes_to_the_even_voxel():
    r = _vox([3], [[2, -2, -3], [3, -2, -3], [4, -2, -3]], sub=1)      # samples at x = 2.5 and 3.5
    assert r["voxels"].tolist() == [[2, 2, 3], [4, 2, 3]] and r["cnt"].tolist() == [1, 1]


def test_samples_outside_each_face_are_counted_not_clamped():
    dims = (4, 5, 6)
    outside = [(-1, 2, 2), (4, 2, 2), (2, -1, 2), (2, 5, 2), (2, 2, -1), (2, 2, 6)]
    for v in outside:
        p = [v[0], -v[1], -v[2]]
        r = _vox([2], [p, p], dims=dims)
        assert len(r["voxels"]) == 0 and r["outside_samples"] == 1, v
    pts = [[v[0], -v[1], -v[2]] for v in outside for _ in (0, 1)]
    r = _vox([2] * 6, pts, dims=dims)
    assert len(r["voxels"]) == 0 and r["outside_samples"] == 6 and r["dropped_segments"] == 0
    # the voxels just inside the same faces are kept
    inside = [(0, 2, 2), (3, 2, 2), (2, 0, 2), (2, 4, 2), (2, 2, 0), (2, 2, 5)]
    r = _vox([2] * 6, [[v[0], -v[1], -v[2]] for v in inside for _ in (0, 1)], dims=dims)
    assert sorted(r["voxels"].tolist()) == sorted(list(v) for v in inside) and r["outside_samples"] == 0


def test_segments_of_8192_and_8193_samples():
    dims = (8, 8, 520)
    r = _vox([2], [[1, -1, 0], [1, -1, -512]], dims=dims, sub=16)               # 16 * 512 = 8192 samples
    assert r["dropped_segments"] == 0 and int(r["cnt"].sum()) == 8192
    assert r["voxels"].tolist() == [[1, 1, z] for z in range(513)]
    assert r["cnt"].tolist() == [8] + [16] * 511 + [8]
    # (the strand runs along world -z; an axis has no sign, and only y > 0 flips it)
    assert np.array_equal(r["ori"], np.array([[0, 0, 1]] * 513, np.float32))
    r = _vox([2], [[1, -1, 0], [1, -1, -512.0625]], dims=dims, sub=16)          # 16 * 512.0625 = 8193
    assert r["dropped_segments"] == 1 and len(r["voxels"]) == 0 and r["outside_samples"] == 0


def test_zero_length_segment_occupies_without_a_direction():
    r = _vox([2], [[3, -2, -3], [3, -2, -3]])
    assert r["voxels"].tolist() == [[3, 2, 3]] and r["cnt"].tolist() == [1]
    assert r["sums"].tolist() == [[0] * 6] and r["ori"].tolist() == [[0.0, 0.0, 0.0]] and r["coh"].tolist() == [0.0]


def test_bust_to_origin_moves_the_strand():
    a = _vox([2], [[1, -2, -3], [5, -2, -3]])
    b = _vox([2], [[0.5, 0, -4], [4.5, 0, -4]], bust=(0.5, -2.0, 1.0))
    for k in ("voxels", "ori", "cnt", "coh", "sums"):
        assert np.array_equal(a[k], b[k]), k


def test_one_point_and_empty_strands_make_nothing():
    r = _vox([1, 0, 1], [[1, -2, -3], [5, -2, -3]])
    assert len(r["voxels"]) == 0 and r["ori"].shape == (0, 3) and (r["dropped_segments"], r["outside_samples"]) == (0, 0)
    r = _vox([], np.zeros((0, 3)))
    assert len(r["voxels"]) == 0


def test_nan_vertex_breaks_its_two_segments_only():
    nan = float("nan")
    r = _vox([5], [[1, -2, -3], [2, -2, -3], [nan, -2, -3], [5, -2, -3], [6, -2, -3]], sub=1)
    # segments 0-1 (sample at 1.5 -> 2) and 3-4 (5.5 -> 6) remain
    assert r["voxels"].tolist() == [[2, 2, 3], [6, 2, 3]] and r["cnt"].tolist() == [1, 1]
    r = _vox([3], [[1, -2, -3], [2, float("inf"), -3], [3, -2, -3]], sub=1)
    assert len(r["voxels"]) == 0 and r["dropped_segments"] == 0


# ---- scores
DIMS = (5, 6, 7)
REACH, COS2 = [0, 1, 1], [-1.0, -1.0, 0.75]


def _cube():
    v = np.array([[x, y, z] for x in (1, 2) for y in (2, 3) for z in (3, 4)], np.int64)
    o = np.tile(np.array([[0, -1, 0]], np.float32), (len(v), 1))
    return v, o


def test_a_volume_against_itself_scores_one():
    v, o = _cube()
    fp, fg, counts = hv.scores((v, o), (v, o), DIMS, REACH, COS2)
    assert fp.tolist() == [7] * 8 and fg.tolist() == [7] * 8
    assert counts["pred"] == {"matched": [8, 8, 8], "voxels": 8} == counts["gt"]


def test_a_volume_moved_by_one_voxel():
    v = np.array([[1, 1, 1], [3, 3, 3]], np.int64)
    o = np.array([[1, 0, 0], [0, 0, 1]], np.float32)
    fp, fg, _ = hv.scores((v, o), (v + 1, o), DIMS, [0, 1], [-1.0, -1.0])
    assert fp.tolist() == [2, 2] and fg.tolist() == [2, 2]          # nothing at reach 0, everything at reach 1


def test_direction_bound_is_inclusive():
    a, b = np.array([[1, 0, 0]], np.float32), np.array([[1, 1, 0]], np.float32)       # dot^2 = 1, |a|^2 |b|^2 = 2
    v = np.array([[2, 2, 2]], np.int64)
    f = hv.match_flags(v, a, v, b, DIMS, [0, 0], [0.5, np.nextafter(0.5, 1.0)])
    assert f.tolist() == [1]


def test_zero_direction_matches_only_without_a_direction_test():
    v = np.array([[2, 2, 2]], np.int64)
    zero, one = np.zeros((1, 3), np.float32), np.array([[1, 0, 0]], np.float32)
    for a, b in ((zero, one), (one, zero), (zero, zero)):
        assert hv.match_flags(v, a, v, b, DIMS, [0, 0], [-1.0, 0.0]).tolist() == [1]
    assert hv.match_flags(v, one, v, one, DIMS, [0, 0], [-1.0, 0.0]).tolist() == [3]


def test_reach_is_clipped_at_the_six_faces():
    X, Y, Z = DIMS
    corners = np.array([[0, 0, 0], [X - 1, Y - 1, Z - 1]], np.int64)
    o = np.array([[1, 0, 0]] * 2, np.float32)
    # a target on the opposite face is not a neighbour "through" the border, whatever the reach
    f = hv.match_flags(corners[:1], o[:1], corners[1:], o[1:], DIMS, [4], [-1.0])
    assert f.tolist() == [0]
    for axis in range(3):
        for q in (0, DIMS[axis] - 1):
            qv = np.array([[2, 2, 2]], np.int64)
            qv[0, axis] = q
            tv = qv.copy()
            tv[0, axis] = q + (1 if q == 0 else -1)
            assert hv.match_flags(qv, o[:1], tv, o[:1], DIMS, [0, 1], [-1.0, -1.0]).tolist() == [2]


def test_voxel_lists_must_be_unique_and_inside():
    o = np.zeros((2, 3), np.float32)
    with pytest.raises(ValueError):
        hv.match_flags([[1, 1, 1], [1, 1, 1]], o, [[1, 1, 1]], o[:1], DIMS, [0], [-1.0])
    with pytest.raises(ValueError):
        hv.match_flags([[1, 1, 1]], o[:1], [[1, 1, 7]], o[:1], DIMS, [0], [-1.0])
