"""CPU-only: the numpy restatement of the silhouette carve (tests/hair_carve_np.py) held to hand-computed cases -- the vote
bounds on the dyadic cameras and hand-made planes of tests/hair_fill_cases.py, the INSIDE decision on its two bounds, and the
mesh of a handful of voxel sets whose vertices, triangles, normals, volume and closedness are known."""
import numpy as np
import pytest

import hair_carve_np as R
import hair_fill_cases as C

F = np.float32
VMIN, VS = (-0.5, -0.25, -1.0), 0.25          # dyadic: every position, normal and volume below is exact


def _records(cams):
    from monohair_amd.camera import camera_records, cameras_from_list

    return camera_records(cameras_from_list(cams))


@pytest.fixture(scope="module")
def hand():
    from monohair_amd.pmvo_utils import map_code_lut

    depth, mask, bust, want = C.hand_planes(map_code_lut()[:, 3])
    rec = _records(C.hand_cameras())
    counts = R.votes(rec, mask, bust, R.centres(R.grid_voxels(C.HAND_DIMS), C.HAND_VMIN, C.HAND_VS))
    return rec, mask, bust, want, counts


# ------------------------------------------------------------------------------------------------- votes
def test_vote_counts_at_every_bound(hand):
    rec, mask, bust, want, counts = hand
    X, Y, Z = C.HAND_DIMS
    got = counts.reshape(X, Y, Z, 3)
    # the fill's hand cases are (n_in, n_vis, n_front, n_bad): the carve's counts are its first, third and fourth
    for (x, y), (n_in, _, n_front, n_bad) in want.items():
        assert tuple(int(v) for v in got[x, y, 0]) == (n_in, n_front, n_bad), (x, y)
    # mask code 51 is float32(0.2), not hair; 52 is hair
    assert got[2, 1, 0].tolist() == [5, 5, 1] and got[3, 1, 0].tolist() == [5, 5, 0]
    # z255 equal to the bust plane counts as free (view 0 alone); one float32 ulp behind it does not
    assert got[0, 1, 0].tolist() == [5, 1, 0] and got[1, 1, 0].tolist() == [5, 0, 0]
    default = np.array([(x, y) not in want for x in range(X) for y in range(Y)]).reshape(X, Y)
    assert (got[:, :, 0][default] == np.array([5, 5, 0])).all()


def test_points_no_view_counts(hand):
    rec, mask, bust, want, counts = hand
    pts = np.array([[10.0, 0.0, 0.5], [np.nan, 0.0, 0.5], [0.0, 0.0, np.nan], [0.0, 0.0, 1.5], [0.0, 0.0, 0.5]], F)
    got = R.votes(rec, mask, bust, pts)
    # outside every image; NaN; NaN; behind camera A and camera B; the centre of voxel (4, 4, 0), seen by all eight
    assert got[:4].tolist() == [[0, 0, 0]] * 4 and got[4].tolist() == [8, 8, 0]
    assert not R.inside_flags(got[:4], min_free=1, max_miss=3).any()


def test_inside_on_both_bounds(hand):
    rec, mask, bust, want, counts = hand
    X, Y, Z = C.HAND_DIMS

    def inside(x, y, **kw):
        return bool(R.inside_flags(counts, **kw).reshape(X, Y, Z)[x, y, 0])

    # n_free exactly min_free and one below it: voxel (3, 0) has n_free 1, voxel (5, 0) has 4
    assert inside(3, 0, min_free=1) and not inside(3, 0, min_free=2)
    assert inside(5, 0, min_free=4) and not inside(5, 0, min_free=5)
    # n_miss exactly max_miss and one above it: voxel (4, 0) has n_miss 1
    assert inside(4, 0, max_miss=1) and not inside(4, 0, max_miss=0)
    assert inside(2, 1, max_miss=1) and not inside(2, 1)
    # hidden by the bust in every view: inside the head, whatever the bounds
    assert not inside(2, 0, min_free=1, max_miss=8)
    assert inside(6, 6)


# ------------------------------------------------------------------------------------------------- mesh
def _flags(dims, voxels):
    f = np.zeros(dims, np.uint8)
    for v in voxels:
        f[v] = 1
    return f


def _mesh(flags):
    v, t = R.mesh(flags, VMIN, VS)
    assert v.dtype == F and t.dtype == np.int32 and v.shape[1:] == (3,) and t.shape[1:] == (3,)
    R.check_mesh(flags, v, t, VS)
    return v, t


def test_one_voxel():
    v, t = _mesh(_flags((3, 3, 3), [(1, 1, 1)]))
    assert len(v) == 8 and len(t) == 12
    # corners (1..2)^3 ascending by (i*4 + j)*4 + k: the first is (1, 1, 1) at vmin + 0.5 * vs, y and z negated
    assert v[0].tolist() == [-0.5 + 0.125, -(-0.25 + 0.125), -(-1.0 + 0.125)]
    assert v[7].tolist() == [-0.5 + 0.375, -(-0.25 + 0.375), -(-1.0 + 0.375)]
    # the -x face first: corners 000 001 011 010 = ranks 0 1 3 2
    assert t[0].tolist() == [0, 1, 3] and t[1].tolist() == [0, 3, 2]
    assert np.array_equal(R.corner_position((1, 1, 1), VMIN, VS), v[0])


def test_two_voxels_sharing_a_face_an_edge():
    v, t = _mesh(_flags((4, 3, 3), [(1, 1, 1), (2, 1, 1)]))
    assert len(v) == 12 and len(t) == 20
    v, t = _mesh(_flags((4, 4, 3), [(1, 1, 1), (2, 2, 1)]))
    assert len(v) == 14 and len(t) == 24


def test_voxel_in_a_grid_corner_and_a_one_voxel_grid():
    for dims, vox in (((2, 2, 2), (0, 0, 0)), ((2, 2, 2), (1, 1, 1)), ((1, 1, 1), (0, 0, 0))):
        v, t = _mesh(_flags(dims, [vox]))
        assert len(v) == 8 and len(t) == 12
    # corner (0, 0, 0) lies half a voxel in front of voxel_min
    v, _ = _mesh(_flags((2, 2, 2), [(0, 0, 0)]))
    assert v[0].tolist() == [-0.5 - 0.125, 0.25 + 0.125, 1.0 + 0.125]


def test_full_block_and_its_cavity():
    full = np.ones((3, 3, 3), np.uint8)
    v, t = _mesh(full)
    assert len(t) == 2 * 54 and len(v) == 4 ** 3 - 2 ** 3
    hollow = full.copy()
    hollow[1, 1, 1] = 0
    v2, t2 = _mesh(hollow)
    assert len(t2) == 2 * 60 and len(v2) == 4 ** 3
    # the cavity's six quads face inward: their normals point at the removed voxel's centre
    centre = R.centres(np.array([[1, 1, 1]]), VMIN, VS)[0].astype(np.float64)
    inward = 0
    for a, b, c in t2.tolist():
        p = v2[[a, b, c]].astype(np.float64)
        n = np.cross(p[1] - p[0], p[2] - p[0])
        if np.abs(p - centre).max() <= VS / 2:          # a triangle of the cavity
            inward += 1
            assert np.dot(n, centre - p.mean(0)) > 0
    assert inward == 12


def test_full_grid_of_several_scan_batches():
    """the full 64 x 64 x 33 grid, whose mesh tests/test_hair_carve_scan_gpu.py holds the kernels to: the six sides, and the
    corners of the grid less those of its interior"""
    X, Y, Z = 64, 64, 33
    v, t = _mesh(np.ones((X, Y, Z), np.uint8))
    assert len(t) == 4 * (X * Y + Y * Z + X * Z) == 33280
    assert len(v) == (X + 1) * (Y + 1) * (Z + 1) - (X - 1) * (Y - 1) * (Z - 1) == 16642
    assert t.min() == 0 and t.max() == len(v) - 1 and len(np.unique(v, axis=0)) == len(v)


def test_empty_flags():
    v, t = R.mesh(np.zeros((3, 2, 4), np.uint8), VMIN, VS)
    assert v.shape == (0, 3) and t.shape == (0, 3) and v.dtype == F and t.dtype == np.int32
    R.check_mesh(np.zeros((3, 2, 4), np.uint8), v, t, VS)


def test_order_of_vertices_and_faces():
    rng = np.random.default_rng(5)
    flags = (rng.random((5, 4, 6)) < 0.4).astype(np.uint8)
    v, t = _mesh(flags)
    # vertices ascend by corner key: x ascending, then world y descending, then world z descending
    key = np.lexsort((-v[:, 2], -v[:, 1], v[:, 0]))
    assert np.array_equal(key, np.arange(len(v))) and len(np.unique(v, axis=0)) == len(v)
    assert t.min() == 0 and t.max() == len(v) - 1
