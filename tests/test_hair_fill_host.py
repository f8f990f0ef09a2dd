"""CPU-only: the numpy restatement of the inner fill (tests/hair_fill_np.py) held to hand-computed cases -- the vote bounds on
the hand-made planes of tests/hair_fill_cases.py, the sweeps between two plates, the degenerate domains -- and the voxel centres
of the production grid taken back through p2v."""
import numpy as np
import pytest

import hair_fill_cases as C
import hair_fill_np as R

F = np.float32


def _records(cams):
    from monohair_amd.camera import camera_records, cameras_from_list

    return camera_records(cameras_from_list(cams))


@pytest.fixture(scope="module")
def hand():
    from monohair_amd.pmvo_utils import map_code_lut

    depth, mask, bust, want = C.hand_planes(map_code_lut()[:, 3])
    rec = _records(C.hand_cameras())
    vox = R.grid_voxels(C.HAND_DIMS)
    counts = R.votes(rec, depth, mask, bust, R.centres(vox, C.HAND_VMIN, C.HAND_VS))
    return rec, (depth, mask, bust), want, vox, counts


def test_vote_counts_at_every_bound(hand):
    rec, planes, want, vox, counts = hand
    X, Y, Z = C.HAND_DIMS
    got = counts.reshape(X, Y, Z, 4)
    for (x, y), c in want.items():
        assert tuple(int(v) for v in got[x, y, 0]) == c, (x, y)
    # the layer z = 0 holds nothing but these cases and default voxels
    default = np.array([(x, y) not in want for x in range(X) for y in range(Y)]).reshape(X, Y)
    assert (got[:, :, 0][default] == np.array([5, 0, 5, 0])).all()


def test_gap_of_exactly_the_bound_counts_as_visible(hand):
    rec, (depth, mask, bust), want, vox, counts = hand
    p = R.centres(np.array([[4, 4, 0]]), C.HAND_VMIN, C.HAND_VS)
    assert p.tolist() == [[0.0, 0.0, 0.5]]
    seen = [bool(R.view_terms(rec[C.N_A + k], depth[C.N_A + k], mask[C.N_A + k], bust[C.N_A + k], p)[1][0]) for k in range(3)]
    assert seen == [True, True, False]      # below the bound, on it, one ulp above it


def test_domain_rule_and_order(hand):
    rec, planes, want, vox, counts = hand
    X, Y, Z = C.HAND_DIMS

    def member(dom, x, y):
        return bool(((dom == (x, y, 0)).all(1)).any())

    d0, d1 = R.domain(counts, C.HAND_DIMS), R.domain(counts, C.HAND_DIMS, max_bad=1)
    # n_vis 2 / 3, n_front 0 / 1, on the bust plane / an ulp behind it, mask code 51 / 52, the gap cases
    assert [member(d0, *k) for k in ((0, 0), (1, 0), (2, 0), (3, 0), (0, 1), (1, 1), (2, 1), (3, 1), (4, 4), (5, 0))] == \
        [True, False, False, True, True, False, False, True, True, True]
    # n_bad 0 / 1 under max_bad 0 / 1
    assert [member(d0, 4, 0), member(d1, 4, 0), member(d0, 6, 6), member(d1, 6, 6)] == [False, True, True, True]
    assert member(d1, 2, 1) and not member(d1, 1, 0)
    key = (d0[:, 0] * Y + d0[:, 1]) * Z + d0[:, 2]
    assert (np.diff(key) > 0).all()
    # an exterior voxel is no domain voxel
    d2 = R.domain(counts, C.HAND_DIMS, ext_voxels=np.array([[0, 0, 0], [6, 6, 0]]))
    assert not member(d2, 0, 0) and not member(d2, 6, 6) and len(d2) == len(d0) - 2


def test_points_no_view_counts(hand):
    rec, (depth, mask, bust), want, vox, counts = hand
    pts = np.array([[10.0, 0.0, 0.5], [np.nan, 0.0, 0.5], [0.0, 0.0, np.nan], [0.0, 0.0, 1.5], [0.0, 0.0, 0.5]], F)
    got = R.votes(rec, depth, mask, bust, pts)
    # outside every image; NaN; NaN; behind camera A and camera B (projecting onto pixel (4, 4)); the centre of voxel (4, 4, 0)
    assert got[:4].tolist() == [[0, 0, 0, 0]] * 4 and got[4].tolist() == [8, 2, 8, 0]
    assert not R.domain_flags(got)[:4].any()


def test_plates_after_one_two_and_three_sweeps():
    dims, ext, ori, dom, want = C.plates()
    for sweeps, (tensor, known, depth) in want.items():
        T, k, d = R.diffuse(ext, ori, dom, dims, sweeps)
        assert np.array_equal(T, np.array(tensor)) and k.tolist() == known and d.tolist() == depth, sweeps
    out = R.fill(ext, ori, dom, dims, 3, min_coh=0.5)
    # the middle voxel: M = diag(a/2, a/2, 0), the first of the two largest diagonal entries -> (1, 0, 0), coh 1/2 exactly
    assert out["ori"][1].tolist() == [1.0, 0.0, 0.0] and out["coh"][1] == 0.5
    assert out["coh"].tolist() == [0.75, 0.5, 0.75] and out["emit"].tolist() == [1, 1, 1]
    assert np.array_equal(out["ori"][0], F([1, 0, 0])) and np.array_equal(out["ori"][2], F([0, -1, 0]))
    assert out["rows"].shape == (3, 7) and (out["rows"][:, 6] == 1).all()
    # voxel (2, 1, 1) of the production grid: x = -0.32 + 2 * 0.0025, y and z negated
    assert np.array_equal(out["rows"][1, :3], F([-0.32 + 2 * 0.0025, 0.32 - 0.0025, 0.24 - 0.0025]))
    above = R.fill(ext, ori, dom, dims, 3, min_coh=np.nextafter(0.5, 1.0))
    assert above["emit"].tolist() == [1, 0, 1] and np.array_equal(above["rows"], out["rows"][[0, 2]])


def test_sweeps_zero_knows_nothing():
    dims, ext, ori, dom, _ = C.plates()
    out = R.fill(ext, ori, dom, dims, 0)
    assert not out["known"].any() and not out["emit"].any() and out["rows"].shape == (0, 7) and not out["tensor"].any()


def test_one_voxel_domain_and_island():
    dims, ext, ori, _, _ = C.plates()
    one = R.fill(ext, ori, np.array([[1, 0, 2]]), dims, 5)
    assert one["known"].tolist() == [1] and one["depth"].tolist() == [1] and one["ori"].tolist() == [[1.0, 0.0, 0.0]]
    assert one["coh"].tolist() == [1.0] and len(one["rows"]) == 1
    # an island: no exterior neighbour and no known domain neighbour, whatever the number of sweeps
    island = R.fill(ext, ori, np.array([[2, 1, 1]]), dims, 64)
    assert island["known"].tolist() == [0] and island["depth"].tolist() == [0] and len(island["rows"]) == 0
    assert island["ori"].tolist() == [[0.0, 0.0, 0.0]] and island["coh"].tolist() == [0.0]


def test_exterior_voxel_without_a_direction_is_no_source():
    dims = (3, 1, 1)
    ext = np.array([[0, 0, 0], [2, 0, 0]])
    dom = np.array([[1, 0, 0]])
    for bad in ((0, 0, 0), (np.nan, 0, 0), (0, np.inf, 0), (1e-5, 0, 0), (0, 0, 3e4)):
        t, src = R.source_tensors(np.array([bad, (0, 0, 1)], F))
        assert src.tolist() == [False, True] and not t[0].any()
        out = R.fill(ext, np.array([bad, (0, 0, 1)], F), dom, dims, 2)
        # the average is over the one source: c = 1, not 2
        assert out["tensor"].tolist() == [[0, 0, 4096.0 ** 2, 0, 0, 0]] and out["ori"].tolist() == [[0.0, 0.0, 1.0]]
    none = R.fill(ext, np.zeros((2, 3), F), dom, dims, 2)
    assert none["known"].tolist() == [0] and len(none["rows"]) == 0
    # half to even: 4096 * a = 2.5 -> 2, 3.5 -> 4
    t, src = R.source_tensors(np.array([(2.5 / 4096, 3.5 / 4096, 0)], F))
    assert t.tolist() == [[4.0, 16.0, 0.0, 8.0, 0.0, 0.0]] and src.tolist() == [True]


def test_centres_of_the_production_grid_return_their_voxels():
    from monohair_amd.pmvo_utils import GRID_RESOLUTION, VOXEL_MIN, VOXEL_SIZE, p2v

    X, Y, Z = (int(v) for v in GRID_RESOLUTION)
    assert (X, Y, Z) == (256, 256, 192) and VOXEL_MIN.tolist() == [-0.32, -0.32, -0.24] and VOXEL_SIZE == 0.0025
    for x0 in range(0, X, 64):                                   # (all 12.6 M voxels, a quarter at a time)
        vox = R.grid_voxels((X, Y, Z), x0, x0 + 64)
        x, y, z = p2v(R.centres(vox, VOXEL_MIN, VOXEL_SIZE).copy(), VOXEL_MIN, VOXEL_SIZE, GRID_RESOLUTION)
        assert np.array_equal(np.stack([x, y, z], 1), vox)
