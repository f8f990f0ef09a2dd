"""GPU: the strand volume and the volume scores (monohair_amd/hairvolume.py, csrc/hairvolume.hip) against the numpy restatement
of their rule (tests/hair_volume_np.py, which tests/test_hair_volume_host.py holds to hand-computed cases): every quantity
EQUAL, not close -- the voxel list, cnt, the six sums, ori, coh and both counters; the flag bytes and the counts.  Only integer
sums and correctly rounded float64 operations in a fixed order are involved, so there is no tolerance anywhere."""
import functools
import json
import math
import os

import numpy as np
import pytest

import hair_volume_np as ref

pytestmark = pytest.mark.gpu

# three different dimensions each: a swapped axis shows
GRID_A, GRID_B, GRID_C = (12, 14, 16), (33, 17, 65), (8, 8, 520)
VS = 0.0025
BUST = (0.001, -0.002, 0.003)


def _vmin(dims):
    return (-0.5 * VS * dims[0] + 0.0003, -0.5 * VS * dims[1] - 0.0002, -0.5 * VS * dims[2] + 0.0001)


def _world(g, vmin, vs, bust):
    """voxel coordinates -> `.hair` coordinates (float32): the inverse of the vertex rule, up to rounding"""
    g = np.asarray(g, np.float64).reshape(-1, 3)
    w = g * vs + np.asarray(vmin)[None, :]
    w[:, 1:] *= -1.0
    return (w - np.asarray(bust)[None, :]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _strands(dims, seed=5):
    """seeded strands of 1, 2, 3, 64, 65 and 513 points, one of each length leaving through each of the six faces; random walks
    inside; piles of more than 64 and more than 1024 samples in one voxel -- in voxel coordinates"""
    rng = np.random.default_rng(seed)
    d = np.array(dims, np.float64)
    out = []
    for n in (1, 2, 3, 64, 65, 513):
        for axis in range(3):
            for side in (0, 1):
                a = rng.uniform(1.0, d - 2.0)
                b = rng.uniform(1.0, d - 2.0)
                b[axis] = -rng.uniform(1.0, 3.0) if side == 0 else d[axis] - 1.0 + rng.uniform(1.0, 3.0)
                t = np.linspace(0.0, 1.0, n)[:, None] if n > 1 else np.ones((1, 1))
                out.append(a[None, :] * (1.0 - t) + b[None, :] * t + rng.normal(0.0, 0.2, (n, 3)))
    for n in (40, 65, 130):
        start = rng.uniform(2.0, d - 3.0)
        out.append(start[None, :] + np.cumsum(rng.normal(0.0, 0.35, (n, 3)), 0))
    heavy, light = np.array([3.0, 4.0, 5.0]), np.array([5.0, 2.0, 7.0])
    for _ in range(3):
        out.append(heavy[None, :] + rng.uniform(-0.2, 0.2, (513, 3)))       # 3 x 512 segments of >= 1 sample each
    out.append(light[None, :] + rng.uniform(-0.2, 0.2, (100, 3)))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def _case(dims, sub):
    vmin = _vmin(dims)
    st = _strands(dims)
    counts = np.array([len(s) for s in st], np.int64)
    pts = _world(np.concatenate(st, 0), vmin, VS, BUST)
    return counts, pts, vmin, ref.voxelize(counts, pts, BUST, vmin, VS, dims, sub)


def _gpu(counts, pts, dims, sub, vmin, vs=VS, bust=BUST):
    from monohair_amd import hairvolume

    return hairvolume.voxelize_strands((counts, pts), bust, vmin, vs, dims, sub, return_details=True)


def _same(got, want):
    assert got["dropped_segments"] == want["dropped_segments"] and got["outside_samples"] == want["outside_samples"]
    assert np.array_equal(got["voxels"], want["voxels"]) and got["voxels"].dtype == np.int64
    assert np.array_equal(got["cnt"], want["cnt"]) and got["cnt"].dtype == np.int32
    assert np.array_equal(got["sums"], want["sums"])
    assert got["ori"].dtype == np.float32 and got["coh"].dtype == np.float64
    assert np.array_equal(got["coh"], want["coh"])
    assert np.array_equal(got["ori"], want["ori"])
    assert got["ori"].tobytes() == want["ori"].tobytes()          # (the signs of the zeros as well)
    assert got["samples"] == int(want["cnt"].sum())


@pytest.mark.parametrize("dims,sub", [(GRID_A, 2), (GRID_B, 1), (GRID_B, 16)])
def test_volume_equals_the_restatement(dims, sub):
    counts, pts, vmin, want = _case(dims, sub)
    # the inputs reach what they are meant to reach
    assert want["outside_samples"] > 0 and len(want["voxels"]) > 50
    assert want["cnt"].max() > 1024 and ((want["cnt"] > 64) & (want["cnt"] <= 1024)).any()
    v = want["voxels"]
    for axis in range(3):
        assert v[:, axis].min() == 0 and v[:, axis].max() == dims[axis] - 1
    _same(_gpu(counts, pts, dims, sub, vmin), want)


def test_two_runs_leave_the_same_bytes():
    counts, pts, vmin, _ = _case(GRID_A, 2)
    a, b = _gpu(counts, pts, GRID_A, 2, vmin), _gpu(counts, pts, GRID_A, 2, vmin)
    for k in ("voxels", "ori", "cnt", "coh", "sums"):
        assert a[k].tobytes() == b[k].tobytes(), k
    assert (a["dropped_segments"], a["outside_samples"]) == (b["dropped_segments"], b["outside_samples"])


def test_half_integer_ties():
    """voxel size 1/4 and a binary voxel_min: every sample of these strands sits exactly on k + 1/2 along its axis"""
    vmin, vs, bust = (-1.0, -1.5, -2.0), 0.25, (0.5, -0.25, 0.75)
    g = []
    for axis in range(3):
        p = np.tile(np.array([[3.0, 4.0, 5.0]]), (9, 1))
        p[:, axis] = np.arange(1, 10)
        g.append(p)
    counts = np.array([9, 9, 9], np.int64)
    pts = _world(np.concatenate(g, 0), vmin, vs, bust)
    want = ref.voxelize(counts, pts, bust, vmin, vs, GRID_A, 1)
    assert sorted(set(want["voxels"][:, 0].tolist())) == [2, 3, 4, 6, 8]      # x = 1.5 .. 8.5 -> the even neighbours
    _same(_gpu(counts, pts, GRID_A, 1, vmin, vs, bust), want)


def test_segments_of_8192_and_8193_samples():
    zero = (0.0, 0.0, 0.0)
    pts = np.array([[1, -1, 0], [1, -1, -512], [2, -2, 0], [2, -2, -512.0625]], np.float32)
    counts = np.array([2, 2], np.int64)
    want = ref.voxelize(counts, pts, zero, zero, 1.0, GRID_C, 16)
    assert want["dropped_segments"] == 1 and int(want["cnt"].sum()) == 8192 and len(want["voxels"]) == 513
    _same(_gpu(counts, pts, GRID_C, 16, zero, 1.0, zero), want)


def test_nan_vertices_zero_length_segments_and_an_empty_set():
    nan = float("nan")
    zero = (0.0, 0.0, 0.0)
    pts = np.array([[1, -2, -3], [2, -2, -3], [nan, -2, -3], [5, -2, -3], [6, -2, -3], [3, -3, -3], [3, -3, -3],
                    [4, -4, -4]], np.float32)
    counts = np.array([5, 2, 0, 1], np.int64)
    want = ref.voxelize(counts, pts, zero, zero, 1.0, GRID_A, 1)
    assert want["voxels"].tolist() == [[2, 2, 3], [3, 3, 3], [6, 2, 3]] and want["ori"][1].tolist() == [0.0, 0.0, 0.0]
    _same(_gpu(counts, pts, GRID_A, 1, zero, 1.0, zero), want)
    for counts in (np.zeros(0, np.int64), np.zeros(3, np.int64)):
        got = _gpu(counts, np.zeros((0, 3), np.float32), GRID_A, 2, zero, 1.0, zero)
        assert got["voxels"].shape == (0, 3) and got["ori"].shape == (0, 3) and got["cnt"].shape == (0,)
        assert got["sums"].shape == (0, 6) and (got["dropped_segments"], got["outside_samples"], got["samples"]) == (0, 0, 0)


def test_arguments_are_checked():
    from monohair_amd import hairvolume

    pts = np.zeros((2, 3), np.float32)
    for kw in (dict(sub=0), dict(sub=17), dict(voxel_size=0.0), dict(grid_resolution=(0, 4, 4)),
               dict(grid_resolution=(2048, 2048, 1024)), dict(bust_to_origin=(0.0, float("nan"), 0.0))):
        with pytest.raises(ValueError):
            hairvolume.voxelize_strands(([2], pts), **kw)
    with pytest.raises(ValueError):
        hairvolume.voxelize_strands(([3], pts))


def test_written_volume_reads_back_and_feeds_hairgrowing(tmp_path):
    import torch

    from monohair_amd import hairvolume
    from monohair_amd.hairgrow import HairGrowing

    counts, pts, vmin, want = _case(GRID_A, 2)
    out = str(tmp_path / "refine")
    hairvolume.write_volume(out, GRID_A, want["voxels"], want["ori"])
    grid, voxels, ori = hairvolume.load_volume(out)
    assert grid.tolist() == list(GRID_A) and np.array_equal(voxels, want["voxels"]) and np.array_equal(ori, want["ori"])
    assert ori.dtype == np.float32 and voxels.dtype == np.int64
    solver = HairGrowing(os.path.join(out, "Occ3D.mat"), os.path.join(out, "Ori3D.mat"))
    X, Y, Z = GRID_A
    assert (solver.W, solver.H, solver.Z) == (X, Y, Z)
    occ = solver.occ[0].cpu().numpy()                  # [Z,Y,X]
    v = want["voxels"]
    assert int(occ.sum()) == len(v) and (occ[v[:, 2], v[:, 1], v[:, 0]] == 1).all()
    got = solver.ori.permute(1, 2, 3, 0).cpu().numpy()[v[:, 2], v[:, 1], v[:, 0]]
    assert np.array_equal(got, want["ori"] * np.array([1, -1, -1], np.float32))
    torch.cuda.synchronize()


def test_voxelize_command_writes_the_volume_of_the_api(tmp_path, capsys):
    from monohair_amd import hairvolume
    from monohair_amd.pmvo_utils import VOXEL_MIN, write_strand

    st = _strands(GRID_A)
    counts = [len(s) for s in st]
    bust = (0.25, -0.125, 0.5)
    pts = _world(np.concatenate(st, 0), VOXEL_MIN, VS, bust)
    hair = str(tmp_path / "s.hair")
    write_strand(pts, hair, counts)
    out = str(tmp_path / "gt" / "refine")
    argv = ["voxelize", hair, "--out", out, "--grid"] + [str(v) for v in GRID_A] + ["--vsize", str(VS), "--sub", "2",
                                                                                   "--bust_to_origin"] + [str(b) for b in bust]
    assert hairvolume.main(argv) == 0
    want = ref.voxelize(counts, pts, bust, VOXEL_MIN, VS, GRID_A, 2)
    line = capsys.readouterr().out
    assert "%d voxels" % len(want["voxels"]) in line and "%d samples outside" % want["outside_samples"] in line
    assert "%d segments dropped" % want["dropped_segments"] in line
    grid, voxels, ori = hairvolume.load_volume(out)
    assert grid.tolist() == list(GRID_A) and np.array_equal(voxels, want["voxels"]) and np.array_equal(ori, want["ori"])


# ---- scores
PAIRS = ((0, None), (1, None), (2, None), (4, None), (1, 30.0), (2, 20.0), (4, 10.0), (0, 90.0))


@functools.lru_cache(maxsize=None)
def _volume(dims, seed, n):
    """a seeded sparse volume: n voxels (the two opposite corners among them), unit directions, a tenth of them zero"""
    rng = np.random.default_rng(seed)
    total = int(np.prod(dims))
    keys = np.sort(np.unique(np.concatenate([[0, total - 1], rng.choice(total, n, replace=False)])))
    v = np.stack([keys // (dims[1] * dims[2]), (keys // dims[2]) % dims[1], keys % dims[2]], 1).astype(np.int64)
    o = rng.normal(size=(len(v), 3))
    o = (o / np.linalg.norm(o, axis=1, keepdims=True)).astype(np.float32)
    o[rng.random(len(v)) < 0.1] = 0.0
    return v, o


def _bounds():
    from monohair_amd import hairvolume

    return hairvolume.threshold_bounds(PAIRS)


@pytest.mark.parametrize("dims,n", [(GRID_A, 300), (GRID_B, 1500)])
def test_scores_equal_the_restatement(dims, n):
    from monohair_amd import hairvolume

    pred, gt = _volume(dims, 1, n), _volume(dims, 2, n)
    reach, cos2 = _bounds()
    assert reach == [0, 1, 2, 4, 1, 2, 4, 0] and cos2[:4] == [-1.0] * 4 and cos2[4] == math.cos(30.0 * (math.pi / 180.0)) ** 2
    fp, fg, counts = ref.scores(pred, gt, dims, reach, cos2)
    assert 0 < counts["pred"]["matched"][4] < counts["pred"]["matched"][1] < len(fp)      # the bounds do bind
    got = hairvolume.score_volumes((dims,) + pred, (dims,) + gt, PAIRS, return_flags=True)
    assert np.array_equal(got["flags"]["pred"], fp) and np.array_equal(got["flags"]["gt"], fg)
    assert got["counts"] == counts
    P = [m / len(fp) for m in counts["pred"]["matched"]]
    R = [m / len(fg) for m in counts["gt"]["matched"]]
    assert got["precision"] == P and got["recall"] == R
    assert got["f_score"] == [2.0 * p * r / (p + r) if p + r else 0.0 for p, r in zip(P, R)]
    assert np.array_equal(hairvolume.match_volume_flags(pred[0], pred[1], gt[0], gt[1], dims, reach, cos2), fp)


def test_a_volume_against_itself_and_moved_by_one_voxel():
    from monohair_amd import hairvolume

    v, o = _volume(GRID_A, 3, 200)
    o = np.where((o == 0).all(1)[:, None], np.array([[1, 0, 0]], np.float32), o)       # every voxel has a direction
    got = hairvolume.score_volumes((GRID_A, v, o), (GRID_A, v, o), PAIRS)
    assert got["precision"] == [1.0] * 8 and got["recall"] == [1.0] * 8 and got["f_score"] == [1.0] * 8
    inner = v[(v[:, 0] < GRID_A[0] - 1) & (v[:, 1] < GRID_A[1] - 1) & (v[:, 2] < GRID_A[2] - 1)][::7]
    d = np.tile(np.array([[1, 0, 0]], np.float32), (len(inner), 1))
    moved = inner + 1
    apart = ~(moved[:, None, :] == inner[None, :, :]).all(2).any(1)     # moved voxels that land on no voxel of the list
    got = hairvolume.score_volumes((GRID_A, inner, d), (GRID_A, moved, d), ((0, None), (1, None)), return_flags=True)
    assert np.array_equal(got["flags"]["gt"] & 1, (~apart).astype(np.uint8)) and (got["flags"]["gt"] >> 1).all()
    assert got["recall"][1] == 1.0 and got["precision"][1] == 1.0


def test_empty_volumes_on_either_side():
    from monohair_amd import hairvolume

    v, o = _volume(GRID_A, 4, 50)
    none = (GRID_A, np.zeros((0, 3), np.int64), np.zeros((0, 3), np.float32))
    for pred, gt in ((none, (GRID_A, v, o)), ((GRID_A, v, o), none), (none, none)):
        got = hairvolume.score_volumes(pred, gt, PAIRS, return_flags=True)
        assert got["precision"] == [0.0] * 8 and got["recall"] == [0.0] * 8 and got["f_score"] == [0.0] * 8
        assert not got["flags"]["pred"].any() and not got["flags"]["gt"].any()
        assert got["counts"]["pred"]["voxels"] == len(pred[1]) and got["counts"]["gt"]["voxels"] == len(gt[1])


def test_exact_direction_bound_and_zero_directions():
    from monohair_amd import hairvolume

    v = np.array([[2, 2, 2]], np.int64)
    a, b = np.array([[1, 0, 0]], np.float32), np.array([[1, 1, 0]], np.float32)
    zero = np.zeros((1, 3), np.float32)
    cos2 = [0.5, float(np.nextafter(0.5, 1.0)), -1.0, 0.0]
    for q, t in ((a, b), (b, a), (zero, a), (a, zero), (zero, zero), (a, a)):
        want = ref.match_flags(v, q, v, t, GRID_A, [0] * 4, cos2)
        assert np.array_equal(hairvolume.match_volume_flags(v, q, v, t, GRID_A, [0] * 4, cos2), want)
    assert hairvolume.match_volume_flags(v, a, v, b, GRID_A, [0] * 4, cos2).tolist() == [1 | 4 | 8]
    assert hairvolume.match_volume_flags(v, zero, v, a, GRID_A, [0] * 4, cos2).tolist() == [4]


def test_reach_is_clipped_at_the_six_faces():
    """a full volume: a walk that wrapped round a face, or read past it, would find neighbours where there are none"""
    from monohair_amd import hairvolume

    dims = (5, 6, 7)
    total = int(np.prod(dims))
    keys = np.arange(total)
    v = np.stack([keys // 42, (keys // 7) % 6, keys % 7], 1).astype(np.int64)
    # the direction names the voxel's x: a query at x asks for x - 4 .. x + 4 through the bound on the angle
    o = np.stack([np.cos(0.3 * v[:, 0]), np.sin(0.3 * v[:, 0]), np.zeros(total)], 1).astype(np.float32)
    reach, cos2 = [4, 4, 1, 2], [math.cos(0.05) ** 2, -1.0, math.cos(0.05) ** 2, math.cos(0.35) ** 2]
    faces = v[((v == 0) | (v == np.array(dims) - 1)).any(1)]
    fo = o[((v == 0) | (v == np.array(dims) - 1)).any(1)]
    sparse_t = (v[::11], o[::11])
    for tv, to in ((v, o), sparse_t):
        want = ref.match_flags(faces, fo, tv, to, dims, reach, cos2)
        assert np.array_equal(hairvolume.match_volume_flags(faces, fo, tv, to, dims, reach, cos2), want)


def test_voxel_lists_must_be_unique_and_inside():
    from monohair_amd import hairvolume

    o = np.zeros((2, 3), np.float32)
    ok = (GRID_A, np.array([[1, 1, 1]]), o[:1])
    with pytest.raises(ValueError):
        hairvolume.score_volumes((GRID_A, np.array([[1, 1, 1], [1, 1, 1]]), o), ok)
    with pytest.raises(ValueError):
        hairvolume.score_volumes(ok, (GRID_A, np.array([[1, 1, 16]]), o[:1]))
    with pytest.raises(ValueError):
        hairvolume.score_volumes(ok, ((12, 14, 17),) + ok[1:])
    with pytest.raises(ValueError):
        hairvolume.score_volumes(ok, ok, ((5, None),))


def test_score_command_json_equals_the_api(tmp_path):
    from monohair_amd import hairvolume

    pred, gt = _volume(GRID_A, 1, 300), _volume(GRID_A, 2, 300)
    # (a written volume keeps a voxel without a direction occupied: Occ is 1, Ori is 0)
    pd, gd = str(tmp_path / "pred"), str(tmp_path / "gt")
    hairvolume.write_volume(pd, GRID_A, *pred)
    hairvolume.write_volume(gd, GRID_A, *gt)
    report = str(tmp_path / "scores.json")
    assert hairvolume.main(["score", pd, gd, "--json", report]) == 0
    api = hairvolume.score_volumes(pd, gd)
    assert json.load(open(report)) == json.loads(json.dumps(api))
    assert api["thresholds"] == [[0, None], [1, None], [1, 30.0], [1, 20.0], [1, 10.0]]
    reach, cos2 = hairvolume.threshold_bounds(hairvolume.DEFAULT_THRESHOLDS)
    assert api["counts"] == ref.scores(pred, gt, GRID_A, reach, cos2)[2]
    assert hairvolume.parse_thresholds("0:-,1:-,1:30,1:20,1:10") == hairvolume.DEFAULT_THRESHOLDS
