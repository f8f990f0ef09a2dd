"""GPU: the silhouette carve (csrc/haircarve.hip, monohair_amd/haircarve.py) against its numpy restatement
(tests/hair_carve_np.py), by equality on every quantity: the three vote counts of every voxel centre on the hand-made planes of
tests/hair_fill_cases.py and on the seeded scene of the inner fill's tests (24 views of 32 x 64, the cameras of
tests/border_cases.py) for grids of 12 x 14 x 16 and 33 x 17 x 65 voxels, through a context of fp32 planes and one of 8-bit
codes, and against the columns of mh_inner_votes; the INSIDE flags of both forms of the kernel; the mesh of seeded and counted
flags, bytewise, into buffers with guard rows; the votes and flags of a scene one of whose views sits inside the grid, on the
plane of a layer of voxel centres; the API and the command.  (Grids whose mesh scans take several batches:
tests/test_hair_carve_scan_gpu.py.)"""
import os

import numpy as np
import pytest

import hair_carve_np as R
import hair_fill_cases as C
from test_hair_fill_gpu import GRIDS as FILL_GRIDS, seeded as fill_seeded          # noqa: F401  (a fixture of that file)
from test_hair_stereo_host import inside                                           # noqa: F401  (a fixture of that file)

pytestmark = pytest.mark.gpu

F = np.float32
GRIDS = {"12x14x16": ((12, 14, 16), 0.04), "33x17x65": ((33, 17, 65), 0.02)}
assert GRIDS == FILL_GRIDS
MESH_VS = 1.0 / 64.0          # dyadic, with the dyadic voxel_min of _mesh_vmin: positions, normals and volumes are exact
SENTINEL_F, SENTINEL_I, GUARD = F(-777.25), np.int32(-77), 5


def _vmin(dims, vs):
    return tuple(-0.5 * d * vs for d in dims)


def _records(cams):
    from monohair_amd.camera import camera_records, cameras_from_list

    return camera_records(cameras_from_list(cams))


def _planes_ctx(rec, mask):
    import torch

    from monohair_amd.pmvo import PMVO

    V, H, W = mask.shape
    z = torch.zeros((V, H, W), device="cuda")
    return PMVO.from_planes(rec, z, torch.zeros((V, H, W, 2), device="cuda"), z,
                            torch.from_numpy(np.ascontiguousarray(mask)).cuda(), patch_size=3)


# ------------------------------------------------------------------------------------------------- votes
def test_votes_on_the_hand_made_planes():
    from monohair_amd import haircarve
    from monohair_amd.pmvo_utils import map_code_lut

    _, mask, bust, want = C.hand_planes(map_code_lut()[:, 3])
    rec = _records(C.hand_cameras())
    ref = R.votes(rec, mask, bust, R.centres(R.grid_voxels(C.HAND_DIMS), C.HAND_VMIN, C.HAND_VS))
    ctx = _planes_ctx(rec, mask)
    got = haircarve.carve_votes(ctx, bust, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS)
    assert got.dtype == np.int32 and got.shape == C.HAND_DIMS + (3,)
    for (x, y), (n_in, _, n_front, n_bad) in want.items():
        assert tuple(int(v) for v in got[x, y, 0]) == (n_in, n_front, n_bad), (x, y)
    assert np.array_equal(got.reshape(-1, 3), ref)
    for min_free, max_miss in ((1, 0), (2, 0), (4, 0), (5, 0), (2, 1), (1, 8)):
        for early in (0, 1):          # (the lab switch between the two forms of the kernel; 1 is the default and is left set)
            ctx.set_lab_option("carve_early_exit", early)
            flags = haircarve.carve_inside(ctx, bust, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS, min_free, max_miss)
            assert flags.dtype == np.uint8 and flags.shape == C.HAND_DIMS
            assert np.array_equal(flags.reshape(-1), R.inside_flags(ref, min_free, max_miss)), (min_free, max_miss, early)
    f1 = haircarve.carve_inside(ctx, bust, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS, min_free=1)
    f2 = haircarve.carve_inside(ctx, bust, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS, min_free=2)
    assert f1[3, 0, 0] == 1 and f2[3, 0, 0] == 0 and f1[2, 0, 0] == 0 and f2[4, 0, 0] == 0
    for kw in (dict(min_free=0), dict(max_miss=-1)):
        with pytest.raises(ValueError):
            haircarve.carve_inside(ctx, bust, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS, **kw)


@pytest.fixture(scope="module")
def seeded(fill_seeded):
    """the seeded scene of tests/test_hair_fill_gpu.py (the same generator calls in the same order; held to that file's own
    fixture below): 24 views of 32 x 64, a bust plane around the points' depth or none, mask codes around the 0.2 bound"""
    import border_cases as B
    from monohair_amd.camera import cameras_from_list
    from monohair_amd.pmvo import PMVO
    from monohair_amd.pmvo_utils import map_code_lut

    rng = np.random.default_rng([17, 4])
    V, H, W = B.V, B.H, B.W
    cams = cameras_from_list(B.cameras())
    rec = _records(B.cameras())
    near = (F(102.0) + (rng.random((V, H, W), dtype=F) - F(0.5)) * F(30.0)).astype(F)
    depth = np.where(rng.random((V, H, W)) < 0.08, near, F(40.0)).astype(F)
    bust = np.where(rng.random((V, H, W)) < 0.5, F(255.0),
                    (F(102.0) + (rng.random((V, H, W), dtype=F) - F(0.5)) * F(30.0)).astype(F)).astype(F)
    m8 = rng.choice(np.array([255, 0, 49, 50, 51, 52], np.uint8), (V, H, W), p=[0.95, 0.01, 0.01, 0.01, 0.01, 0.01])
    k8, c8 = (rng.integers(0, 256, (V, H, W), dtype=np.uint8) for _ in range(2))
    mask = np.ascontiguousarray(map_code_lut()[m8][..., 3])
    ctxs = {"fp32": _planes_ctx(rec, mask),
            "u8": PMVO.from_u8(cams, depth, k8, c8, m8, image_size=[H, W], patch_size=3)}
    ref = {}
    for name, (dims, vs) in GRIDS.items():
        ref[name] = R.votes(rec, mask, bust, R.centres(R.grid_voxels(dims), _vmin(dims, vs), vs))
    # the same scene as the inner fill's tests: their bust planes, and their restatement's n_in, n_front and n_bad on their grids
    _, fill_bust, fill_ref = fill_seeded
    assert fill_bust.tobytes() == bust.tobytes() and sorted(fill_ref) == sorted(ref)
    assert all(np.array_equal(fill_ref[name][:, [0, 2, 3]], ref[name]) for name in ref)
    return ctxs, bust, ref


@pytest.mark.parametrize("kind", ["fp32", "u8"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_votes_and_flags_on_the_seeded_scene(seeded, grid, kind):
    from monohair_amd import haircarve, hairfill

    ctxs, bust, ref = seeded
    dims, vs = GRIDS[grid]
    vmin = _vmin(dims, vs)
    got = haircarve.carve_votes(ctxs[kind], bust, dims, vmin, vs).reshape(-1, 3)
    c = ref[grid]
    assert np.array_equal(got, c)
    # ... which are three of the inner fill's four columns, on either context
    fill = hairfill.inner_votes(ctxs[kind], bust, dims, vmin, vs).reshape(-1, 4)
    assert np.array_equal(got, fill[:, [0, 2, 3]])
    # the scene exercises the rule: views abstain, every count spreads, both clauses decide
    assert c[:, 0].min() < c[:, 0].max() and c[:, 1].min() < 5 <= c[:, 1].max() and (c[:, 2] == 1).any() and (c[:, 2] > 3).any()
    seen = set()
    for min_free in (1, 2, 5):
        for max_miss in (0, 1, 3):
            want = R.inside_flags(c, min_free, max_miss)
            for early in (0, 1):
                ctxs[kind].set_lab_option("carve_early_exit", early)
                flags = haircarve.carve_inside(ctxs[kind], bust, dims, vmin, vs, min_free, max_miss)
                assert np.array_equal(flags.reshape(-1), want), (min_free, max_miss, early)
            seen.add(int(want.sum()))
    # (on the coarse grid every voxel has n_free >= 2: min_free 1 and 2 decide alike there)
    assert len(seen) == (9 if grid == "33x17x65" else 6) and 0 not in seen and len(c) not in seen


@pytest.mark.parametrize("kind", ["fp32", "u8"])
def test_votes_and_flags_with_a_view_inside_the_grid(inside, kind):
    """the textured sphere of tests/hair_stereo_cases.py with a thirteenth view on the plane of a layer of voxel centres: 1 024
    centres have z' = 0 in it, where the projection divides by zero, and 15 360 lie behind it, over a thousand of them with a
    pixel inside its image (tests/test_hair_stereo_host.py::test_view_inside_the_grid asserts that of the restatement): the
    view abstains there by the sign of z' alone"""
    import hair_stereo_cases as S
    from monohair_amd import haircarve
    from test_hair_stereo_gpu import contexts

    ctx = contexts(S.inside_cameras(), inside["mask"])[0][kind]
    grid = (S.SPHERE_DIMS, S.SPHERE_VMIN, S.SPHERE_VS)
    c = inside["votes"]
    got = haircarve.carve_votes(ctx, inside["bust"], *grid).reshape(-1, 3)
    assert np.array_equal(got, c)
    assert c[:, 0].max() == 13 and c[:, 0].min() < 12
    seen = set()
    for min_free, max_miss in ((2, 0), (12, 0), (13, 0), (13, 1)):
        want = R.inside_flags(c, min_free, max_miss)
        for early in (0, 1):
            ctx.set_lab_option("carve_early_exit", early)
            flags = haircarve.carve_inside(ctx, inside["bust"], *grid, min_free, max_miss)
            assert np.array_equal(flags.reshape(-1), want), (min_free, max_miss, early)
        seen.add(int(want.sum()))
    assert np.array_equal(R.inside_flags(c).reshape(S.SPHERE_DIMS), inside["flags"])
    assert len(seen) >= 3 and 0 not in seen          # (min_free 13: the voxels the thirteenth view counts as well)


# ------------------------------------------------------------------------------------------------- mesh
def _mesh_vmin(dims):
    return tuple(-0.5 * (d + (d & 1)) * MESH_VS for d in dims)


def _guarded_mesh(flags):
    """the two entry points on buffers with GUARD rows behind the stated sizes and a guarded scratch, all full of a sentinel
    -> (vertices, faces) as numpy; asserts the counts, the guards and that no sentinel is left inside"""
    import torch

    from monohair_amd import _lib

    L, st = _lib.lib(), _lib.stream_ptr()
    dims = np.array(flags.shape, np.int32)
    vmin = np.array(_mesh_vmin(flags.shape), np.float64)
    ctx = _lib.bare_ctx("cuda:0")
    f = torch.from_numpy(np.ascontiguousarray(flags).reshape(-1)).cuda()
    need = int(L.mh_carve_mesh_scratch_bytes(_lib.host_ptr(dims)))
    assert need > 0
    scratch = torch.full((need + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    counts = torch.full((3,), -5, dtype=torch.int64, device="cuda")
    _lib.check(L.mh_carve_mesh_count(ctx, _lib.ptr(f), _lib.host_ptr(dims), _lib.ptr(counts), _lib.ptr(scratch), need, st))
    nv, nt, guard = (int(c) for c in counts.cpu().numpy())
    assert guard == -5 and (scratch[need:] == 0xA5).all()
    v = torch.full((nv + GUARD, 3), float(SENTINEL_F), dtype=torch.float32, device="cuda")
    t = torch.full((nt + GUARD, 3), int(SENTINEL_I), dtype=torch.int32, device="cuda")
    scratch.fill_(0x5A)      # (nothing is carried from the count to the mesh)
    _lib.check(L.mh_carve_mesh(ctx, _lib.ptr(f), _lib.host_ptr(vmin), MESH_VS, _lib.host_ptr(dims), nv, nt, _lib.ptr(v),
                               _lib.ptr(t), _lib.ptr(scratch), need, st))
    v, t = v.cpu().numpy(), t.cpu().numpy()
    assert (v[nv:] == SENTINEL_F).all() and (t[nt:] == SENTINEL_I).all() and (scratch[need:] == 0x5A).all()
    assert not (v[:nv] == SENTINEL_F).any() and not (t[:nt] == SENTINEL_I).any()
    return v[:nv], t[:nt]


def _check_flags(flags):
    from monohair_amd import haircarve

    vmin = _mesh_vmin(flags.shape)
    want_v, want_t = R.mesh(flags, vmin, MESH_VS)
    v, t = _guarded_mesh(flags)
    assert v.shape == want_v.shape and t.shape == want_t.shape          # both counts
    assert v.tobytes() == want_v.tobytes() and np.array_equal(t, want_t)
    R.check_mesh(flags, v, t, MESH_VS)
    # the API, and a second run
    for _ in range(2):
        av, at = haircarve.hull_mesh(flags, vmin, MESH_VS)
        assert av.dtype == F and at.dtype == np.int32 and av.tobytes() == v.tobytes() and at.tobytes() == t.tobytes()
    return v, t


def _seeded_flags(dims, density=None, count=None):
    rng = np.random.default_rng([23, dims[0], int(1000 * (density or 0)), count or 0])
    n = dims[0] * dims[1] * dims[2]
    if count is None:
        return (rng.random(dims) < density).astype(np.uint8)
    f = np.zeros(n, np.uint8)
    f[rng.choice(n, count, replace=False)] = rng.integers(1, 256, count, dtype=np.uint8)      # any non-zero byte is INSIDE
    return f.reshape(dims)


@pytest.mark.parametrize("density", [0.02, 0.5, 0.98, 1.0])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_mesh_of_seeded_flags(grid, density):
    dims = GRIDS[grid][0]
    flags = _seeded_flags(dims, density)
    v, t = _check_flags(flags)
    if density == 1.0:          # the full grid: its six sides
        X, Y, Z = dims
        assert flags.all() and len(t) == 4 * (X * Y + Y * Z + X * Z)
    else:
        assert 0 < flags.sum() < flags.size and len(t) > 0


@pytest.mark.parametrize("count", [0, 1, 63, 64, 65, 257])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_mesh_of_a_counted_number_of_voxels(grid, count):
    flags = _seeded_flags(GRIDS[grid][0], count=count)
    assert int(np.count_nonzero(flags)) == count
    v, t = _check_flags(flags)
    if count == 0:
        assert v.shape == (0, 3) and t.shape == (0, 3)
    if count == 1:
        assert len(v) == 8 and len(t) == 12


def test_mesh_of_the_hand_cases_and_a_one_voxel_grid():
    v, t = _check_flags(np.ones((1, 1, 1), np.uint8))
    assert len(v) == 8 and len(t) == 12
    _check_flags(np.zeros((1, 1, 1), np.uint8))
    two = np.zeros((4, 4, 3), np.uint8)
    two[1, 1, 1] = two[2, 2, 1] = 1
    v, t = _check_flags(two)
    assert len(v) == 14 and len(t) == 24
    two[2, 2, 1], two[2, 1, 1] = 0, 1
    v, t = _check_flags(two)
    assert len(v) == 12 and len(t) == 20
    hollow = np.ones((3, 3, 3), np.uint8)
    hollow[1, 1, 1] = 0
    v, t = _check_flags(hollow)
    assert len(v) == 64 and len(t) == 120
    corner = np.zeros((2, 3, 2), np.uint8)
    corner[1, 2, 1] = 1
    v, t = _check_flags(corner)
    assert len(v) == 8 and len(t) == 12


def test_grids_an_int32_cannot_index_are_refused():
    import torch

    from monohair_amd import _lib, haircarve

    L = _lib.lib()
    ok = np.array([1289, 1289, 1289], np.int32)
    assert int(L.mh_carve_mesh_scratch_bytes(_lib.host_ptr(ok))) > 0
    small = torch.zeros(64, dtype=torch.uint8, device="cuda")
    counts = torch.zeros(2, dtype=torch.int64, device="cuda")
    # 1290^3 < 2^31 <= 1291^3: the cells fit, the corners do not; 2048 x 1024 x 1024 = 2^31 cells
    for dims in ((1290, 1290, 1290), (2048, 1024, 1024), (0, 4, 4), (1 << 31, 1, 1)):
        d = np.array(dims, np.int64).astype(np.int32)
        assert int(L.mh_carve_mesh_scratch_bytes(_lib.host_ptr(d))) == 0
        with pytest.raises(_lib.MhError):
            _lib.check(L.mh_carve_mesh_count(_lib.bare_ctx("cuda:0"), _lib.ptr(small), _lib.host_ptr(d), _lib.ptr(counts),
                                             _lib.ptr(small), 64, _lib.stream_ptr()))
        with pytest.raises(_lib.MhError):
            _lib.check(L.mh_carve_mesh(_lib.bare_ctx("cuda:0"), _lib.ptr(small), _lib.host_ptr(np.zeros(3)), 1.0,
                                       _lib.host_ptr(d), 0, 0, None, None, _lib.ptr(small), 64, _lib.stream_ptr()))
    for dims in ((1290, 1290, 1290), (2048, 1024, 1024)):          # (a view of one byte: nothing of that size exists)
        with pytest.raises(ValueError):
            haircarve.hull_mesh(np.broadcast_to(np.zeros(1, np.uint8), dims))
    with pytest.raises(ValueError):
        haircarve.hull_mesh(np.zeros((4, 4), np.uint8))
    # a scratch that is too small is refused as well
    d = np.array([4, 4, 4], np.int32)
    with pytest.raises(_lib.MhError):
        _lib.check(L.mh_carve_mesh_count(_lib.bare_ctx("cuda:0"), _lib.ptr(small), _lib.host_ptr(d), _lib.ptr(counts),
                                         _lib.ptr(small), 64, _lib.stream_ptr()))


# ------------------------------------------------------------------------------------------------- API and command
def test_carve_equals_the_steps_run_one_by_one(seeded):
    from monohair_amd import haircarve

    ctxs, bust, ref = seeded
    dims, vs = GRIDS["33x17x65"]
    vmin = _vmin(dims, vs)
    for kind in ("fp32", "u8"):
        for min_free, max_miss in ((2, 0), (3, 1)):
            v, t, flags = haircarve.carve(ctxs[kind], None, bust, vs, min_free, max_miss, voxel_min=vmin, grid_resolution=dims)
            step = haircarve.carve_inside(ctxs[kind], bust, dims, vmin, vs, min_free, max_miss)
            assert flags.dtype == np.uint8 and np.array_equal(flags, step)
            assert np.array_equal(flags.reshape(-1), R.inside_flags(ref["33x17x65"], min_free, max_miss))
            sv, st = haircarve.hull_mesh(flags, vmin, vs)
            wv, wt = R.mesh(flags, vmin, vs)
            assert v.tobytes() == sv.tobytes() == wv.tobytes() and t.tobytes() == st.tobytes() == wt.tobytes() and len(t) > 0
            assert R.odd_edges(t) == 0


V_CMD, H_CMD, W_CMD = 6, 96, 54
OFFSET = [0.004, -0.008, 0.002]
CARVE = ["--voxel-size", "0.005"]


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a small synthetic capture on disk whose ground-truth coarse geometry and depth maps are taken away again"""
    import shutil

    from monohair_amd import synth_hair

    data = str(tmp_path_factory.mktemp("haircarve") / "data")
    base = synth_hair.write_case(data, "synthetic_hair", V=V_CMD, H=H_CMD, W=W_CMD, seed=0, n_strands=300, n_points=32)
    os.remove(os.path.join(base, "ours", "colmap_points.obj"))
    shutil.rmtree(os.path.join(base, "render_depth"))
    argv = ["--yaml=configs/reconstruct/synthetic_hair", "--data.root=%s" % data, "--data.image_size=[%d,%d]" % (H_CMD, W_CMD),
            "--PMVO.patch_size=3", "--name=t", "--bust_to_origin=[%g,%g,%g]" % tuple(OFFSET)]
    return base, argv


def _api(argv, bias_mm=0.0):
    import PMVO as cli
    from monohair_amd import gridviews, haircarve
    from monohair_amd.camera import load_cam, parsing_camera
    from monohair_amd.pmvo_utils import load_bust

    args = cli.config_parser(argv)
    assert np.array_equal(args.bust_to_origin, np.array(OFFSET))
    camera = parsing_camera(load_cam(args.image_camera_path), os.path.join(args.data.root, "capture_images"))
    masks = haircarve.load_masks(camera, args.data.mask_path)
    bv, bf, _ = load_bust(args.data.bust_path)
    bust = (bv + args.bust_to_origin, bf)
    v, t, flags = haircarve.carve(masks, camera, bust, 0.005, voxel_min=args.bbox_min, image_size=[H_CMD, W_CMD])
    pmvo = haircarve.mask_context(masks, camera, [H_CMD, W_CMD])
    depth = haircarve.carve_depth(pmvo, v, t, bust, bias_mm)
    hull, head = (gridviews.bust_planes(pmvo, m).cpu().numpy() for m in ((v, t), bust))
    return v, t, flags, depth, hull, head, list(camera.keys())


def test_command_writes_the_api_mesh_and_depth_and_guards_an_existing_file(case, capsys, monkeypatch):
    from monohair_amd import haircarve
    from monohair_amd.pmvo_utils import read_obj

    base, argv = case
    monkeypatch.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    obj, depth_dir = os.path.join(base, "ours", "colmap_points.obj"), os.path.join(base, "render_depth")
    assert not os.path.exists(obj) and not os.path.exists(depth_dir)          # it runs before render_depth/ exists
    assert haircarve.main(argv + CARVE) == 0
    out = capsys.readouterr().out
    v, t, flags, depth, hull, head, views = _api(argv)
    assert flags.shape == (128, 128, 96) and flags.any() and len(t) > 0 and R.odd_edges(t) == 0
    assert "%d INSIDE voxels" % int(np.count_nonzero(flags)) in out and "%d triangles" % len(t) in out
    fv, ft = read_obj(obj)
    # the file holds the vertices with bust_to_origin taken off, to nine decimals: load_colmap_points adds it back
    assert np.array_equal(ft, t) and np.abs(fv + np.array(OFFSET) - v.astype(np.float64)).max() <= 1e-9
    assert np.abs(fv - v.astype(np.float64)).max() > 1e-3
    first = open(obj, "rb").read()

    def planes():
        d = [np.load(os.path.join(depth_dir, view + ".npy")) for view in views]
        assert all(p.dtype == F and p.shape == (H_CMD, W_CMD, 3) and (p == p[..., :1]).all() for p in d)
        return np.stack([p[..., 0] for p in d])

    d0 = planes()
    assert d0.tobytes() == depth.tobytes() and np.array_equal(d0, np.minimum(hull, head))
    on_hull = hull != 255.0
    assert on_hull.any() and (d0[on_hull] < 255.0).all() and (hull < head).any()
    # an existing colmap_points.obj may be instant-ngp's: refused without --force, and left as it is
    with pytest.raises(SystemExit) as e:
        haircarve.main(argv + CARVE + ["--depth-bias-mm", "2"])
    assert "--force" in str(e.value) and open(obj, "rb").read() == first and planes().tobytes() == d0.tobytes()
    assert haircarve.main(argv + CARVE + ["--depth-bias-mm", "2", "--force"]) == 0
    assert open(obj, "rb").read() == first          # the bias moves the depth maps, not the mesh
    d2 = planes()
    c = haircarve.depth_bias(2.0)
    assert c.dtype == F and c == F(2.0 / 1000.0 / 2.0 * 255.0) and c > 0
    assert d2.tobytes() == _api(argv, 2.0)[3].tobytes()
    assert np.array_equal(d2, np.minimum(np.where(on_hull, (hull + c).astype(F), hull), head))
    assert np.array_equal(d2[~on_hull], d0[~on_hull]) and (d2[on_hull] != d0[on_hull]).any()
    front = on_hull & ((hull + c).astype(F) < head)
    assert np.array_equal(d2[front], (d0[front] + c).astype(F))
    # other bounds carve another hull
    assert haircarve.main(argv + CARVE + ["--min-free=3", "--max-miss=1", "--force"]) == 0
    assert open(obj, "rb").read() != first
