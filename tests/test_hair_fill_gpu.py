"""GPU: the inner fill (csrc/hairfill.hip, monohair_amd/hairfill.py) against its numpy restatement (tests/hair_fill_np.py), by
equality on every quantity: the four vote counts of every voxel centre on the hand-made planes of tests/hair_fill_cases.py and on
a seeded scene of 24 views of 32 x 64 (the cameras of tests/border_cases.py) for grids of 12 x 14 x 16 and 33 x 17 x 65 voxels,
through a context of fp32 planes and one of 8-bit codes; the domain list; the tensors, `known`, `depth`, coh, ori and rows of the
sweeps on the hand cases and on seeded sparse exteriors; the API and the command."""
import os

import numpy as np
import pytest

import hair_fill_cases as C
import hair_fill_np as R

pytestmark = pytest.mark.gpu

F = np.float32
GRIDS = {"12x14x16": ((12, 14, 16), 0.04), "33x17x65": ((33, 17, 65), 0.02)}
SWEEPS = (0, 1, 2, 7, 64)


def _vmin(dims, vs):
    return tuple(-0.5 * d * vs for d in dims)


def _records(cams):
    from monohair_amd.camera import camera_records, cameras_from_list

    return camera_records(cameras_from_list(cams))


def _planes_ctx(rec, depth, mask):
    import torch

    from monohair_amd.pmvo import PMVO

    V, H, W = depth.shape
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()      # noqa: E731
    return PMVO.from_planes(rec, t(depth), torch.zeros((V, H, W, 2), device="cuda"), torch.zeros((V, H, W), device="cuda"),
                            t(mask), patch_size=3)


# ------------------------------------------------------------------------------------------------- votes
@pytest.fixture(scope="module")
def hand():
    from monohair_amd.pmvo_utils import map_code_lut

    depth, mask, bust, want = C.hand_planes(map_code_lut()[:, 3])
    rec = _records(C.hand_cameras())
    counts = R.votes(rec, depth, mask, bust, R.centres(R.grid_voxels(C.HAND_DIMS), C.HAND_VMIN, C.HAND_VS))
    return _planes_ctx(rec, depth, mask), bust, want, counts


def test_votes_on_the_hand_made_planes(hand):
    from monohair_amd import hairfill

    ctx, bust, want, ref = hand
    got = hairfill.inner_votes(ctx, bust, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS)
    assert got.dtype == np.int32 and got.shape == C.HAND_DIMS + (4,)
    for (x, y), c in want.items():
        assert tuple(int(v) for v in got[x, y, 0]) == c, (x, y)
    assert np.array_equal(got.reshape(-1, 4), ref)
    for max_bad in (0, 1):
        dom = hairfill.inner_domain(ctx, bust, None, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS, max_bad=max_bad)
        assert dom.dtype == np.int64 and np.array_equal(dom, R.domain(ref, C.HAND_DIMS, max_bad=max_bad))
    assert len(hairfill.inner_domain(ctx, bust, None, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS, max_bad=1)) > \
        len(hairfill.inner_domain(ctx, bust, None, C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS))


@pytest.fixture(scope="module")
def seeded():
    """24 views of 32 x 64: in most pixels a surface far in front (not visible), a bust plane around the points' depth or none,
    mask codes around the 0.2 bound -- so that the four counts spread over their ranges and the domain is neither empty nor full"""
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
    lut = map_code_lut()
    mask = np.ascontiguousarray(lut[m8][..., 3])
    ctxs = {"fp32": _planes_ctx(rec, depth, mask),
            "u8": PMVO.from_u8(cams, depth, k8, c8, m8, image_size=[H, W], patch_size=3)}
    ref = {}
    for name, (dims, vs) in GRIDS.items():
        ref[name] = R.votes(rec, depth, mask, bust, R.centres(R.grid_voxels(dims), _vmin(dims, vs), vs))
    return ctxs, bust, ref


@pytest.mark.parametrize("kind", ["fp32", "u8"])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_votes_and_domain_on_the_seeded_scene(seeded, grid, kind):
    from monohair_amd import hairfill

    ctxs, bust, ref = seeded
    dims, vs = GRIDS[grid]
    vmin = _vmin(dims, vs)
    got = hairfill.inner_votes(ctxs[kind], bust, dims, vmin, vs).reshape(-1, 4)
    assert np.array_equal(got, ref[grid])
    # the scene exercises the rule: every count takes several values, views abstain, and each clause of the domain decides
    c = ref[grid]
    assert c[:, 0].min() < c[:, 0].max() and (c[:, 1] == 2).any() and (c[:, 1] == 3).any() and (c[:, 3] == 1).any()
    dom = hairfill.inner_domain(ctxs[kind], bust, None, dims, vmin, vs)
    want = R.domain(ref[grid], dims)
    assert 0 < len(want) < len(c) and np.array_equal(dom, want)
    X, Y, Z = dims
    assert (np.diff((dom[:, 0] * Y + dom[:, 1]) * Z + dom[:, 2]) > 0).all()
    # exterior voxels leave the domain: every third domain voxel and some voxels that were not in it
    ext = np.concatenate([want[::3], R.grid_voxels(dims)[~R.domain_flags(c)][::97]])
    dom2 = hairfill.inner_domain(ctxs[kind], bust, ext, dims, vmin, vs, max_bad=1)
    assert np.array_equal(dom2, R.domain(ref[grid], dims, ext, max_bad=1))
    assert not (dom2[:, None, :] == want[::3][None, :8, :]).all(2).any()


# ------------------------------------------------------------------------------------------------- sweeps and resolve
def _same(got_rows, got, ref):
    assert got_rows.dtype == F and got_rows.tobytes() == ref["rows"].tobytes()
    assert np.array_equal(got["tensor"], ref["tensor"]) and got["tensor"].dtype == np.float64
    assert np.array_equal(got["known"], ref["known"]) and np.array_equal(got["depth"], ref["depth"])
    assert np.array_equal(got["coh"], ref["coh"], equal_nan=True)
    assert got["ori"].tobytes() == ref["ori"].tobytes() and got["world"].tobytes() == ref["world"].tobytes()
    assert np.array_equal(got["emit"], ref["emit"])


def _check(ext, ori, dom, dims, sweeps, min_coh=0.0, vmin=(-0.32, -0.32, -0.24), vs=0.0025):
    from monohair_amd import hairfill

    rows, det = hairfill.diffuse_orientation(ext, ori, dom, dims, sweeps, min_coh, True, vmin, vs)
    ref = R.fill(ext, ori, dom, dims, sweeps, min_coh, vmin, vs)
    _same(rows, det, ref)
    return rows, det


def test_hand_cases_of_the_sweeps():
    dims, ext, ori, dom, want = C.plates()
    for sweeps, (tensor, known, depth) in want.items():
        rows, det = _check(ext, ori, dom, dims, sweeps, 0.5)
        assert np.array_equal(det["tensor"], np.array(tensor)) and det["known"].tolist() == known
        assert det["depth"].tolist() == depth
    assert det["coh"].tolist() == [0.75, 0.5, 0.75] and det["ori"][1].tolist() == [1.0, 0.0, 0.0] and len(rows) == 3
    rows, det = _check(ext, ori, dom, dims, 3, np.nextafter(0.5, 1.0))
    assert det["emit"].tolist() == [1, 0, 1]
    _check(ext, ori, np.array([[1, 0, 2]]), dims, 5)                      # a one-voxel domain
    rows, det = _check(ext, ori, np.array([[2, 1, 1]]), dims, 64)         # an island
    assert det["known"].tolist() == [0] and len(rows) == 0
    for bad in ((0, 0, 0), (np.nan, 0, 0), (0, np.inf, 0), (1e-5, 0, 0), (0, 0, 3e4)):      # no source
        rows, det = _check(np.array([[0, 0, 0], [2, 0, 0]]), np.array([bad, (0, 0, 1)], F), np.array([[1, 0, 0]]), (3, 1, 1), 2)
        assert det["ext_source"].tolist() == [0, 1] and det["tensor"].tolist() == [[0, 0, 4096.0 ** 2, 0, 0, 0]]


@pytest.mark.parametrize("n_dom", [1, 63, 64, 65, 257, 3000])
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_sweeps_on_seeded_sparse_exteriors(grid, n_dom):
    dims, vs = GRIDS[grid]
    nvox = dims[0] * dims[1] * dims[2]
    if n_dom == 3000:
        n_dom = {"12x14x16": 1100, "33x17x65": 6000}[grid]
    ext, ori, dom = C.seeded_sparse(dims, nvox // 5, n_dom, seed=3, faces=n_dom > 257)
    depths = set()
    for sweeps in SWEEPS:
        for min_coh in (0.0, 0.5):
            rows, det = _check(ext, ori, dom, dims, sweeps, min_coh, _vmin(dims, vs), vs)
        depths |= set(det["depth"].tolist())
        assert not det["known"].any() if sweeps == 0 else (det["known"].any() or n_dom == 1)
    if n_dom > 257:
        # the front moved for several sweeps, some rows were never reached, and min_coh 0.5 dropped rows that 0 kept
        assert {0, 1, 2, 3} <= depths
        assert 0 < len(rows) < len(_check(ext, ori, dom, dims, 64, 0.0, _vmin(dims, vs), vs)[0])
        for face, d in enumerate(dims):                     # the domain touches all six faces
            assert (dom[:, face] == 0).any() and (dom[:, face] == d - 1).any()


def test_empty_lists():
    dims, ext, ori, dom, _ = C.plates()
    none = np.zeros((0, 3), np.int64)
    rows, det = _check(ext, ori, none, dims, 3)
    assert rows.shape == (0, 7) and det["tensor"].shape == (0, 6)
    rows, det = _check(none, np.zeros((0, 3), F), dom, dims, 3)
    assert rows.shape == (0, 7) and not det["known"].any()
    _check(none, np.zeros((0, 3), F), none, dims, 0)


def test_two_runs_leave_the_same_bytes_and_a_permuted_domain_the_permuted_result():
    from monohair_amd import hairfill

    dims, vs = GRIDS["33x17x65"]
    ext, ori, dom = C.seeded_sparse(dims, 7000, 5000, seed=5, faces=True)
    a_rows, a = hairfill.diffuse_orientation(ext, ori, dom, dims, 9, 0.3, True, _vmin(dims, vs), vs)
    b_rows, b = hairfill.diffuse_orientation(ext, ori, dom, dims, 9, 0.3, True, _vmin(dims, vs), vs)
    assert a_rows.tobytes() == b_rows.tobytes() and all(a[k].tobytes() == b[k].tobytes() for k in a)
    perm = np.random.default_rng(2).permutation(len(dom))
    p_rows, p = hairfill.diffuse_orientation(ext, ori, dom[perm], dims, 9, 0.3, True, _vmin(dims, vs), vs)
    for k in ("tensor", "known", "depth", "coh", "ori", "world", "emit"):
        assert p[k].tobytes() == a[k][perm].tobytes(), k
    keep = a["emit"][perm] != 0
    assert p_rows[:, :3].tobytes() == a["world"][perm][keep].tobytes() and len(p_rows) == len(a_rows) > 0


def test_bad_lists_and_arguments_are_refused():
    from monohair_amd import hairfill

    dims, ext, ori, dom, _ = C.plates()
    for bad_dom in (np.array([[1, 1, 1], [1, 1, 1]]), np.array([[0, 1, 1]]), np.array([[5, 1, 1]]), np.array([[1, -1, 1]])):
        with pytest.raises(ValueError):          # listed twice; an exterior voxel; outside the grid
            hairfill.diffuse_orientation(ext, ori, bad_dom, dims, 1)
    for kw in (dict(sweeps=-1), dict(sweeps=1025), dict(min_coh=float("nan"))):
        with pytest.raises(ValueError):
            hairfill.diffuse_orientation(ext, ori, dom, dims, **kw)


# ------------------------------------------------------------------------------------------------- API and command
def test_fill_inner_equals_the_steps_run_one_by_one(seeded):
    from monohair_amd import hairfill

    ctxs, bust, ref = seeded
    dims, vs = GRIDS["33x17x65"]
    vmin = _vmin(dims, vs)
    ext, ori, _ = C.seeded_sparse(dims, 9000, 8, seed=9)
    for kind in ("fp32", "u8"):
        rows, det = hairfill.fill_inner(ctxs[kind], bust, (np.array(dims, np.int32), ext, ori), sweeps=5, min_coh=0.4,
                                        max_bad=1, voxel_min=vmin, voxel_size=vs, return_details=True)
        dom = hairfill.inner_domain(ctxs[kind], bust, ext, dims, vmin, vs, max_bad=1)
        assert np.array_equal(det["domain"], dom) and np.array_equal(dom, R.domain(ref["33x17x65"], dims, ext, max_bad=1))
        step = hairfill.diffuse_orientation(ext, ori, dom, dims, 5, 0.4, False, vmin, vs)
        want = R.fill(ext, ori, dom, dims, 5, 0.4, vmin, vs)
        assert rows.tobytes() == step.tobytes() == want["rows"].tobytes() and 0 < len(rows) < len(dom)


V_CMD, H_CMD, W_CMD = 6, 96, 54


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    """a small synthetic capture on disk and, in place of a run of PMVO.py, the volume of its strands as refine/"""
    from monohair_amd import hairvolume, synth_hair

    data = str(tmp_path_factory.mktemp("hairfill") / "data")
    base = synth_hair.write_case(data, "synthetic_hair", V=V_CMD, H=H_CMD, W=W_CMD, seed=0, n_strands=300, n_points=32)
    argv = ["--yaml=configs/reconstruct/synthetic_hair", "--data.root=%s" % data, "--data.image_size=[%d,%d]" % (H_CMD, W_CMD),
            "--PMVO.patch_size=3", "--name=t"]
    refine = os.path.join(base, "output", "t", "refine")
    r = hairvolume.voxelize_strands(os.path.join(base, "gt_strands.hair"))
    hairvolume.write_volume(refine, r["grid_resolution"], r["voxels"], r["ori"])
    return base, argv, refine


def _api_rows(base, argv, refine, **kw):
    import PMVO as cli
    from monohair_amd import hairfill
    from monohair_amd.camera import load_cam, parsing_camera
    from monohair_amd.pmvo_utils import load_bust

    args = cli.config_parser(argv)
    camera = parsing_camera(load_cam(args.image_camera_path), os.path.join(args.data.root, "capture_images"))
    vertices, faces, _ = load_bust(args.data.bust_path)
    return hairfill.fill_inner(cli.load_views(camera, args), (vertices + args.bust_to_origin, faces), refine, **kw)


def test_command_writes_the_api_rows_and_guards_an_existing_file(case, capsys, monkeypatch):
    from monohair_amd import hairfill

    base, argv, refine = case
    monkeypatch.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    raw = os.path.join(base, "ours", "raw.npy")
    assert not os.path.exists(raw)
    assert hairfill.main(argv + ["--sweeps", "6"]) == 0
    out = capsys.readouterr().out
    first = np.load(raw)
    want = _api_rows(base, argv, refine, sweeps=6)
    assert first.dtype == F and first.shape[1] == 7 and first.tobytes() == want.tobytes()
    assert "%d rows written" % len(first) in out and "domain voxels" in out and "rows by the sweep" in out
    # an existing raw.npy may be a network's output: refused without --force, and left as it is
    with pytest.raises(SystemExit) as e:
        hairfill.main(argv + ["--sweeps=2", "--min-coh=0.6"])
    assert "--force" in str(e.value) and np.load(raw).tobytes() == first.tobytes()
    assert hairfill.main(argv + ["--sweeps=2", "--min-coh=0.6", "--max-bad", "1", "--force"]) == 0
    second = np.load(raw)
    assert second.tobytes() == _api_rows(base, argv, refine, sweeps=2, min_coh=0.6, max_bad=1).tobytes()
    print("command: %d rows at 6 sweeps, %d at 2 sweeps / min_coh 0.6 / max_bad 1" % (len(first), len(second)))
