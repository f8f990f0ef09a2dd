"""GPU: the photo-consistent carve (csrc/hairstereo.hip, monohair_amd/hairstereo.py) against its numpy restatement
(tests/hair_stereo_np.py), bit for bit on every quantity -- the reduced images and census planes, every winner key, the
agreement counts, the refined flags and the depth planes -- on the hand-made scenes and on the textured sphere of
tests/hair_stereo_cases.py (scene and control, the hull and the hull with the spike), at candidate counts of 1, 63, 64, 65 and
257, through a context of fp32 planes and one of 8-bit codes; neighbour tables of 3 to 8 columns with `keep` up to the table's
width, whose distances arrive out of order, on a hand-made scene and on the sphere; a thirteenth view inside the sphere's grid,
with voxel centres on its plane z' = 0 and behind it; the refusals; and the refined flags as a mesh."""
import numpy as np
import pytest

import hair_carve_np as CARVE
import hair_fill_cases as C
import hair_stereo_cases as S
import hair_stereo_np as R
from test_hair_stereo_host import (INSIDE_KEEPS, M255, SPHERE, WIDE, inside, records, sphere, wide,          # noqa: F401
                                   wide_conditions)          # (sphere, wide and inside are fixtures of that file)

pytestmark = pytest.mark.gpu

F = np.float32
KINDS = ("fp32", "u8")


def contexts(cams, mask):
    """-> ({kind: PMVO context}, the float32 mask planes both hold): mask codes 255 and 0 through the loaders' table"""
    import torch

    from monohair_amd.camera import cameras_from_list
    from monohair_amd.pmvo import PMVO
    from monohair_amd.pmvo_utils import map_code_lut

    m8 = np.where(mask > 0.5, 255, 0).astype(np.uint8)
    planes = np.ascontiguousarray(map_code_lut()[m8][..., 3])
    assert np.array_equal(planes > F(0.2), mask > 0.5)
    V, H, W = mask.shape
    rec, cam = records(cams), cameras_from_list(cams)
    z = torch.zeros((V, H, W), device="cuda")
    zero8 = np.zeros((V, H, W), np.uint8)
    fp32 = PMVO.from_planes(rec, z, torch.zeros((V, H, W, 2), device="cuda"), z, torch.from_numpy(planes).cuda(), camera=cam,
                            patch_size=3)
    u8 = PMVO.from_u8(cam, np.full((V, H, W), 255.0, F), zero8, zero8, m8, image_size=[H, W], patch_size=3)
    return {"fp32": fp32, "u8": u8}, planes


def reference(t, gray, flags, nb, radius, keep, max_cost, m255, min_agree, min_through):
    """the restatement on terms made once"""
    codes = R.census(R.reduce_gray(gray, t.cell_size), radius)
    keys = R.winners(t, codes, nb, radius, keep, np.flatnonzero(np.asarray(flags).reshape(-1) != 0))
    a = R.agree(t, flags, keys, max_cost, m255)
    refined, depth = R.refine(t, flags, keys, a, max_cost, m255, min_agree, min_through)
    return dict(keys=keys, agree=a, refined=refined, depth=depth)


def run_stages(ctx, bust, flags, gray, nb, grid, cell, radius, keep, max_cost, m255, min_agree, min_through):
    """the four entry points one by one through the Python layer"""
    from monohair_amd import hairstereo

    dims, vmin, vs = grid
    keys = hairstereo.stereo_winners(ctx, bust, flags, gray, nb, dims, vmin, vs, cell, radius, keep)
    a = hairstereo.stereo_agree(ctx, bust, flags, keys, dims, vmin, vs, cell, max_cost, m255)
    refined, depth = hairstereo.stereo_refine(ctx, bust, flags, keys, a, dims, vmin, vs, cell, max_cost, m255, min_agree,
                                              min_through)
    assert keys.dtype == np.uint64 and a.dtype == np.int32 and a.shape == tuple(dims) and refined.dtype == np.uint8 and \
        refined.shape == tuple(dims) and depth.dtype == F and depth.shape == keys.shape
    return dict(keys=keys, agree=a.reshape(-1), refined=refined.reshape(-1), depth=depth)


def same(got, want, what=""):
    for name in ("keys", "agree", "refined", "depth"):
        assert got[name].shape == want[name].shape and got[name].tobytes() == want[name].tobytes(), (what, name)


# ------------------------------------------------------------------------------------------------- census
@pytest.mark.parametrize("cell,radius", [(1, 1), (2, 1), (2, 2), (3, 3), (5, 2), (48, 1)])
def test_census_planes(cell, radius):
    from monohair_amd import hairstereo

    hand, reduced, _ = S.census_image()
    for gray in (hand, S.hand_scene_one()["gray"], S.sphere_views()[0][:3]):
        g, code = hairstereo.stereo_census(gray, cell, radius)
        want = R.reduce_gray(gray, cell)
        assert g.dtype == np.uint8 and code.dtype == np.uint64 and np.array_equal(g, want)
        assert code.shape == want.shape and code.tobytes() == R.census(want, radius).tobytes()
    if (cell, radius) == (2, 1):
        assert np.array_equal(hairstereo.stereo_census(hand, 2, 1)[0], reduced)


# ------------------------------------------------------------------------------------------------- the hand-made scenes
HAND_GRID = (C.HAND_DIMS, C.HAND_VMIN, C.HAND_VS)


@pytest.fixture(scope="module")
def hand():
    out = {}
    for name, scene in (("one", S.hand_scene_one()), ("two", S.hand_scene_two())):
        ctxs, planes = contexts(C.hand_cameras(), scene["mask"])
        assert np.array_equal(planes, scene["mask"])
        out[name] = (scene, ctxs)
    return out


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("cell", [1, 2, 3])
@pytest.mark.parametrize("name", ["one", "two"])
def test_hand_scenes_equal_the_restatement(hand, name, cell, kind):
    scene, ctxs = hand[name]
    t = R.Terms(records(C.hand_cameras()), scene["mask"], scene["bust"], C.HAND_VMIN, C.HAND_VS, C.HAND_DIMS, cell)
    margins = (S.GAP, np.nextafter(S.GAP, F(0)), np.nextafter(S.GAP, F(100)), F(0)) + \
        tuple(S.hand_scene_two()["margins"][k] for k in ("sum_below", "sum_above"))
    seen = set()
    for keep in (1, 2):
        for max_cost, m255, min_agree, min_through in [(1024, margins[0], 3, 3), (384, margins[1], 4, 1), (383, margins[2], 1, 2),
                                                       (128, margins[3], 3, 3), (128, margins[4], 3, 4), (0, margins[5], 3, 3)]:
            args = (S.HAND_NB, 1, keep, max_cost, m255, min_agree, min_through)
            want = reference(t, scene["gray"], scene["flags"], *args)
            got = run_stages(ctxs[kind], scene["bust"], scene["flags"], scene["gray"], S.HAND_NB, HAND_GRID, cell, *args[1:])
            same(got, want, (keep, max_cost, float(m255)))
            seen.add(int(got["refined"].sum()))
    # the hand-computed values themselves, at the cell they were worked out for
    if name == "one" and cell == 1:
        from monohair_amd import hairstereo

        for keep in (1, 2):
            keys = hairstereo.stereo_winners(ctxs[kind], scene["bust"], scene["flags"], scene["gray"], S.HAND_NB, *HAND_GRID,
                                             cell=1, radius=1, keep=keep)
            for (r, i, j), k in scene["keys"][keep].items():
                assert keys[r, i, j] == k, (keep, r, i, j)
            for (kp, max_cost, m255), cases in scene["agree"].items():
                if kp == keep:
                    a = hairstereo.stereo_agree(ctxs[kind], scene["bust"], scene["flags"], keys, *HAND_GRID, cell=1,
                                                max_cost=max_cost, m255=m255)
                    assert all(a[v] == n for v, n in cases.items()), (keep, max_cost, float(m255))
    if name == "two" and cell == 2:
        assert seen == {3, 5}          # the through test removes w and u, or nothing


@pytest.fixture(scope="module")
def hand_wide():
    scene = S.hand_scene_wide()
    ctxs, planes = contexts(C.hand_cameras(), scene["mask"])
    assert np.array_equal(planes, scene["mask"])
    return scene, ctxs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("table,keep", [("keys4", 1), ("keys4", 2), ("keys4", 3), ("keys4", 4), ("keys7", 1), ("keys7", 4),
                                        ("keys7", 5), ("keys7", 7)])
def test_hand_scene_with_wide_tables(hand_wide, table, keep, kind):
    """tables of four and seven columns: the hand-computed keys, and every stage against the restatement"""
    from monohair_amd import hairstereo

    scene, ctxs = hand_wide
    nb = S.HAND_NB4 if table == "keys4" else S.HAND_NB7
    keys = hairstereo.stereo_winners(ctxs[kind], scene["bust"], scene["flags"], scene["gray"], nb, *HAND_GRID, cell=1, radius=1,
                                     keep=keep)
    for (r, i, j), k in scene[table].get(keep, {}).items():
        assert keys[r, i, j] == k, (r, i, j, hex(int(keys[r, i, j])), hex(int(k)))
    t = R.Terms(records(C.hand_cameras()), scene["mask"], scene["bust"], C.HAND_VMIN, C.HAND_VS, C.HAND_DIMS, 1)
    for max_cost, m255, min_agree, min_through in [(1024, S.GAP, 3, 3), (426, np.nextafter(S.GAP, F(0)), 2, 1), (341, F(0), 1, 2)]:
        args = (nb, 1, keep, max_cost, m255, min_agree, min_through)
        want = reference(t, scene["gray"], scene["flags"], *args)
        got = run_stages(ctxs[kind], scene["bust"], scene["flags"], scene["gray"], nb, HAND_GRID, 1, *args[1:])
        same(got, want, (table, keep, max_cost))
        assert np.array_equal(got["keys"], keys)


@pytest.mark.parametrize("kind", KINDS)
def test_no_candidate_and_flat_images(hand, kind):
    scene, ctxs = hand["one"]
    t = R.Terms(records(C.hand_cameras()), scene["mask"], scene["bust"], C.HAND_VMIN, C.HAND_VS, C.HAND_DIMS, 1)
    args = (S.HAND_NB, 2, 2, 128, S.GAP, 3, 2)
    empty = np.zeros_like(scene["flags"])
    got = run_stages(ctxs[kind], scene["bust"], empty, scene["gray"], S.HAND_NB, HAND_GRID, 1, *args[1:])
    same(got, reference(t, scene["gray"], empty, *args))
    assert (got["keys"] == S.NONE).all() and not got["agree"].any() and not got["refined"].any() and (got["depth"] == 255).all()
    flat = np.full_like(scene["gray"], 31)
    got = run_stages(ctxs[kind], scene["bust"], scene["flags"], flat, S.HAND_NB, HAND_GRID, 1, *args[1:])
    same(got, reference(t, flat, scene["flags"], *args))
    assert (got["keys"][got["keys"] != S.NONE] >> np.uint64(32) == 0).all() and (got["keys"] != S.NONE).any()


# ------------------------------------------------------------------------------------------------- the textured sphere
SPHERE_GRID = (S.SPHERE_DIMS, S.SPHERE_VMIN, S.SPHERE_VS)


@pytest.fixture(scope="module")
def sphere_ctx(sphere):
    ctxs, planes = contexts(S.sphere_cameras(), sphere[(False, "hull")]["mask"])
    assert np.array_equal(planes, sphere[(False, "hull")]["mask"])
    return ctxs


def _sphere_args():
    return (S.SPHERE_RADIUS, SPHERE["keep"], SPHERE["max_cost"], M255, SPHERE["min_agree"], SPHERE["min_through"])


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("flags", ["hull", "spike"])
@pytest.mark.parametrize("control", [False, True])
def test_sphere_equals_the_restatement(sphere, sphere_ctx, control, flags, kind):
    want = sphere[(control, flags)]
    got = run_stages(sphere_ctx[kind], want["bust"], want["flags"], want["gray"], sphere["neighbours"], SPHERE_GRID,
                     S.SPHERE_CELL, *_sphere_args())
    same(got, want, (control, flags))
    assert (got["keys"] != S.NONE).sum() > 1000 and got["agree"].max() >= 3
    if not control:
        assert 0 < got["refined"].sum() < (want["flags"] != 0).sum() and (got["depth"] != 255).sum() > 500


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257])
def test_a_counted_number_of_candidates(sphere, sphere_ctx, count, kind):
    run = sphere[(False, "spike")]
    hull = np.flatnonzero(run["flags"].reshape(-1))
    flags = np.zeros(run["flags"].size, np.uint8)
    flags[np.random.default_rng([5, count]).choice(hull, count, replace=False)] = 1
    flags = flags.reshape(S.SPHERE_DIMS)
    # (another cell and radius than the scene's own: a cell that does not divide 48, the widest census; one neighbour kept)
    for cell, args in ((S.SPHERE_CELL, _sphere_args()), (5, (3, 1, 700, M255, 1, 1))):
        t = run["terms"] if cell == S.SPHERE_CELL else R.Terms(sphere["records"], run["mask"], run["bust"], S.SPHERE_VMIN,
                                                                 S.SPHERE_VS, S.SPHERE_DIMS, cell)
        want = reference(t, run["gray"], flags, sphere["neighbours"], *args)
        got = run_stages(sphere_ctx[kind], run["bust"], flags, run["gray"], sphere["neighbours"], SPHERE_GRID, cell, *args)
        same(got, want, (count, cell))
        assert int((got["keys"] != S.NONE).sum()) > 0


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("K,keep", WIDE)
def test_sphere_with_wide_tables_equals_the_restatement(sphere, wide, sphere_ctx, K, keep, kind):
    """3, 5 and 8 neighbours whose distances do not arrive in order, keep up to K: every slot of the kernel's list is written"""
    run, w = sphere[(False, "hull")], wide[(K, keep)]
    wide_conditions(run, w, K, keep)
    got = run_stages(sphere_ctx[kind], run["bust"], run["flags"], run["gray"], w["nb"], SPHERE_GRID, S.SPHERE_CELL, S.SPHERE_RADIUS,
                     keep, w["max_cost"], M255, SPHERE["min_agree"], SPHERE["min_through"])
    same(got, w, (K, keep))


def test_stereo_with_five_neighbours_of_which_three_are_kept(sphere, sphere_ctx):
    from monohair_amd import hairstereo

    run = sphere[(False, "hull")]
    cams = sphere_ctx["fp32"].camera_dict
    nb = hairstereo.neighbour_table(cams, 5)
    # (the two views three steps along the ring are equally far but for the rounding of the records: either is the fifth)
    assert nb.shape == (S.SPHERE_V, 5) and np.array_equal(np.sort(nb[:, :4], 1), np.sort(S.sphere_neighbours(4), 1))
    assert all(nb[r, 4] in ((r + 3) % S.SPHERE_V, (r - 3) % S.SPHERE_V) for r in range(S.SPHERE_V))
    want = R.stereo(sphere["records"], run["gray"], run["mask"], run["bust"], S.SPHERE_VMIN, S.SPHERE_VS, S.SPHERE_DIMS,
                    run["flags"], nb, S.SPHERE_CELL, S.SPHERE_RADIUS, 3, SPHERE["max_cost"], M255, SPHERE["min_agree"],
                    SPHERE["min_through"])
    assert 0 < want["refined"].sum() and (want["depth"] != 255).sum() > 100
    for kind in KINDS:
        refined, depth = hairstereo.stereo(sphere_ctx[kind], cams, run["gray"], run["bust"], run["flags"], S.SPHERE_VS,
                                           S.SPHERE_VMIN, neighbours=5, keep=3, radius=S.SPHERE_RADIUS,
                                           max_cost=SPHERE["max_cost"], min_agree=SPHERE["min_agree"])
        assert refined.reshape(-1).tobytes() == want["refined"].tobytes() and depth.tobytes() == want["depth"].tobytes()


@pytest.fixture(scope="module")
def inside_ctx(inside):
    ctxs, planes = contexts(S.inside_cameras(), inside["mask"])
    assert np.array_equal(planes, inside["mask"])
    return ctxs


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("keep", INSIDE_KEEPS)
def test_a_view_inside_the_grid_equals_the_restatement(inside, inside_ctx, keep, kind):
    """a thirteenth view on the plane of a layer of voxel centres (z' = 0 there, where the projection divides by zero), with
    candidates behind it whose pixels lie inside its image: it abstains by the sign of z' alone.  (What the restatement says of
    the scene is asserted by tests/test_hair_stereo_host.py::test_view_inside_the_grid.)"""
    want = inside["runs"][keep]
    got = run_stages(inside_ctx[kind], inside["bust"], inside["flags"], inside["gray"], inside["nb"], SPHERE_GRID, S.SPHERE_CELL,
                     S.SPHERE_RADIUS, keep, SPHERE["max_cost"], M255, SPHERE["min_agree"], SPHERE["min_through"])
    same(got, want, keep)
    assert (got["keys"][S.INSIDE_VIEW] != S.NONE).sum() > 50


def test_stereo_runs_the_stages_and_its_flags_make_a_closed_mesh(sphere, sphere_ctx):
    from monohair_amd import haircarve, hairstereo

    run = sphere[(False, "spike")]
    cams = sphere_ctx["fp32"].camera_dict
    nb = hairstereo.neighbour_table(cams, 2)
    # (the two ring neighbours of a view are equally far but for the rounding of the records: either order)
    assert nb.dtype == np.int32 and np.array_equal(np.sort(nb, 1), np.sort(sphere["neighbours"], 1))
    cell = hairstereo.auto_cell(cams, S.SPHERE_VS, S.SPHERE_VMIN, S.SPHERE_DIMS, (S.SPHERE_HW, S.SPHERE_HW))
    # a voxel of 1/128 at depth 1 under a focal length of 10 over 48 pixels: 10 * 48 / 2 / 128 = 1.875 pixels
    assert cell == 2 == S.SPHERE_CELL
    assert hairstereo.margin255(SPHERE["margin_vox"], S.SPHERE_VS) == M255
    for kind in KINDS:
        refined, depth = hairstereo.stereo(sphere_ctx[kind], cams, run["gray"], run["bust"], run["flags"], S.SPHERE_VS,
                                           S.SPHERE_VMIN, radius=S.SPHERE_RADIUS, max_cost=SPHERE["max_cost"],
                                           min_agree=SPHERE["min_agree"])
        assert refined.tobytes() == run["refined"].tobytes() and depth.tobytes() == run["depth"].tobytes()
        assert refined.shape == S.SPHERE_DIMS
    v, t = haircarve.hull_mesh(refined, S.SPHERE_VMIN, S.SPHERE_VS)
    CARVE.check_mesh(refined, v, t, S.SPHERE_VS)
    assert len(t) > 0


def test_gray_planes():
    from monohair_amd import hairstereo

    rng = np.random.default_rng(3)
    bgr = rng.integers(0, 256, (2, 5, 7, 3), dtype=np.uint8)
    bgr[0, 0, 0], bgr[0, 0, 1] = (255, 255, 255), (0, 0, 0)
    g = hairstereo.gray_planes([bgr[0], bgr[1]])
    b = bgr.astype(np.int64)
    assert g.dtype == np.uint8 and np.array_equal(g, (29 * b[..., 0] + 150 * b[..., 1] + 77 * b[..., 2] + 128) >> 8)
    assert g[0, 0, 0] == 255 and g[0, 0, 1] == 0
    plain = rng.integers(0, 256, (5, 7), dtype=np.uint8)
    assert np.array_equal(hairstereo.gray_planes({"a": plain, "b": np.stack([plain] * 3, -1)}), np.stack([plain, plain]))
    with pytest.raises(ValueError):
        hairstereo.gray_planes([plain, plain[:4]])


# ------------------------------------------------------------------------------------------------- the command
V_CMD, H_CMD, W_CMD = 6, 96, 54
CMD_CARVE = ["--voxel-size", "0.005"]


def test_command_writes_the_refined_mesh_and_depth_and_guards_an_existing_file(tmp_path, capsys, monkeypatch):
    """a small synthetic capture of photographs: the command's files are the API's, step by step"""
    import os
    import shutil

    import PMVO as cli
    from monohair_amd import gridviews, haircarve, hairstereo, synth_hair
    from monohair_amd.camera import camera_records, load_cam, parsing_camera
    from monohair_amd.pmvo_utils import load_bust, map_code_lut, read_obj

    data = str(tmp_path / "data")
    base = synth_hair.write_case(data, "synthetic_hair", V=V_CMD, H=H_CMD, W=W_CMD, seed=0, n_strands=300, n_points=32, photo=True)
    obj, depth_dir = os.path.join(base, "ours", "colmap_points.obj"), os.path.join(base, "render_depth")
    os.remove(obj)
    shutil.rmtree(depth_dir)
    argv = ["--yaml=configs/reconstruct/synthetic_hair", "--data.root=%s" % data, "--data.image_size=[%d,%d]" % (H_CMD, W_CMD),
            "--PMVO.patch_size=3", "--name=t"]
    monkeypatch.chdir(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    own = ["--max-cost", "1024", "--min-agree", "1", "--min-through", "1", "--margin-vox", "1"]      # bounds that remove a lot
    assert hairstereo.main(argv + CMD_CARVE + own) == 0
    out = capsys.readouterr().out
    args = cli.config_parser(argv)
    camera = parsing_camera(load_cam(args.image_camera_path), os.path.join(args.data.root, "capture_images"))
    masks = haircarve.load_masks(camera, args.data.mask_path)
    gray = hairstereo.load_gray(camera, os.path.join(args.data.root, "capture_images"))
    assert gray.shape == (V_CMD, H_CMD, W_CMD) and gray.dtype == np.uint8 and len(np.unique(gray)) > 16
    bv, bf, _ = load_bust(args.data.bust_path)
    bust = (bv + args.bust_to_origin, bf)
    _, _, hull = haircarve.carve(masks, camera, bust, 0.005, voxel_min=args.bbox_min, image_size=[H_CMD, W_CMD])
    pmvo = haircarve.mask_context(masks, camera, [H_CMD, W_CMD])
    refined, cells = hairstereo.stereo(pmvo, camera, gray, bust, hull, 0.005, args.bbox_min, max_cost=1024, min_agree=1,
                                       min_through=1, margin_vox=1.0)
    removed = int(hull.sum()) - int(refined.sum())
    assert 0 < removed < int(hull.sum()) and not (refined & ~hull).any()
    assert "the refinement removed %d, %d remain" % (removed, int(refined.sum())) in out
    assert "%d of %d cells have a confirmed winner" % (int((cells != 255).sum()), cells.size) in out
    v, t = haircarve.hull_mesh(refined, args.bbox_min, 0.005)
    fv, ft = read_obj(obj)
    assert np.array_equal(ft, t) and np.abs(fv + np.asarray(args.bust_to_origin) - v.astype(np.float64)).max() <= 1e-9
    depth = haircarve.carve_depth(pmvo, v, t, bust, 0.0)
    views = list(camera.keys())
    got = np.stack([np.load(os.path.join(depth_dir, view + ".npy"))[..., 0] for view in views])
    assert got.dtype == F and got.tobytes() == depth.tobytes()
    # the restatement on the same inputs
    planes = gridviews.bust_planes(pmvo, bust).cpu().numpy()
    mask = np.stack([masks[k] for k in views])
    vmin, vs, dims = gridviews.grid(args.bbox_min, 0.005, hull.shape)
    cell = hairstereo.auto_cell(camera, vs, vmin, dims, (H_CMD, W_CMD))
    want = R.stereo(camera_records(camera), gray, np.ascontiguousarray(map_code_lut()[mask][..., 3]), planes, vmin, vs,
                    hull.shape, hull, hairstereo.neighbour_table(camera, 2), cell, 2, 2, 1024, hairstereo.margin255(1.0, vs), 1, 1)
    assert want["refined"].tobytes() == refined.tobytes() and want["depth"].tobytes() == cells.tobytes()
    # an existing colmap_points.obj may be instant-ngp's: refused without --force, and left as it is
    first = open(obj, "rb").read()
    with pytest.raises(SystemExit) as e:
        hairstereo.main(argv + CMD_CARVE)
    assert "--force" in str(e.value) and open(obj, "rb").read() == first
    assert hairstereo.main(argv + CMD_CARVE + ["--force", "--max-cost", "0", "--min-agree", "24"]) == 0      # nothing is confirmed
    assert "the refinement removed 0," in capsys.readouterr().out
    hv, ht = haircarve.hull_mesh(hull, args.bbox_min, 0.005)
    assert np.array_equal(read_obj(obj)[1], ht) and open(obj, "rb").read() != first


# ------------------------------------------------------------------------------------------------- refusals
def test_bad_arguments_are_refused(hand):
    import torch

    from monohair_amd import _lib, hairstereo

    scene, ctxs = hand["one"]
    ctx = ctxs["fp32"]
    call = lambda **kw: hairstereo.stereo_winners(ctx, scene["bust"], scene["flags"], scene["gray"],          # noqa: E731
                                                  kw.pop("nb", S.HAND_NB), *HAND_GRID, **kw)
    for kw in (dict(keep=3), dict(keep=0), dict(radius=4), dict(radius=0), dict(cell=0), dict(cell=257)):
        with pytest.raises(ValueError):
            call(**kw)
    own = S.HAND_NB.copy()
    own[3, 1] = 3          # a row that names itself
    for nb in (own, np.full((8, 2), 8, np.int32), S.HAND_NB[:7], np.zeros((8, 9), np.int32) - 1):
        with pytest.raises(ValueError):
            call(nb=nb)
    # ... and at the C ABI
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    dims, vmin = np.array(C.HAND_DIMS, np.int32), np.array(C.HAND_VMIN, np.float64)
    bust = torch.from_numpy(scene["bust"]).cuda()
    gray = torch.from_numpy(scene["gray"]).cuda()
    flags = torch.from_numpy(scene["flags"].reshape(-1)).cuda()
    cand = torch.arange(128, dtype=torch.int32, device="cuda")
    nb = torch.from_numpy(S.HAND_NB).cuda()
    sentinel = 0x5A5A5A5A5A5A5A5A
    census = torch.full((8, 8, 8), sentinel, dtype=torch.int64, device="cuda")
    reduced = torch.full((8, 8, 8), 7, dtype=torch.uint8, device="cuda")
    keys = torch.full((8, 8, 8), sentinel, dtype=torch.int64, device="cuda")
    agree = torch.full((128,), -9, dtype=torch.int32, device="cuda")
    refined = torch.full((128,), 7, dtype=torch.uint8, device="cuda")
    depth = torch.full((8, 8, 8), -3.0, dtype=torch.float32, device="cuda")
    hp = _lib.host_ptr

    def census_rc(cell=1, radius=1):
        return L.mh_stereo_census(ctx._ctx, p(gray), 8, 8, 8, cell, radius, p(reduced), p(census), st)

    def winners_rc(K=2, cell=1, radius=1, keep=2, n=128):
        return L.mh_stereo_winners(ctx._ctx, p(bust), hp(vmin), C.HAND_VS, hp(dims), p(cand), n, p(census), p(nb), K, cell, radius,
                                   keep, p(keys), st)

    def agree_rc(cell=1, max_cost=128, m255=1.0):
        return L.mh_stereo_agree(ctx._ctx, p(bust), hp(vmin), C.HAND_VS, hp(dims), p(flags), p(keys), cell, max_cost, m255,
                                 p(agree), st)

    def refine_rc(cell=1, max_cost=128, m255=1.0, min_agree=3, min_through=2):
        return L.mh_stereo_refine(ctx._ctx, p(bust), hp(vmin), C.HAND_VS, hp(dims), p(flags), p(keys), p(agree), cell, max_cost,
                                  m255, min_agree, min_through, p(refined), p(depth), st)

    bad = [census_rc(cell=0), census_rc(radius=4), census_rc(cell=257), winners_rc(keep=3), winners_rc(K=9, keep=1),
           winners_rc(cell=0), winners_rc(radius=4), winners_rc(keep=0), winners_rc(n=-1), agree_rc(cell=0),
           agree_rc(max_cost=-1), agree_rc(m255=float("nan")), agree_rc(m255=-1.0), refine_rc(cell=0), refine_rc(min_agree=0),
           refine_rc(min_through=0), refine_rc(m255=float("inf"))]
    assert all(rc != 0 for rc in bad), bad
    torch.cuda.synchronize()
    # a refused call has written nothing
    assert (census == sentinel).all() and (reduced == 7).all() and (keys == sentinel).all() and (agree == -9).all() and \
        (refined == 7).all() and (depth == -3.0).all()
    assert census_rc() == 0 and winners_rc() == 0
