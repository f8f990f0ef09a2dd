"""GPU: the capture agreement (csrc/hairreproj.hip, monohair_amd/hairreproj.py) against the numpy restatement of its rule
(tests/hair_reproj_np.py): every counter EQUAL -- per strand, per view, the silhouette, the dropped segments.  As in
tests/test_hair_capture_gpu.py the segment cases are built in pixel space and handed to the per-step entry points as vertices,
so that each one sits exactly where it is meant to; world points go through support_counts (mh_support_view)."""
import ctypes
import os

import numpy as np
import pytest

import hair_reproj_np as hr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
ANGLES = (10, 20, 30)
up = lambda x: np.nextafter(F32(x), F32(np.inf))          # noqa: E731


def device_support(vert, valid, counts, H, W, planes, conf_min, bounds, radius=1, tol=0.25, depth0=None, strand_init=None):
    """the per-step entry points on given vertices -> the dict hair_reproj_np.support returns"""
    import torch

    from monohair_amd import _lib
    from monohair_amd.pmvo_utils import _ctx_for
    from monohair_amd.synth_hair import code_table

    L, ctx, st = _lib.lib(), _ctx_for(DEV), _lib.stream_ptr()
    counts = np.asarray(counts, np.int64).reshape(-1)
    offs = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    n, S = int(offs[-1]), len(counts)
    bounds = np.ascontiguousarray(bounds, np.float64)
    K = bounds.shape[0]
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(DEV)          # noqa: E731
    vert_d, valid_d, offs_d = dv(np.reshape(vert, (-1, 3)), F32), dv(valid, np.uint8), dv(offs, np.int64)
    ori, conf, mask = (dv(a, np.uint8) for a in planes)
    d0 = None if depth0 is None else dv(depth0, F32)
    zmin = torch.empty((H, W), dtype=torch.float32, device=DEV)
    dropped = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    strand = dv(np.zeros((max(S, 1), hr.COLS + K), np.int64) if strand_init is None else strand_init, np.int64)
    view = torch.full((hr.COLS + K,), -7, dtype=torch.int64, device=DEV)
    sil = torch.full((3,), -7, dtype=torch.int64, device=DEV)
    table = code_table()
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    p = _lib.ptr
    _lib.check(L.mh_capture_zmin(ctx, p(vert_d), p(valid_d), p(offs_d), S, n, H, W, radius, p(d0), p(zmin), p(dropped), st))
    _lib.check(L.mh_support_accumulate(ctx, p(vert_d), p(valid_d), p(offs_d), S, n, H, W, float(tol), p(d0), p(zmin), p(ori),
                                       p(conf), p(mask), int(conf_min), hp(table), hp(bounds), K, p(strand), p(view), st))
    _lib.check(L.mh_support_silhouette(ctx, p(zmin), p(mask), H, W, p(sil), st))
    torch.cuda.synchronize()
    return dict(strand=strand.cpu().numpy()[:S], view=view.cpu().numpy(), silhouette=sil.cpu().numpy(),
                zmin=zmin.cpu().numpy(), dropped=int(dropped.item()))


def assert_same(got, ref, what):
    for k in ("zmin", "strand", "view", "silhouette"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k, got[k].shape, ref[k].shape)
        assert got[k].tobytes() == ref[k].tobytes(), "%s: %s differs in %d places" % (what, k, int((got[k] != ref[k]).sum()))
    assert got["dropped"] == int(ref["view"][3]), what


def random_planes(rng, H, W):
    """per-pixel codes over all 256 values, each plane on its own"""
    return tuple(rng.integers(0, 256, (H, W), dtype=np.uint8) for _ in range(3))


def walk(rng, n_points, H, W, z=100.0):
    """a strand of n_points that stays about the image: steps of about a pixel, depth within a few tol of z"""
    start = rng.uniform([0, 0, z - 0.3], [H, W, z + 0.3])
    steps = rng.normal(0, [0.9, 0.9, 0.05], (max(n_points - 1, 0), 3))
    pts = np.concatenate([start[None], start[None] + np.cumsum(steps, 0)]) if n_points else np.zeros((0, 3))
    pts[:, 0] = np.clip(pts[:, 0], -3, H + 3)
    pts[:, 1] = np.clip(pts[:, 1], -3, W + 3)
    return pts.astype(F32)


def case_strands(view, H, W, n_random, seed, walks=True):
    """-> (strands [n,3] (row, col, z255), valid flags, occluder).  The hand cases of tests/test_hair_reproj_host.py, segments
    across each border and wholly outside, an invalid end, the 8192- / 8193-sample segments, then strands of 1, 2, 3, 64, 65 and
    513 points between short ones -- strand boundaries inside a wave, a strand over several waves, one over several blocks --
    and n_random seeded segments in strands of 1..6 points."""
    rng = np.random.default_rng(seed + 100 * view)
    S = [
        [(5, 2, 100), (5, 10, 100)],                                      # the horizontal strand of the host file
        [(9, 3, 100), (6, 7, 100)],                                       # qc = 1147, qs = 3932
        [(3, 3, 100), (3, 3, 100)],                                       # zero length
        [(7, 7, 100), (7, 7, 100)], [(7, 7, 100.25), (7, 7, 100.25)], [(7, 7, up(100.25)), (7, 7, up(100.25))],
        [(8, 8, 100), (8, 8, 100)], [(8, 8, up(100)), (8, 8, up(100))],   # at the equal-depth occluder and one ulp behind
        [(-3.3, 10.2, 90), (4.1, 12.7, 91)], [(H - 3.4, 20.1, 92), (H + 3.2, 22.4, 93)],          # across the borders
        [(10.3, -4.2, 94), (12.1, 3.6, 95)], [(15.5, W - 3.7, 96), (17.2, W + 3.8, 97)],
        [(-10, -10, 90), (-5, -3, 90)], [(H + 8, W + 6, 90), (H + 13, W + 16, 90)],               # wholly outside
        [(5, -5000, 100), (5, 5000, 100)],                                # n > 8192: dropped and counted
        [(6, -4000.25, 100), (6, 4191.75, 100)],                          # n = 8192
        [(20.5, 40.5, 100), (20.5, 40.5, 100)], [(8, 20, 100), (8, 24, 100.5)],                   # centres on k + 0.5
    ]
    V = [[1] * len(s) for s in S]
    S.append([(10, 45, 100), (11, 50, 100), (12, 55, 100), (13, 58, 100)])
    V.append([1, 0, 1, 1])
    S.append([(np.nan, 45, 100), (18, 50, np.inf), (19, 55, 100), (19, 58, 100)])
    V.append([0, 0, 1, 1])
    S = [np.array(s, F32).reshape(-1, 3) for s in S]
    for n_points in (1, 2, 3, 64, 3, 65, 2, 513, 1, 0, 4) if walks else ():
        S.append(walk(rng, n_points, H, W))
        V.append([1] * n_points)
    left = n_random
    while left > 0:
        k = int(min(left, rng.integers(1, 6)))
        start = rng.uniform([-4, -4, 98], [H + 4, W + 4, 102])
        steps = rng.normal(0, [3.0, 3.0, 0.2], (k, 3))
        if rng.random() < 0.2:
            steps[:, :2] = np.rint(steps[:, :2])
            start[:2] = np.rint(start[:2] * 2) / 2
        S.append(np.concatenate([start[None], start[None] + np.cumsum(steps, 0)]).astype(F32))
        V.append(list((rng.random(k + 1) > 0.03).astype(np.uint8)))
        left -= k
    depth0 = None
    if view % 3 == 1:
        depth0 = np.full((H, W), 100, F32)
    elif view % 3 == 2:
        depth0 = rng.uniform(99, 103, (H, W)).astype(F32)
        depth0[rng.random((H, W)) < 0.3] = 255
    return S, [np.array(v, np.uint8) for v in V], depth0


def check_view(view, H, W, n_random, radius, seed=0, tol=0.25, use_occluder=True, angles=ANGLES):
    S, V, depth0 = case_strands(view, H, W, n_random, seed)
    if not use_occluder:
        depth0 = None
    vert, valid, counts = np.concatenate(S), np.concatenate(V), [len(s) for s in S]
    planes = random_planes(np.random.default_rng(1000 + seed + view), H, W)
    bounds, cmin = hr.bounds_of(angles), hr.conf_min_code(0.15)
    ref = hr.support(vert, valid, counts, H, W, *planes, cmin, bounds, radius=radius, tol=tol, depth0=depth0)
    got = device_support(vert, valid, counts, H, W, planes, cmin, bounds, radius, tol, depth0)
    assert_same(got, ref, "view %d radius %d tol %g" % (view, radius, tol))
    return got, (vert, valid, counts, planes, depth0, bounds, cmin)


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_edge_cases_equal_the_restatement(radius):
    H, W = 32, 64
    for view in range(3):
        for tol in (0.0, 0.25):
            got, (vert, valid, counts, planes, depth0, bounds, cmin) = check_view(view, H, W, 240, radius, tol=tol)
            assert got["dropped"] == 1 and got["view"][0] > 0
        assert got["view"][0] > 100 and got["view"][2] > 20 and got["view"][4] > 0          # (the run at tol 0.25)
        check_view(view, H, W, 240, radius, use_occluder=False)
        # run to run: the integer atomics leave the same numbers; and a second call ADDS to the strand rows
        again = device_support(vert, valid, counts, H, W, planes, cmin, bounds, radius, 0.25, depth0, strand_init=got["strand"])
        assert again["strand"].tobytes() == (2 * got["strand"]).tobytes() and again["view"].tobytes() == got["view"].tobytes()
    # the hand cases of the host file alone, on planes of one code each (view 0: no occluder; view 1: the plane of 100)
    for view, want8 in ((0, [1, 1, 0, 1, 1]), (1, [1, 0, 0, 1, 0])):
        S, V, depth0 = case_strands(view, H, W, 0, 0, walks=False)
        vert, valid, counts = np.concatenate(S), np.concatenate(V), [len(s) for s in S]
        flat = (np.full((H, W), 45, np.uint8), np.full((H, W), 39, np.uint8), np.full((H, W), 52, np.uint8))
        T = hr.hc.code_table().astype(np.float64)
        exact = 1147.0 * T[45, 0] + 3932.0 * T[45, 1]
        bounds = [exact, np.nextafter(exact, np.inf)]
        got = device_support(vert, valid, counts, H, W, flat, 39, bounds, 0, 0.25, depth0)
        assert_same(got, hr.support(vert, valid, counts, H, W, *flat, 39, bounds, radius=0, tol=0.25, depth0=depth0), "flat")
        assert got["strand"][1].tolist() == [4, 4, 4, 0, 4, 0] and got["strand"][2].tolist() == [1, 1, 1, 0, 0, 0]
        assert got["strand"][3:8, 0].tolist() == want8
        for planes, col in (((flat[0], flat[1], flat[2] - 1), 1), ((flat[0], flat[1] - 1, flat[2]), 2),
                            ((flat[0] + 135, flat[1], flat[2]), 2)):
            got = device_support(vert, valid, counts, H, W, planes, 39, bounds, 0, 0.25, depth0)
            assert got["view"][0] > 0 and got["view"][col] == 0 and got["view"][col - 1] > 0


def test_seeded_sweep_and_odd_image_sizes():
    for view in range(5):
        got, _ = check_view(view, 48, 80, 2000, 1, seed=11)
        assert got["view"][2] > 100 and got["silhouette"].sum() > 0
    for (H, W), radius in (((17, 37), 2), ((1, 1), 1), ((5, 130), 0)):
        check_view(2, H, W, 150, radius, seed=3)


def test_empty_and_degenerate_strand_sets():
    H, W = 32, 64
    planes = random_planes(np.random.default_rng(5), H, W)
    d0 = np.full((H, W), 77, F32)
    for counts in ([], [0, 0], [1], [1, 0, 1]):
        n = int(sum(counts))
        vert = np.tile(np.array([[5, 5, 60]], F32), (n, 1))
        got = device_support(vert, np.ones(n, np.uint8), counts, H, W, planes, 39, hr.bounds_of(ANGLES), depth0=d0)
        assert_same(got, hr.support(vert, np.ones(n, np.uint8), counts, H, W, *planes, 39, hr.bounds_of(ANGLES), depth0=d0),
                    str(counts))
        assert not got["strand"].any() and not got["view"].any() and got["silhouette"][:2].tolist() == [0, 0]
        assert got["silhouette"][2] == int((planes[2] >= 52).sum())


@pytest.mark.parametrize("n_bounds", [1, 8])
def test_one_and_eight_bounds(n_bounds):
    angles = np.linspace(2, 88, n_bounds)
    got, _ = check_view(1, 32, 64, 240, 1, seed=2, angles=angles)
    assert got["strand"].shape[1] == 4 + n_bounds
    if n_bounds == 8:
        assert (np.diff(got["view"][4:]) >= 0).all() and got["view"][-1] > got["view"][4]      # wider bounds hold more


def test_nine_bounds_and_bad_arguments_are_refused():
    import torch

    from monohair_amd import _lib, hairreproj
    from monohair_amd.pmvo_utils import _ctx_for
    from monohair_amd.synth_hair import code_table

    with pytest.raises(ValueError):
        hairreproj.angle_bounds(np.linspace(2, 88, 9))
    L, ctx, st = _lib.lib(), _ctx_for(DEV), _lib.stream_ptr()
    H, W = 8, 8
    z = lambda shape, t: torch.zeros(shape, dtype=t, device=DEV)      # noqa: E731
    vert, valid, offs = z((2, 3), torch.float32), z(2, torch.uint8), torch.tensor([0, 2], device=DEV)
    zmin, plane = z((H, W), torch.float32), z((H, W), torch.uint8)
    strand, view = z((1, 13), torch.int64), z(13, torch.int64)
    table, bounds = code_table(), np.zeros(9, np.float64)
    hp = lambda a: a.ctypes.data_as(ctypes.c_void_p)      # noqa: E731
    p = _lib.ptr

    def rc(n_bounds=3, tol=0.25, cmin=39, H=H, W=W):
        return L.mh_support_accumulate(ctx, p(vert), p(valid), p(offs), 1, 2, H, W, tol, None, p(zmin), p(plane), p(plane),
                                       p(plane), cmin, hp(table), hp(bounds), n_bounds, p(strand), p(view), st)

    assert rc() == 0 and rc(n_bounds=8) == 0 and rc(n_bounds=1) == 0
    for kw in (dict(n_bounds=9), dict(n_bounds=0), dict(tol=-1.0), dict(tol=float("nan")), dict(cmin=257), dict(cmin=-1),
               dict(H=0), dict(H=1 << 16, W=1 << 15)):
        assert rc(**kw) != 0, kw
    scratch = z(int(L.mh_support_scratch_bytes(2, H, W)), torch.uint8)
    cam, pts, sil = np.zeros(48, F32), z((2, 3), torch.float32), z(3, torch.int64)

    def view_rc(radius=1, nbytes=scratch.numel()):
        return L.mh_support_view(ctx, hp(cam), p(pts), p(offs), 1, 2, H, W, radius, 0.25, None, p(plane), p(plane), p(plane), 39,
                                 hp(table), hp(bounds), 3, p(scratch), nbytes, p(strand), p(view), p(sil), st)

    assert view_rc(radius=17) != 0 and view_rc(radius=-1) != 0 and view_rc(nbytes=scratch.numel() - 1) != 0
    assert L.mh_support_scratch_bytes(2, 1 << 16, 1 << 15) == 0
    torch.cuda.synchronize()


@pytest.fixture(scope="module")
def world():
    """a small world-space strand set in front of three cameras, with points a projection must refuse, and the bust"""
    import tempfile

    from monohair_amd import synth, synth_hair as sh
    from monohair_amd.camera import cameras_from_list
    from monohair_amd.pmvo_utils import read_obj

    H, W = 32, 64
    cams = cameras_from_list(synth.make_cameras(3, H, W))
    counts, pts = sh.make_hairstyle(40, 8, seed=4)
    pts = pts.copy()
    pts[25] = (np.nan, 0.0, 0.0)
    pts[33] = (np.inf, 0.0, 0.0)
    pts[57] = (1.0e5, 0.0, 0.05)
    with tempfile.TemporaryDirectory() as d:
        synth.sphere_obj(os.path.join(d, "b.obj"), sh.BUST_R, 12, 24)
        bust = read_obj(os.path.join(d, "b.obj"))
    return H, W, cams, counts, pts, bust


@pytest.mark.parametrize("with_bust", [False, True])
def test_one_call_equals_the_steps_and_views_add_up(world, with_bust):
    import torch

    from monohair_amd import _lib, hairreproj, synth_hair as sh
    from monohair_amd.camera import camera_records
    from monohair_amd.pmvo_utils import _ctx_for

    H, W, cams, counts, pts, bust = world
    bust = bust if with_bust else None
    V = len(cams)
    rng = np.random.default_rng(8)
    planes = tuple(rng.integers(0, 256, (V, H, W), dtype=np.uint8) for _ in range(3))
    b2o = (0.001, -0.002, 0.0005)
    stored = (pts.astype(np.float64) - np.array(b2o)).astype(F32)           # what a .hair file would hold
    kw = dict(bust=bust, bust_to_origin=b2o, angles_deg=ANGLES, conf_threshold=0.15, radius=1, tol=0.25, device=DEV)
    sc, vc, sil, det = hairreproj.support_counts((counts, stored), cams, planes, return_details=True, **kw)
    sc2, vc2, sil2 = hairreproj.support_counts((counts, stored), cams, planes, **kw)
    assert sc.tobytes() == sc2.tobytes() and vc.tobytes() == vc2.tobytes() and sil.tobytes() == sil2.tobytes()
    assert det.shape == (V, len(counts), 7) and np.array_equal(det.sum(0), sc) and np.array_equal(det.sum(1), vc)
    assert sc[:, 0].sum() > 100 and sc[:, 2].sum() > 10
    # the steps one by one on the vertices the projection makes, and the restatement on the same vertices
    world_pts = (stored.astype(np.float64) + np.array(b2o)).astype(F32)
    recs = np.ascontiguousarray(camera_records(cams), F32)
    L, ctx, st = _lib.lib(), _ctx_for(DEV), _lib.stream_ptr()
    n = len(world_pts)
    pts_d = torch.from_numpy(world_pts).to(DEV)
    depth0 = [None] * V
    if bust is not None:
        from monohair_amd.render import DepthRenderer

        r = DepthRenderer([bust], DEV)
        depth0 = [r.render(recs[v], H, W, 0.0).cpu().numpy() for v in range(V)]
    bounds, cmin = hr.bounds_of(ANGLES), hr.conf_min_code(0.15)
    total = np.zeros_like(sc)
    for v in range(V):
        vert = torch.empty((n, 3), dtype=torch.float32, device=DEV)
        valid = torch.empty(n, dtype=torch.uint8, device=DEV)
        _lib.check(L.mh_capture_project(ctx, recs[v].ctypes.data_as(ctypes.c_void_p), _lib.ptr(pts_d), n, H, W, _lib.ptr(vert),
                                        _lib.ptr(valid), st))
        vert, valid = vert.cpu().numpy(), valid.cpu().numpy()
        assert not valid[[25, 33]].any()
        view_planes = tuple(a[v] for a in planes)
        got = device_support(vert, valid, counts, H, W, view_planes, cmin, bounds, 1, 0.25, depth0[v])
        ref = hr.support(vert, valid, counts, H, W, *view_planes, cmin, bounds, radius=1, tol=0.25, depth0=depth0[v])
        assert_same(got, ref, "world view %d" % v)
        assert got["strand"].tobytes() == det[v].tobytes() and got["view"].tobytes() == vc[v].tobytes()
        assert got["silhouette"].tobytes() == sil[v].tobytes()
        total += got["strand"]
    assert total.tobytes() == sc.tobytes()
    if with_bust:
        free = hairreproj.support_counts((counts, stored), cams, planes, **dict(kw, bust=None))
        assert free[0][:, 0].sum() > sc[:, 0].sum()                        # the bust hides samples


def test_a_captures_own_strands_lie_on_its_hair(world):
    from monohair_amd import hairreproj, synth_hair as sh

    H, W, cams, _, _, bust = world
    strands = sh.make_hairstyle(60, 12, seed=6)
    for radius, tol in ((1, 0.25), (0, 0.0), (2, 1.0)):
        depth, ori, conf, mask = sh.capture_planes(strands, cams, H, W, radius=radius, tol=tol, bust=bust, device=DEV)
        sc, vc, sil = hairreproj.support_counts(strands, cams, (ori, conf, mask), bust=bust, radius=radius, tol=tol, device=DEV)
        # a visible sample's centre pixel received that sample's fragment in pass B
        assert sc[:, 0].sum() > 100 and np.array_equal(sc[:, 1], sc[:, 0]) and np.array_equal(vc[:, 1], vc[:, 0])
        assert (sil[:, 1:] == 0).all() and (sil[:, 0] > 0).all()           # predicted == observed, pixel for pixel
        res = hairreproj.build_result(ANGLES, 0.15, radius, tol, sc, vc, sil, len(strands[1]))
        assert res["overall"]["coverage"] == 1.0 and res["overall"]["silhouette"]["iou"] == 1.0
