"""GPU: the hair capture (csrc/haircapture.hip, monohair_amd/synth_hair.py) against the numpy restatement of its rule
(tests/hair_capture_np.py): every quantity EQUAL, not close -- the four planes, cnt, C2, S2, zmin and the dropped count.  The
segment cases are built in pixel space and handed to the per-step entry points as vertices, so that each one sits exactly
where it is meant to (a centre on k + 0.5, a length one ulp past an integer); the projection that makes such vertices from
world points is held to mh_project_points separately, and the planes to the files write_case writes."""
import ctypes
import os

import numpy as np
import pytest

import hair_capture_np as hc

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
KEYS = ("depth", "ori_u8", "conf_u8", "mask_u8", "zmin", "cnt", "c2", "s2")


def device_capture(vert, valid, counts, H, W, radius, tol=0.25, depth0=None, n_full=None):
    """the three per-step entry points on given vertices -> the dict hair_capture_np.capture returns"""
    import torch

    from monohair_amd import _lib
    from monohair_amd.pmvo_utils import _ctx_for
    from monohair_amd.synth_hair import code_table

    L, ctx, st = _lib.lib(), _ctx_for(DEV), _lib.stream_ptr()
    counts = np.asarray(counts, np.int64).reshape(-1)
    offs = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    n, S = int(offs[-1]), len(counts)
    dv = lambda a, t: torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(DEV)          # noqa: E731
    vert_d, valid_d, offs_d = dv(np.reshape(vert, (-1, 3)), F32), dv(valid, np.uint8), dv(offs, np.int64)
    d0 = None if depth0 is None else dv(depth0, F32)
    zmin = torch.empty((H, W), dtype=torch.float32, device=DEV)
    cnt = torch.empty((H, W), dtype=torch.int32, device=DEV)
    c2, s2 = (torch.empty((H, W), dtype=torch.int64, device=DEV) for _ in range(2))
    dropped = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    depth = torch.empty((H, W), dtype=torch.float32, device=DEV)
    ori, conf, mask = (torch.empty((H, W), dtype=torch.uint8, device=DEV) for _ in range(3))
    table = code_table()
    p = _lib.ptr
    _lib.check(L.mh_capture_zmin(ctx, p(vert_d), p(valid_d), p(offs_d), S, n, H, W, radius, p(d0), p(zmin), p(dropped), st))
    _lib.check(L.mh_capture_accumulate(ctx, p(vert_d), p(valid_d), p(offs_d), S, n, H, W, radius, float(tol), p(d0), p(zmin),
                                       p(cnt), p(c2), p(s2), st))
    _lib.check(L.mh_capture_resolve(ctx, p(zmin), p(cnt), p(c2), p(s2), p(d0), table.ctypes.data_as(ctypes.c_void_p),
                                    2 * radius + 1 if n_full is None else n_full, H, W, p(depth), p(ori), p(conf), p(mask),
                                    st))
    torch.cuda.synchronize()
    out = dict(depth=depth, ori_u8=ori, conf_u8=conf, mask_u8=mask, zmin=zmin, cnt=cnt, c2=c2, s2=s2)
    out = {k: v.cpu().numpy() for k, v in out.items()}
    out["dropped"] = int(dropped.item())
    return out


def assert_same(got, ref, what):
    assert got["dropped"] == ref["dropped"], (what, got["dropped"], ref["dropped"])
    for k in KEYS:
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        assert got[k].tobytes() == ref[k].tobytes(), "%s: %s differs at %d pixels" % (what, k, int((got[k] != ref[k]).sum()))


def edge_strands(H, W):
    """-> (list of [n,3] float32 (row, col, z255) strands, list of valid flags).  One strand per case of the rule."""
    up = lambda x: np.nextafter(F32(x), F32(np.inf))          # noqa: E731
    S = [
        [(-3.3, 10.2, 90), (4.1, 12.7, 91)],                              # across the top border
        [(H - 3.4, 20.1, 92), (H + 3.2, 22.4, 93)],                       # ... the bottom
        [(10.3, -4.2, 94), (12.1, 3.6, 95)],                              # ... the left
        [(15.5, W - 3.7, 96), (17.2, W + 3.8, 97)],                       # ... the right
        [(-10, -10, 90), (-5, -3, 90)], [(H + 8, W + 6, 90), (H + 13, W + 16, 90)],     # wholly outside
        [(-4, 5, 90), (-4, 40, 90)],                                      # outside along a border, footprint may reach in
        [(5.25, 10.25, 100), (5.25, 14.25, 100)],                         # n exactly at an integer length: 4 samples
        [(7.25, 10.25, 100), (7.25, up(14.25), 100)],                     # ... one ulp above: 5
        [(9.25, 10.25, 100), (up(13.25), 10.25, 100)],
        [(8, 20, 100), (8, 24, 100.5)], [(10, 30, 100), (13, 30, 99)],    # centres exactly on k + 0.5 (half to even)
        [(20.5, 40.5, 100), (20.5, 40.5, 100)], [(21.5, 41.5, 100.1), (22.5, 42.5, 100.1)],
        [(0, 0, 80), (0, 0, 80)], [(H - 1, W - 1, 80), (H - 1, W - 1, 80)],           # footprints clipped at the corners
        [(0, W - 1, 80), (0.4, W - 0.6, 80)], [(H - 1, 0, 80), (H - 0.6, 0.3, 80)],
        [(5, -5000, 100), (5, 5000, 100)],                                # n > 8192: dropped and counted
        [(6, -4000.25, 100), (6, 4191.75, 100)],                          # n = 8192: drawn
        [(3, 3, 50)],                                                     # a strand of one point
        [],                                                               # an empty strand
        [(12, 5, 100), (14, 9, 100), (16.5, 9.5, 100), (16.5, 15, 100.2), (12, 15, 100.4), (12.2, 5.1, 100.1)],   # a loop
        [(25.2, 5.3, 70), (25.9, 50.2, 120)],                             # a depth ramp under ...
        [(20.1, 30.2, 95.1), (30.3, 30.9, 95.2)],                         # ... a crossing strand
        [(2, 50, 100), (2.2, 50.1, 100), (2.3, 50.3, 100.3)],             # sub-pixel segments on one pixel
    ]
    V = [[1] * len(s) for s in S]
    # one end behind the near plane / not finite: the projection marks such a vertex invalid and both its segments go
    S.append([(10, 45, 100), (11, 50, 100), (12, 55, 100), (13, 58, 100)])
    V.append([1, 0, 1, 1])
    S.append([(np.nan, 45, 100), (18, 50, np.inf), (19, 55, 100), (19, 58, 100)])
    V.append([0, 0, 1, 1])
    return [np.array(s, F32).reshape(-1, 3) for s in S], [np.array(v, np.uint8) for v in V]


def view_case(view, H, W, n_random, seed):
    """the edge cases + n_random seeded segments in strands of 1..6 points, and the occluder of this view"""
    rng = np.random.default_rng(seed + 100 * view)
    S, V = edge_strands(H, W)
    left = n_random
    while left > 0:
        k = int(min(left, rng.integers(1, 6)))
        start = rng.uniform([-4, -4, 60], [H + 4, W + 4, 140])
        steps = rng.normal(0, [3.0, 3.0, 0.2], (k, 3))
        if rng.random() < 0.2:
            steps[:, :2] = np.rint(steps[:, :2])        # integer steps from a grid point: ties and exact lengths
            start[:2] = np.rint(start[:2] * 2) / 2
        pts = np.concatenate([start[None], start[None] + np.cumsum(steps, 0)])
        S.append(pts.astype(F32))
        V.append((rng.random(k + 1) > 0.03).astype(np.uint8))
        left -= k
    depth0 = None
    if view % 3 == 1:
        depth0 = np.full((H, W), 100, F32)              # equal depth stays: several cases sit at exactly 100
    elif view % 3 == 2:
        depth0 = rng.uniform(80, 130, (H, W)).astype(F32)
        depth0[rng.random((H, W)) < 0.3] = 255
    return S, V, depth0


def check_view(view, H, W, n_random, radius, seed=0, tol=0.25):
    S, V, depth0 = view_case(view, H, W, n_random, seed)
    vert, valid, counts = np.concatenate(S), np.concatenate(V), [len(s) for s in S]
    ref = hc.capture(vert, valid, counts, H, W, radius=radius, tol=tol, depth0=depth0)
    got = device_capture(vert, valid, counts, H, W, radius, tol, depth0)
    assert_same(got, ref, "view %d radius %d" % (view, radius))
    return got, (vert, valid, counts, depth0)


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_edge_cases_equal_the_restatement(radius):
    H, W = 32, 64
    for view in range(3):
        got, (vert, valid, counts, depth0) = check_view(view, H, W, 240, radius)
        assert sum(max(c - 1, 0) for c in counts) <= 300
        assert got["dropped"] == 1 and got["mask_u8"].any() and (got["cnt"] > 2 * radius + 1).any()
        # run to run: the integer atomics leave the same bytes
        again = device_capture(vert, valid, counts, H, W, radius, 0.25, depth0)
        assert_same(again, got, "second run")


def test_seeded_sweep_and_odd_image_sizes():
    for view in range(5):
        got, _ = check_view(view, 48, 80, 2000, 1, seed=11)
        assert got["mask_u8"].mean() > 0.5
    for (H, W), radius in (((17, 37), 2), ((1, 1), 1), ((5, 130), 0)):
        check_view(2, H, W, 150, radius, seed=3)
    # another layer bound and a sample count that is not the footprint's
    S, V, depth0 = view_case(1, 32, 64, 200, 5)
    vert, valid, counts = np.concatenate(S), np.concatenate(V), [len(s) for s in S]
    for tol, n_full in ((0.0, 1), (3.5, 7)):
        ref = hc.capture(vert, valid, counts, 32, 64, radius=1, tol=tol, depth0=depth0, n_full=n_full)
        assert_same(device_capture(vert, valid, counts, 32, 64, 1, tol, depth0, n_full), ref, "tol %g" % tol)


def test_empty_and_degenerate_strand_sets():
    H, W = 32, 64
    d0 = np.full((H, W), 77, F32)
    for counts in ([], [0, 0], [1], [1, 0, 1]):
        n = int(sum(counts))
        vert = np.tile(np.array([[5, 5, 60]], F32), (n, 1))
        got = device_capture(vert, np.ones(n, np.uint8), counts, H, W, 1, depth0=d0)
        assert_same(got, hc.capture(vert, np.ones(n, np.uint8), counts, H, W, depth0=d0), str(counts))
        assert not got["mask_u8"].any() and (got["depth"] == 77).all() and got["dropped"] == 0


@pytest.fixture(scope="module")
def world():
    """a small world-space strand set in front of three cameras, with the points a projection must refuse"""
    from monohair_amd import synth, synth_hair as sh
    from monohair_amd.camera import cameras_from_list

    H, W = 32, 64
    cams = cameras_from_list(synth.make_cameras(3, H, W))
    counts, pts = sh.make_hairstyle(40, 8, seed=4)
    pts = pts.copy()
    eye = np.linalg.inv(np.array(list(cams.values())[0].pose.numpy(), np.float64))[:3, 3]
    pts[9] = (2.0 * eye).astype(F32)                 # behind the first camera
    pts[17] = (0.95 * eye).astype(F32)               # in front of it, inside the near plane
    pts[25] = (np.nan, 0.0, 0.0)
    pts[33] = (np.inf, 0.0, 0.0)
    pts[41] = (0.0, -np.inf, 0.0)
    pts[49] = (3.0e38, 3.0e38, -3.0e38)
    pts[57] = (1.0e5, 0.0, 0.05)                     # far off to the side: a finite pixel beyond 2^20 in some view
    return H, W, cams, counts, pts


@pytest.mark.parametrize("radius", [0, 1, 2])
def test_world_points_through_the_whole_path(world, radius):
    from monohair_amd import synth, synth_hair as sh
    from monohair_amd.pmvo_utils import read_obj

    H, W, cams, counts, pts = world
    bust = None
    if radius == 1:
        import tempfile

        with tempfile.TemporaryDirectory() as d:
            synth.sphere_obj(os.path.join(d, "b.obj"), sh.BUST_R, 12, 24)
            bust = read_obj(os.path.join(d, "b.obj"))
    depth, ori, conf, mask, details = sh.capture_planes((counts, pts), cams, H, W, radius=radius, bust=bust, device=DEV,
                                                        return_details=True)
    fused = sh.capture_planes((counts, pts), cams, H, W, radius=radius, bust=bust, device=DEV)
    planes = [t.cpu().numpy() for t in (depth, ori, conf, mask)]
    for a, b in zip(planes, fused):
        assert a.tobytes() == b.cpu().numpy().tobytes()          # the one-call form is the four steps
    assert planes[3].any()
    for v, det in enumerate(details):
        vert, valid = det["vert"].cpu().numpy(), det["valid"].cpu().numpy()
        assert not valid[[25, 33, 41, 49]].any() and (v > 0 or not valid[[9, 17]].any())
        d0 = None if det["depth0"] is None else det["depth0"].cpu().numpy()
        ref = hc.capture(vert, valid, counts, H, W, radius=radius, depth0=d0)
        got = dict(depth=planes[0][v], ori_u8=planes[1][v], conf_u8=planes[2][v], mask_u8=planes[3][v], dropped=det["dropped"],
                   **{k: det[k].cpu().numpy() for k in ("zmin", "cnt", "c2", "s2")})
        assert_same(got, ref, "world view %d" % v)


def test_projection_is_pmvos_own(world):
    """vert / valid against mh_project_points on the same points: the rounded pixel of every in-bounds vertex, z_half * 255,
    and the validity rule restated on the projected values"""
    import torch

    from monohair_amd import synth_hair as sh
    from monohair_amd.pmvo import PMVO

    H, W, cams, counts, pts = world
    depth, ori, conf, mask, details = sh.capture_planes((counts, pts), cams, H, W, device=DEV, return_details=True)
    pm = PMVO.from_u8(cams, depth, ori, conf, mask, device=DEV, image_size=[H, W])
    seen = 0
    for v, det in enumerate(details):
        vert, valid = det["vert"].cpu().numpy(), det["valid"].cpu().numpy()
        rc, zp, oob = pm.project_points(pts, v)
        rc, zp, oob = rc.cpu().numpy(), zp.cpu().numpy(), oob.cpu().numpy()
        with np.errstate(over="ignore"):
            z255 = (zp * F32(255.0)).astype(F32)
        assert z255.tobytes() == vert[:, 2].tobytes()
        inb = ~oob
        assert np.array_equal(np.rint(vert[inb, :2]).astype(np.int64), rc[inb])
        with np.errstate(invalid="ignore"):
            z = -(zp * F32(2.0))                                   # exact: the halving was
            rule = (z < F32(-0.1)) & (np.abs(vert[:, 0]) < 2.0 ** 20) & (np.abs(vert[:, 1]) < 2.0 ** 20)
        assert np.array_equal(rule, valid != 0)
        seen += int((inb & (valid != 0)).sum())
    assert seen > 300
    del pm
    torch.cuda.synchronize()


def test_planes_equal_the_files_of_a_written_case(tmp_path):
    """PMVO.from_u8 on capture_planes' tensors and a PMVO built by the loaders from the files write_case wrote give the same
    forward() rows on 64 strand points"""
    from monohair_amd import synth_hair as sh
    from monohair_amd.camera import load_cam, parsing_camera
    from monohair_amd.pmvo import PMVO
    from monohair_amd.pmvo_utils import load_depth_plane, load_maps_u8, load_strand, read_obj

    V, H, W = 20, 64, 40
    strands = sh.make_hairstyle(150, 24, seed=9)
    base = sh.write_case(str(tmp_path), "synthetic_hair", V=V, H=H, W=W, strands=strands, device=DEV)
    segs, gt = load_strand(os.path.join(base, "gt_strands.hair"))
    assert segs == [24] * 150 and np.array_equal(gt.astype(F32), strands[1])
    assert np.load(os.path.join(base, "render_depth", "view_000.npy")).shape == (H, W, 3)
    cams = parsing_camera(load_cam(os.path.join(base, "ours", "cam_params.json")), os.path.join(base, "capture_images"))
    assert len(cams) == V
    o8, c8, m8 = load_maps_u8(cams, os.path.join(base, "best_ori"), os.path.join(base, "conf"),
                              os.path.join(base, "hair_mask"))
    kw = dict(device=DEV, image_size=[H, W], patch_size=5, conf_threshold=0.15)
    from_files = PMVO.from_u8(cams, load_depth_plane(cams, os.path.join(base, "render_depth")), o8, c8, m8, **kw)
    planes = sh.capture_planes(strands, cams, H, W, bust=read_obj(os.path.join(base, "ours", "bust_long_tsfm.obj")),
                               device=DEV)
    assert planes[3].any() and planes[2].max() > 100
    from_planes = PMVO.from_u8(cams, *planes, **kw)
    pts = strands[1][np.random.default_rng(1).choice(len(strands[1]), 64, replace=False)].astype(np.float64)
    a = [t.cpu().numpy() for t in from_files.forward(pts)[1:]]
    b = [t.cpu().numpy() for t in from_planes.forward(pts)[1:]]
    for x, y in zip(a, b):
        assert np.array_equal(x, y, equal_nan=True)
    assert np.isfinite(a[1]).any()
