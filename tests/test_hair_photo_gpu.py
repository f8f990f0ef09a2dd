"""GPU: the photograph renderer (the photo kernels of csrc/haircapture.hip, monohair_amd.synth_hair.photo_planes) against the
numpy restatement of its rule (tests/hair_photo_np.py): every quantity EQUAL, not close -- the segment shades, the whole key
plane, cover, gray and the dropped count.  The segment cases are built on the sub-pixel grid and handed to the per-step entry
points as vertices, so that each one sits exactly where it is meant to (a centre on k + 0.5, a length one ulp past 8192
samples); world points go through photo_planes."""
import ctypes
import os

import numpy as np
import pytest

import hair_photo_np as hp

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = np.float32
BUST, BG = 70, 25


def _dev(a, t):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=t)).to(DEV)


def _offsets(counts):
    counts = np.asarray(counts, np.int64).reshape(-1)
    offs = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    return offs


def device_photo(vert, valid, counts, shade, H, W, S, w, depth0=None):
    """mh_photo_front and mh_photo_resolve on given vertices and shades -> the dict hair_photo_np.photo returns"""
    import torch

    from monohair_amd import _lib
    from monohair_amd.pmvo_utils import _ctx_for

    L, ctx, st = _lib.lib(), _ctx_for(DEV), _lib.stream_ptr()
    offs = _offsets(counts)
    n, ns = int(offs[-1]), len(offs) - 1
    pad = lambda a, t, k: _dev(np.concatenate([np.reshape(a, (-1, k)), np.zeros((1, k))]), t)          # noqa: E731
    vert_d, valid_d, shade_d = pad(vert, F32, 3), pad(valid, np.uint8, 1), pad(shade, np.uint8, 1)
    offs_d = _dev(offs, np.int64)
    d0 = None if depth0 is None else _dev(depth0, F32)
    keys = torch.full((S * H, S * W), 5, dtype=torch.int64, device=DEV)
    dropped = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    gray = torch.empty((H, W), dtype=torch.uint8, device=DEV)
    cover = torch.empty((H, W), dtype=torch.int32, device=DEV)
    p = _lib.ptr
    _lib.check(L.mh_photo_front(ctx, p(vert_d), p(valid_d), p(offs_d), ns, n, p(shade_d), H, W, S, w, p(d0), p(keys),
                                p(dropped), st))
    _lib.check(L.mh_photo_resolve(ctx, p(keys), p(d0), H, W, S, BUST, BG, p(gray), p(cover), st))
    torch.cuda.synchronize()
    return dict(keys=keys.cpu().numpy().view(np.uint64), gray=gray.cpu().numpy(), cover=cover.cpu().numpy(),
                dropped=int(dropped.item()))


def device_shade(points, valid, counts, albedo, light, ambient):
    import torch

    from monohair_amd import _lib
    from monohair_amd.pmvo_utils import _ctx_for

    L, ctx, st = _lib.lib(), _ctx_for(DEV), _lib.stream_ptr()
    offs = _offsets(counts)
    n, ns = int(offs[-1]), len(offs) - 1
    shade = torch.full((max(n, 1),), 77, dtype=torch.uint8, device=DEV)
    pts_d, valid_d, offs_d, alb_d = _dev(points, F32), _dev(valid, np.uint8), _dev(offs, np.int64), _dev(albedo, F32)
    light = np.ascontiguousarray(light, np.float64)
    p = _lib.ptr
    _lib.check(L.mh_photo_shade(ctx, p(pts_d), p(valid_d), p(offs_d), ns, n, p(alb_d), light.ctypes.data_as(ctypes.c_void_p),
                                float(ambient), p(shade), st))
    torch.cuda.synchronize()
    return shade.cpu().numpy()[:n]


def assert_same(got, ref, what):
    assert got["dropped"] == ref["dropped"], (what, got["dropped"], ref["dropped"])
    for k in ("keys", "cover", "gray"):
        assert got[k].dtype == ref[k].dtype and got[k].shape == ref[k].shape, (what, k)
        assert got[k].tobytes() == ref[k].tobytes(), "%s: %s differs at %d places" % (what, k, int((got[k] != ref[k]).sum()))


def edge_strands(H, W, S):
    """-> (list of [n,3] float32 (row, col, z255) strands, list of valid flags).  One strand per case of the rule, written on
    the sub-pixel grid (row', col') and carried to pixels by the inverse of row' = S row + (S-1)/2, which is exact for the
    dyadic positions below."""
    HS, WS = S * H, S * W
    px = lambda x: (np.float64(x) - (S - 1) / 2.0) / S          # noqa: E731
    sub = [
        [(-3.3, 10.2, 90), (4.1, 12.7, 91)],                              # across the top border
        [(HS - 3.4, 20.1, 92), (HS + 3.2, 22.4, 93)],                     # ... the bottom
        [(10.3, -4.2, 94), (12.1, 3.6, 95)],                              # ... the left
        [(15.5, WS - 3.7, 96), (17.2, WS + 3.8, 97)],                     # ... the right
        [(-10, -10, 90), (-5, -3, 90)], [(HS + 8, WS + 6, 90), (HS + 13, WS + 16, 90)],     # wholly outside
        [(-2, 5, 90), (-2, 40, 90)],                                      # outside along a border, the footprint reaches in
        [(5.25, 10.25, 100), (5.25, 14.25, 100)],                         # n exactly at an integer length: 4 samples
        [(8, 20, 100), (8, 24, 100.5)], [(10, 30, 100), (13, 30, 99)],    # centres exactly on k + 0.5 (half to even)
        [(20.5, 40.5, 100), (20.5, 40.5, 100)], [(21.5, 41.5, 100.125), (22.5, 42.5, 100.125)],
        [(0, 0, 80), (0, 0, 80)], [(HS - 1, WS - 1, 80), (HS - 1, WS - 1, 80)],       # footprints clipped at the corners
        [(0, WS - 1, 80), (0.4, WS - 0.6, 80)], [(HS - 1, 0, 80), (HS - 0.6, 0.3, 80)],
        [(5, -5000, 100), (5, 5000, 100)],                                # n > 8192: dropped and counted
        [(6, -4000.25, 100), (6, 4191.75, 100)],                          # n = 8192: drawn
        [(3, 3, 50)],                                                     # a strand of one point
        [],                                                               # an empty strand
        [(12, 5, 100), (14, 9, 100), (16.5, 9.5, 100), (16.5, 15, 100.25), (12, 15, 100.5), (12.25, 5.125, 100.125)],
        [(25.2, 5.3, 70), (25.9, 50.2, 120)],                             # a depth ramp under ...
        [(20.1, 30.2, 95.1), (30.3, 30.9, 95.2)],                         # ... a crossing strand
        [(9, 12, 100), (9, 28, 100)], [(2, 16, 100), (18, 16, 100)],      # a crossing at exactly equal depth
        [(2, 50, 100), (2.2, 50.1, 100), (2.3, 50.3, 100.3)],             # sub-pixel segments on one sub-pixel
    ]
    out = [np.array([(px(r), px(c), z) for r, c, z in s], F32).reshape(-1, 3) for s in sub]
    V = [[1] * len(s) for s in out]
    # n = 8193 by one float32 ulp of the pixel position
    s = np.array([(px(7), px(-4000.25), 100), (px(7), px(4191.75), 100)], F32)
    s[1, 1] = np.nextafter(s[1, 1], F32(np.inf))
    out.append(s)
    V.append([1, 1])
    # one end invalid: both its segments go
    out.append(np.array([(px(10), px(45), 100), (px(11), px(50), 100), (px(12), px(55), 100), (px(13), px(58), 100)], F32))
    V.append([1, 0, 1, 1])
    out.append(np.array([(np.nan, 45, 100), (18, 50, np.inf), (px(19), px(55), 100), (px(19), px(58), 100)], F32))
    V.append([0, 0, 1, 1])
    return out, [np.array(v, np.uint8) for v in V]


def view_case(view, H, W, S, n_random, seed):
    """the edge cases + n_random seeded segments in strands of 1..6 points, a shade per segment, the occluder of this view"""
    rng = np.random.default_rng(seed + 100 * view)
    strands, V = edge_strands(H, W, S)
    left = n_random
    while left > 0:
        k = int(min(left, rng.integers(1, 6)))
        start = rng.uniform([-4, -4, 60], [H + 4, W + 4, 140])
        steps = rng.normal(0, [3.0, 3.0, 0.2], (k, 3))
        if rng.random() < 0.2:
            steps[:, :2] = np.rint(steps[:, :2] * S) / S        # whole sub-pixel steps from a half sub-pixel: ties
            start[:2] = np.rint(start[:2] * 2 * S) / (2 * S)
            steps[:, 2] = 0
            start[2] = 100
        pts = np.concatenate([start[None], start[None] + np.cumsum(steps, 0)])
        strands.append(pts.astype(F32))
        V.append((rng.random(k + 1) > 0.03).astype(np.uint8))
        left -= k
    vert, valid, counts = np.concatenate(strands), np.concatenate(V), [len(s) for s in strands]
    shade = rng.integers(0, 256, len(vert)).astype(np.uint8)
    depth0 = None
    if view % 3 == 1:
        depth0 = np.full((H, W), 100, F32)              # equal depth stays: several cases sit at exactly 100
        depth0[:, W // 2:] = 255
    elif view % 3 == 2:
        depth0 = rng.uniform(80, 130, (H, W)).astype(F32)
        depth0[rng.random((H, W)) < 0.3] = 255
    return vert, valid, counts, shade, depth0


def check_view(view, H, W, S, w, n_random, seed=0):
    vert, valid, counts, shade, depth0 = view_case(view, H, W, S, n_random, seed)
    ref = hp.photo(vert, valid, counts, shade, H, W, S, w, depth0, BUST, BG)
    got = device_photo(vert, valid, counts, shade, H, W, S, w, depth0)
    assert_same(got, ref, "view %d S %d w %d" % (view, S, w))
    return got, (vert, valid, counts, shade, depth0)


@pytest.mark.parametrize("w", [0, 1, 2])
@pytest.mark.parametrize("S", [1, 2, 4])
def test_edge_cases_equal_the_restatement(S, w):
    H, W = 32, 64
    for view in range(3):
        got, (vert, valid, counts, shade, depth0) = check_view(view, H, W, S, w, 230)
        assert sum(max(c - 1, 0) for c in counts) <= 300
        assert got["dropped"] == 2 and got["cover"].any() and got["cover"].max() <= S * S
        assert len(np.unique(got["gray"])) > 8
        if depth0 is not None:
            bare = got["cover"] == 0
            assert (got["gray"][bare & (depth0 < 255)] == BUST).all() and (got["gray"][bare & ~(depth0 < 255)] == BG).all()
        # run to run: the integer minimum leaves the same bytes
        assert_same(device_photo(vert, valid, counts, shade, H, W, S, w, depth0), got, "second run")


def test_seeded_sweep():
    for view in range(5):
        got, _ = check_view(view, 48, 80, (4, 2)[view % 2], (1, 2)[view % 2], 2000, seed=11)
        assert (got["cover"] > 0).mean() > 0.25


def test_odd_image_sizes_and_eightfold_supersampling():
    for (H, W), S, w in (((17, 37), 4, 2), ((1, 1), 4, 1), ((1, 1), 1, 0), ((5, 130), 2, 0), ((8, 8), 8, 1), ((8, 8), 8, 3)):
        check_view(2, H, W, S, w, 150, seed=3)
        check_view(0, H, W, S, w, 150, seed=4)


def test_empty_and_degenerate_strand_sets():
    H, W = 32, 64
    d0 = np.full((H, W), 255, F32)
    d0[:, :10] = 77
    for counts in ([], [0, 0], [1], [1, 0, 1]):
        n = int(sum(counts))
        vert = np.tile(np.array([[5, 5, 60]], F32), (n, 1))
        ones = np.ones(n, np.uint8)
        got = device_photo(vert, ones, counts, np.full(n, 200, np.uint8), H, W, 2, 1, d0)
        assert_same(got, hp.photo(vert, ones, counts, np.full(n, 200, np.uint8), H, W, 2, 1, d0, BUST, BG), str(counts))
        assert not got["cover"].any() and (got["keys"] == hp.EMPTY).all() and got["dropped"] == 0
        assert (got["gray"][:, :10] == BUST).all() and (got["gray"][:, 10:] == BG).all()
        shade = device_shade(np.zeros((n, 3), F32), ones, counts, np.ones(max(len(counts), 1), F32), [0, 0, 1], 0.3)
        assert shade.shape == (n,) and not shade.any()


def test_segment_shades_equal_the_restatement():
    rng = np.random.default_rng(5)
    counts = rng.integers(0, 7, 900)
    n = int(counts.sum())
    pts = rng.normal(0, 0.1, (n, 3)).astype(F32)
    pts[rng.random(n) < 0.05] = pts[0]                               # repeated points
    same = np.nonzero(rng.random(n - 1) < 0.05)[0]
    pts[same + 1] = pts[same]                                        # zero-length segments
    L = np.array([0.36, -0.48, 0.8])
    along = np.nonzero(rng.random(n - 1) < 0.05)[0]
    pts[along + 1] = pts[along] + (L * 0.125).astype(F32)            # (nearly) along the light
    axis = np.nonzero(rng.random(n - 1) < 0.05)[0]
    pts[axis + 1] = pts[axis] + np.array([0, 0.25, 0], F32)
    valid = (rng.random(n) > 0.05).astype(np.uint8)
    albedo = rng.uniform(0, 1.2, len(counts)).astype(F32)
    albedo[:3] = (0.0, 1.0, 0.5)
    for light, ambient in ((L, 0.3), (L, 0.0), (L, 1.0), ([0.0, 1.0, 0.0], 0.25), ([0.0, 0.0, 1.0], 0.5)):
        ref = hp.segment_shades(pts, valid, counts, albedo, light, ambient)
        got = device_shade(pts, valid, counts, albedo, light, ambient)
        assert got.dtype == ref.dtype and got.tobytes() == ref.tobytes(), int((got != ref).sum())
        assert len(np.unique(ref)) > 100 or ambient == 1.0


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
    synth_bust = None
    import tempfile

    from monohair_amd.pmvo_utils import read_obj

    with tempfile.TemporaryDirectory() as d:
        synth.sphere_obj(os.path.join(d, "b.obj"), sh.BUST_R, 12, 24)
        synth_bust = read_obj(os.path.join(d, "b.obj"))
    return H, W, cams, counts, pts, synth_bust


@pytest.mark.parametrize("S,w,with_bust", [(4, 1, True), (2, 0, False), (1, 2, True)])
def test_world_points_through_photo_planes(world, S, w, with_bust):
    from monohair_amd import synth_hair as sh

    H, W, cams, counts, pts, bust = world
    bust = bust if with_bust else None
    before = [t.cpu().numpy().tobytes() for t in sh.capture_planes((counts, pts), cams, H, W, bust=bust, device=DEV)]
    kw = dict(supersample=S, width=w, ambient=0.2, seed=3, bust=bust, bust_code=BUST, background_code=BG, device=DEV)
    gray, details = sh.photo_planes((counts, pts), cams, H, W, return_details=True, **kw)
    fused = sh.photo_planes((counts, pts), cams, H, W, **kw)
    assert gray.dtype == fused.dtype and gray.shape == fused.shape == (3, H, W)
    gray = gray.cpu().numpy()
    assert gray.tobytes() == fused.cpu().numpy().tobytes()             # the one-call form is the steps
    assert gray.tobytes() == sh.photo_planes((counts, pts), cams, H, W, **kw).cpu().numpy().tobytes()
    after = [t.cpu().numpy().tobytes() for t in sh.capture_planes((counts, pts), cams, H, W, bust=bust, device=DEV)]
    assert before == after                                             # and leaves the capture's planes alone
    albedo, light = sh.strand_albedo(len(counts), 3), sh.light_directions(cams)
    seen = 0
    for v, det in enumerate(details):
        vert, valid = det["vert"].cpu().numpy(), det["valid"].cpu().numpy()
        assert not valid[[25, 33, 41, 49]].any() and (v > 0 or not valid[[9, 17]].any())
        d0 = None if det["depth0"] is None else det["depth0"].cpu().numpy()
        assert (d0 is not None) == with_bust
        shade = hp.segment_shades(pts, valid, counts, albedo, light[v], 0.2)
        assert det["shade"].cpu().numpy().tobytes() == shade.tobytes()
        ref = hp.photo(vert, valid, counts, shade, H, W, S, w, d0, BUST, BG)
        got = dict(keys=det["keys"].cpu().numpy().view(np.uint64), gray=gray[v], cover=det["cover"].cpu().numpy(),
                   dropped=det["dropped"])
        assert_same(got, ref, "world view %d" % v)
        seen += int((got["cover"] > 0).sum())
    assert seen > 100


def test_bad_arguments_are_refused():
    from monohair_amd import _lib, synth, synth_hair as sh
    from monohair_amd.camera import cameras_from_list

    L = _lib.lib()
    assert L.mh_photo_scratch_bytes(10, 8, 8, 3) == 0 and L.mh_photo_scratch_bytes(10, 8, 8, 16) == 0
    assert L.mh_photo_scratch_bytes(10, 1 << 14, 1 << 14, 8) == 0          # 2^34 sub-pixels
    assert L.mh_photo_scratch_bytes(10, 8, 8, 4) >= 8 * 32 * 32
    cams = cameras_from_list(synth.make_cameras(2, 8, 8))
    strands = sh.make_hairstyle(3, 4, seed=1)
    with pytest.raises(ValueError):
        sh.photo_planes(strands, cams, 8, 8, supersample=3, device=DEV)
    with pytest.raises(ValueError):
        sh.photo_planes(strands, cams, 8, 8, albedo=np.ones(2, F32), device=DEV)
    with pytest.raises(_lib.MhError):
        sh.photo_planes(strands, cams, 8, 8, width=99, device=DEV)
    with pytest.raises(_lib.MhError):
        sh.photo_planes(strands, cams, 8, 8, ambient=1.5, device=DEV)
