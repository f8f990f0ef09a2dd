"""CPU: the photograph rule (include/mh_pmvo.h, "Hair photograph") as tests/hair_photo_np.py restates it, against cases
worked out by hand, and the two host functions of monohair_amd.synth_hair that feed it (strand_albedo, light_directions)."""
import numpy as np
import pytest

import hair_photo_np as hp

H, W = 16, 16
F32 = np.float32
BG, BUST = 32, 64


def strand(*pts):
    """one strand of (row, col, z255) vertices, all valid"""
    return np.array(pts, F32).reshape(-1, 3)


def run(strands, shades, S=4, w=0, depth0=None, valid=None, h=H, wd=W):
    """shades: one q per strand, given to every segment of it"""
    vert = np.concatenate(strands)
    valid = np.ones(len(vert), np.uint8) if valid is None else np.asarray(valid, np.uint8)
    shade = np.concatenate([np.full(len(s), q, np.uint8) for s, q in zip(strands, shades)])
    return hp.photo(vert, valid, [len(s) for s in strands], shade, h, wd, S=S, w=w, depth0=depth0, bust_code=BUST,
                    background_code=BG)


def key_of(z, q):
    return (np.uint64(np.array(z, F32).view(np.uint32)) << np.uint64(32)) | np.uint64(q)


def test_horizontal_strand_through_pixel_centres_covers_one_sub_pixel_row():
    # row' = 4*5 + 1.5 = 21.5 -> 22 (half to even), col' from 10.5 to 42.5: 32 samples on the sub-pixel columns 11 .. 42
    q = 200
    out = run([strand((5, 2.25, 100), (5, 10.25, 100))], [q])
    hit = out["keys"] != hp.EMPTY
    assert sorted(zip(*np.nonzero(hit))) == [(22, c) for c in range(11, 43)]
    assert (out["keys"][hit] == key_of(100, q)).all()
    assert (out["cover"][5, 3:10] == 4).all() and out["cover"][5, 2] == 1 and out["cover"][5, 10] == 3
    assert out["cover"].sum() == 32 and out["dropped"] == 0
    assert (2 * (4 * q + 12 * BG) + 16) // 32 == 74
    assert (out["gray"][5, 3:10] == 74).all()
    assert out["gray"][5, 2] == (2 * (q + 15 * BG) + 16) // 32 and out["gray"][5, 10] == (2 * (3 * q + 13 * BG) + 16) // 32
    assert out["gray"][4, 5] == BG and out["gray"][0, 0] == BG
    # with w = 1 the strand is three sub-pixel rows wide: 21 .. 23, all of pixel 5
    wide = run([strand((5, 2.25, 100), (5, 10.25, 100))], [q], w=1)
    assert (wide["cover"][5, 3:10] == 12).all() and (wide["gray"][5, 3:10] == (2 * (12 * q + 4 * BG) + 16) // 32).all()
    assert wide["cover"][4].sum() == 0 and wide["cover"][6].sum() == 0


def test_the_same_strand_without_supersampling():
    q = 200
    out = run([strand((5, 2.25, 100), (5, 10.25, 100))], [q], S=1)
    assert sorted(zip(*np.nonzero(out["cover"]))) == [(5, c) for c in range(3, 11)]
    assert (out["gray"][5, 3:11] == q).all() and (out["cover"][5, 3:11] == 1).all()
    assert (np.delete(out["gray"].reshape(-1), 5 * W + np.arange(3, 11)) == BG).all()


def test_crossing_strands_the_nearer_wins_and_at_equal_depth_the_darker():
    hor = strand((6, 2.125, 100), (6, 10.125, 100))
    ver_far, ver_near, ver_same = (strand((2.125, 6, z), (10.125, 6, z)) for z in (101, 99, 100))
    # S = 2, w = 0: the horizontal strand is sub-pixel row 2*6 + 0.5 = 12.5 -> 12, columns 5 .. 20 (samples on 5.25 ..
    # 20.25: no ties); the vertical one sub-pixel column 12, rows 5 .. 20
    for other, q_other, want in ((ver_far, 50, 200), (ver_near, 250, 250), (ver_same, 50, 50), (ver_same, 250, 200)):
        out = run([hor, other], [200, q_other], S=2)
        z = min(F32(100), other[0, 2])
        assert out["keys"][12, 12] == key_of(z, want)
        assert out["keys"][12, 11] == key_of(100, 200) and out["keys"][11, 12] == key_of(other[0, 2], q_other)
    # the order of the strands does not matter
    a = run([hor, ver_same], [200, 50], S=2)
    b = run([ver_same, hor], [50, 200], S=2)
    assert a["keys"].tobytes() == b["keys"].tobytes() and a["gray"].tobytes() == b["gray"].tobytes()


def test_occluder_keeps_equal_depth_and_discards_one_ulp_behind():
    d0 = np.full((H, W), 100, F32)
    at = run([strand((5, 5, 100), (5, 5, 100))], [180], depth0=d0)
    assert at["cover"][5, 5] == 1 and at["cover"].sum() == 1
    assert at["gray"][5, 5] == (2 * (180 + 15 * BUST) + 16) // 32
    behind = np.nextafter(F32(100), F32(np.inf))
    out = run([strand((5, 5, behind), (5, 5, behind))], [180], depth0=d0)
    assert (out["cover"] == 0).all() and (out["keys"] == hp.EMPTY).all() and (out["gray"] == BUST).all()


def test_bust_pixels_get_the_bust_code_and_the_rest_the_background_code():
    d0 = np.full((H, W), 255, F32)
    d0[4:9, 4:9] = 120
    out = run([strand((1, 1, 100), (1, 1, 100))], [255], S=2, depth0=d0)
    want = np.full((H, W), BG)
    want[4:9, 4:9] = BUST
    want[1, 1] = (2 * (255 + 3 * BG) + 4) // 8
    assert np.array_equal(out["gray"], want)
    # a strand behind the bust is hidden there and shows beyond it (the occluder is looked up at the owning pixel)
    out = run([strand((6, 1.125, 130), (6, 12.125, 130))], [255], S=2, depth0=d0)
    assert (out["cover"][6, 4:9] == 0).all() and (out["gray"][6, 4:9] == BUST).all()
    assert (out["cover"][6, 2:4] == 2).all() and (out["cover"][6, 9:12] == 2).all()
    no_plane = run([strand((6, 1.125, 130), (6, 12.125, 130))], [255], S=2)
    assert (no_plane["cover"][6, 2:12] == 2).all()


def test_shade_along_across_and_of_a_zero_length_segment():
    pts = np.array([[0, 0, 0], [0, 0, 0.5],                 # T parallel to L
                    [0, 0, 0], [0.25, 0, 0],                # T across L
                    [1, 1, 1], [1, 1, 1],                   # zero length
                    [0, 0, 0], [0.5, 0, 0.5]], F32)         # 45 degrees: sin = sqrt(1/2)
    L = np.array([0.0, 0.0, 1.0])
    albedo = np.array([0.75, 0.75, 0.75, 1.0], F32)
    shade = hp.segment_shades(pts, np.ones(8, np.uint8), [2, 2, 2, 2], albedo, L, 0.25)
    assert shade[0] == round(255 * 0.75 * 0.25) == 48        # rint(47.8125)
    assert shade[2] == 191                                   # rint(191.25)
    assert shade[4] == 48
    assert shade[6] == int(np.rint(255 * (0.25 + 0.75 * np.sqrt(0.5))))
    assert (shade[1::2] == 0).all()                          # no segment starts at a strand's last point
    # an invalid end: no segment, shade 0; a shade above 255 is clamped
    assert hp.segment_shades(pts[:2], [1, 0], [2], albedo[:1], L, 0.25)[0] == 0
    assert hp.segment_shades(pts[2:4], [1, 1], [2], np.array([1.5], F32), L, 0.25)[0] == 255
    # half to even: 255 * 0.5 * 1 = 127.5 -> 128, 255 * 0.5 * (0.5 + 0.5 * 0) ... = 63.75 -> 64
    assert hp.segment_shades(pts[2:4], [1, 1], [2], np.array([0.5], F32), L, 0.0)[0] == 128


def test_a_centre_on_a_half_lands_where_pmvo_rounds_it_to():
    """PMVO rounds half to even.  Without supersampling the sample centre is rounded by the same rint; with it, row' =
    S*(k + 1/2) + (S-1)/2 is the tie between the last sub-pixel of pixel k and the first of k + 1 and goes to the even one,
    the first of pixel k + 1: PMVO's pixel for odd k (the header says so for even k)."""
    for k in (5, 6, 7, 8):
        out = run([strand((k + 0.5, 3, 100), (k + 0.5, 3, 100))], [255], S=1)
        r, c = (int(x[0]) for x in np.nonzero(out["cover"]))
        assert (r, c) == (int(np.rint(F32(k + 0.5))), 3)
    for S in (2, 4, 8):
        for k in (5, 7):
            out = run([strand((k + 0.5, k + 0.5, 100), (k + 0.5, k + 0.5, 100))], [255], S=S)
            assert out["cover"].sum() == 1 and out["cover"][k + 1, k + 1] == 1
            assert int(np.rint(F32(k + 0.5))) == k + 1
            assert out["keys"][S * (k + 1), S * (k + 1)] != hp.EMPTY
        out = run([strand((6.5, 3, 100), (6.5, 3, 100))], [255], S=S)
        assert out["cover"][7, 3] == 1                        # (PMVO: 6)
    # just inside pixel k: its last sub-pixel
    below = np.nextafter(F32(7.5), F32(0))
    out = run([strand((below, 3, 100), (below, 3, 100))], [255], S=4)
    assert out["cover"][7, 3] == 1 and out["keys"][31, 14] != hp.EMPTY


def test_segments_of_8192_samples_stay_and_of_8193_are_dropped_and_counted():
    wide = 4192
    a = run([strand((5, -4000.25, 100), (5, 4192.25, 100)), strand((5, -4000.25, 100), (5, 4191.75, 100))], [9, 9], S=1,
            wd=wide)
    assert a["dropped"] == 1 and (a["cover"][5, :wide] == 1).all() and a["cover"].sum() == wide
    # in sub-pixel units: 2048 pixels at S = 4 are 8192 samples
    b = run([strand((5, -1000, 100), (5, 1048, 100))], [9], S=4, wd=1100)
    assert b["dropped"] == 0 and (b["cover"][5, :1048] == 4).all() and b["cover"].sum() == 4 * 1048 + 2
    c = run([strand((5, -1000, 100), (5, 1048.25, 100))], [9], S=4, wd=1100)
    assert c["dropped"] == 1 and c["cover"].sum() == 0 and (c["gray"] == BG).all()
    d = run([strand((5, -1000, 100), (5, 1048.25, 100))] * 3, [9] * 3, S=4, wd=1100)
    assert d["dropped"] == 3


def test_invalid_ends_and_one_point_strands_make_nothing():
    s = strand((5, 2.25, 100), (5, 10.25, 100), (9, 10.25, 100))
    out = run([s], [200], valid=[1, 0, 1])
    assert out["cover"].sum() == 0 and (out["gray"] == BG).all() and out["dropped"] == 0
    assert run([strand((5, 5, 100))], [200])["cover"].sum() == 0


def test_strand_albedo_repeats_for_a_seed():
    from monohair_amd import synth_hair as sh

    a, b = sh.strand_albedo(500, 7, 0.3, 0.9), sh.strand_albedo(500, 7, 0.3, 0.9)
    assert a.dtype == np.float32 and a.shape == (500,) and a.tobytes() == b.tobytes()
    assert a.min() >= F32(0.3) and a.max() <= F32(0.9) and a.std() > 0.1
    assert not np.array_equal(a, sh.strand_albedo(500, 8, 0.3, 0.9))
    assert sh.strand_albedo(0, 7).shape == (0,)
    d = sh.strand_albedo(500, 7)
    assert d.min() >= F32(sh.PHOTO_ALBEDO[0]) and d.max() <= F32(sh.PHOTO_ALBEDO[1])
    with pytest.raises(ValueError):
        sh.strand_albedo(5, 0, 0.9, 0.3)


def test_light_directions_are_unit_and_point_at_the_camera():
    from monohair_amd import synth, synth_hair as sh
    from monohair_amd.camera import camera_records, cameras_from_list

    cam_list = synth.make_cameras(12, 48, 32, rings=2)
    cams = cameras_from_list(cam_list)
    L = sh.light_directions(cams)
    assert L.dtype == np.float64 and L.shape == (12, 3)
    assert np.abs(np.sqrt((L * L).sum(1)) - 1.0).max() <= 2e-16
    # a plain float64 computation from the pose
    for v, cam in enumerate(cams.values()):
        row = cam.pose.numpy()[2, :3].astype(np.float64)
        assert np.array_equal(L[v], row / np.sqrt((row * row).sum()))
    assert np.array_equal(L, sh.light_directions(camera_records(cams)))
    # ... which is the camera's own +z axis in the world (it looks down -z), from the scene towards the eye
    for v, c in enumerate(cam_list):
        c2w = np.array(c["pose"], np.float64)
        axis = c2w[:3, 2] / np.linalg.norm(c2w[:3, 2])
        assert np.abs(L[v] - axis).max() < 1e-6
        assert float(L[v] @ c2w[:3, 3]) > 0                   # the cameras surround the origin
