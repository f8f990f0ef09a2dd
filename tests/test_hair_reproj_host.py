"""CPU: the numpy restatement of the capture-agreement rule (tests/hair_reproj_np.py) against cases worked out by hand, and
the host functions of monohair_amd.hairreproj (conf_min_code, prune_strands, the report) on hand-made counters.  The strands
are given in pixel space as (row, col, z255) vertices, so every sample sits exactly where the case needs it."""
import numpy as np
import pytest

import hair_reproj_np as hr

F32 = np.float32
H, W = 16, 24
up = lambda x: np.nextafter(F32(x), F32(np.inf))          # noqa: E731


def planes(ori=0, conf=255, mask=255):
    return (np.full((H, W), ori, np.uint8), np.full((H, W), conf, np.uint8), np.full((H, W), mask, np.uint8))


def run(strands, ori_conf_mask, bounds, conf_min=39, radius=0, tol=0.25, depth0=None, valid=None):
    vert = np.concatenate([np.array(s, F32).reshape(-1, 3) for s in strands]) if strands else np.zeros((0, 3), F32)
    counts = [len(s) for s in strands]
    valid = np.ones(len(vert), np.uint8) if valid is None else valid
    return hr.support(vert, valid, counts, H, W, *ori_conf_mask, conf_min, bounds, radius=radius, tol=tol, depth0=depth0)


HORIZONTAL = [(5, 2, 100), (5, 10, 100)]          # eight samples on row 5, centres on k + 0.5: columns 2 4 4 6 6 8 8 10


def test_a_horizontal_strand_agrees_with_code_0_and_not_with_code_90():
    bounds = hr.bounds_of([0, 10, 20, 30, 44.9])
    assert bounds[0] == 4096.0
    got = run([HORIZONTAL], planes(ori=0), bounds)
    assert got["strand"].tolist() == [[8, 8, 8, 0, 8, 8, 8, 8, 8]]      # qc = 4096, T[0] = (1, 0): 4096 >= every bound
    assert got["view"].tolist() == got["strand"][0].tolist()
    got = run([HORIZONTAL], planes(ori=90), bounds)
    assert got["strand"].tolist() == [[8, 8, 8, 0, 0, 0, 0, 0, 0]]           # -4096 + 0 * T[90][1]
    # the silhouette: pass A at radius 0 touches the five pixels the centres round to
    assert got["silhouette"].tolist() == [5, 0, H * W - 5]
    assert np.isfinite(got["zmin"]).sum() == 5 and np.isfinite(got["zmin"][5, [2, 4, 6, 8, 10]]).all()
    # at 90 degrees the bound is -4096 and equality counts
    assert run([HORIZONTAL], planes(ori=90), [-4096.0])["strand"][0, 4] == 8
    assert run([HORIZONTAL], planes(ori=90), [np.nextafter(-4096.0, 0.0)])["strand"][0, 4] == 0


def test_the_bound_is_included_and_the_next_float64_is_not():
    T = hr.hc.code_table().astype(np.float64)
    strand = [(9, 3, 100), (6, 7, 100)]                     # dr = -3, dc = 4: c2 = 0.28, s2 = 0.96
    seg, _ = hr.segments(np.array(strand, F32), [1, 1], [2])
    assert seg["qc"].tolist() == [1147] and seg["qs"].tolist() == [3932] and seg["n"].tolist() == [4]
    exact = 1147.0 * T[45, 0] + 3932.0 * T[45, 1]
    assert 3931.9 < exact <= 3932.0001
    got = run([strand], planes(ori=45), [exact, np.nextafter(exact, np.inf), np.nextafter(exact, -np.inf)])
    assert got["strand"].tolist() == [[4, 4, 4, 0, 4, 0, 4]]


def test_mask_confidence_and_orientation_codes_at_their_thresholds():
    b = hr.bounds_of([30])
    assert run([HORIZONTAL], planes(mask=51), b)["strand"].tolist() == [[8, 0, 0, 0, 0]]
    assert run([HORIZONTAL], planes(mask=52), b)["strand"].tolist() == [[8, 8, 8, 0, 8]]
    assert run([HORIZONTAL], planes(mask=51), b)["silhouette"].tolist() == [0, 5, 0]
    cmin = hr.conf_min_code(0.15)
    assert cmin == 39                                       # 38 / 255 = 0.14902, 39 / 255 = 0.15294
    assert run([HORIZONTAL], planes(conf=cmin), b, conf_min=cmin)["strand"].tolist() == [[8, 8, 8, 0, 8]]
    assert run([HORIZONTAL], planes(conf=cmin - 1), b, conf_min=cmin)["strand"].tolist() == [[8, 8, 0, 0, 0]]
    assert run([HORIZONTAL], planes(conf=255), b, conf_min=256)["strand"].tolist() == [[8, 8, 0, 0, 0]]
    low = hr.bounds_of([90])                                # every direction agrees with every code that is one
    assert run([HORIZONTAL], planes(ori=179), low)["strand"].tolist() == [[8, 8, 8, 0, 8]]
    assert run([HORIZONTAL], planes(ori=180), low)["strand"].tolist() == [[8, 8, 0, 0, 0]]
    assert run([HORIZONTAL], planes(ori=255), low)["strand"].tolist() == [[8, 8, 0, 0, 0]]


def test_a_zero_length_segment_is_counted_and_never_agrees():
    got = run([[(3, 3, 100), (3, 3, 100)]], planes(), [-4096.0, -1.0e9])
    assert got["strand"].tolist() == [[1, 1, 1, 0, 0, 0]]


def test_the_front_layer_and_the_occluder_at_equality_and_one_ulp_behind():
    dot = lambda z: [(7, 7, z), (7, 7, z)]                 # noqa: E731  (one sample on pixel (7, 7))
    b = hr.bounds_of([30])
    assert float(F32(100.0) + F32(0.25)) == 100.25
    got = run([dot(100), dot(100.25), dot(up(100.25))], planes(), b, tol=0.25)
    assert got["strand"][:, 0].tolist() == [1, 1, 0]
    got = run([dot(100), dot(100), dot(up(100))], planes(), b, tol=0.0)
    assert got["strand"][:, 0].tolist() == [1, 1, 0]
    d0 = np.full((H, W), 255, F32)
    d0[7, 7] = 100
    d0[8, 8] = 100
    got = run([dot(100), [(8, 8, up(100)), (8, 8, up(100))]], planes(), b, depth0=d0)
    assert got["strand"][:, 0].tolist() == [1, 0]
    assert got["silhouette"].tolist() == [1, 0, H * W - 1]      # the discarded fragment predicts nothing


def test_centres_outside_the_image_and_invalid_ends_belong_to_no_class():
    b = hr.bounds_of([30])
    got = run([[(-3, 5, 100), (-3, 9, 100)], [(5, W, 100), (5, W + 6, 100)], [(5, W - 2.6, 100), (5, W + 1.4, 100)]],
              planes(), b)
    assert got["strand"][:, 0].tolist() == [0, 0, 2]       # columns W - 2 and W - 1, then W and W + 1
    got = run([[(5, 2, 100), (5, 6, 100), (5, 10, 100)]], planes(), b, valid=np.array([1, 0, 1], np.uint8))
    assert got["strand"].tolist() == [[0, 0, 0, 0, 0]]
    got = run([[(5, 2, 100), (5, 6, np.inf)]], planes(), b)
    assert got["strand"].tolist() == [[0, 0, 0, 0, 0]]     # every sample's depth is infinite


def test_segments_of_8192_and_8193_samples_one_point_and_empty_strands():
    b = hr.bounds_of([30])
    got = run([[(6, -4000.25, 100), (6, 4191.75, 100)], [(5, -5000, 100), (5, 5000, 100)], [(3, 3, 50)], [],
               [(2, 2, 60), (2, 3, 60)]], planes(), b)
    assert got["strand"].tolist() == [[W, W, W, 0, W], [0, 0, 0, 1, 0], [0, 0, 0, 0, 0], [0, 0, 0, 0, 0], [1, 1, 1, 0, 1]]
    assert got["view"].tolist() == [W + 1, W + 1, W + 1, 1, W + 1]
    got = run([], planes(), b)
    assert got["strand"].shape == (0, 5) and got["view"].tolist() == [0] * 5 and got["silhouette"].tolist() == [0, 0, H * W]


@pytest.mark.parametrize("threshold", [0.15, 0.2, 0.4])
def test_conf_min_code_is_the_plain_loop_over_the_codes(threshold):
    from monohair_amd import hairreproj
    from monohair_amd.pmvo_utils import map_code_lut

    lut = map_code_lut()
    loop = 256
    for c in range(256):
        if lut[c, 2] > np.float32(threshold):
            loop = c
            break
    assert hairreproj.conf_min_code(threshold) == loop == hr.conf_min_code(threshold)
    assert {0.15: 39, 0.2: 52, 0.4: 103}[threshold] == loop
    assert hairreproj.conf_min_code(1.0) == 256 and hairreproj.conf_min_code(-1.0) == 0


def test_angle_bounds_are_what_the_restatement_is_handed():
    from monohair_amd import hairreproj

    angles, bounds = hairreproj.angle_bounds((10, 20, 30))
    assert angles == [10.0, 20.0, 30.0] and bounds.tobytes() == hr.bounds_of([10, 20, 30]).tobytes()
    for bad in ([], list(range(9)), [91.0], [-1.0]):
        with pytest.raises(ValueError):
            hairreproj.angle_bounds(bad)


def test_prune_strands_on_hand_made_counters():
    from monohair_amd import hairreproj

    #        visible hair conf dropped a10 a30
    rows = np.array([[10, 5, 4, 0, 1, 2],        # both thresholds met with equality: kept
                     [10, 4, 4, 0, 4, 4],        # coverage 0.4: dropped
                     [10, 10, 4, 0, 4, 1],       # agreement 0.25 at the last angle: dropped (0.5 at the first would not be)
                     [0, 0, 0, 0, 0, 0],         # unseen
                     [10, 10, 0, 0, 0, 0],       # seen, on hair, nothing confident: 0 >= 0.5 * 0, kept
                     [3, 3, 3, 2, 3, 3]], np.int64)
    counts = np.array([2, 3, 2, 1, 2, 4], np.int64)
    points = np.arange(int(counts.sum()) * 3, dtype=F32).reshape(-1, 3)
    (kc, kp), keep = hairreproj.prune_strands((counts, points), rows)
    assert keep.tolist() == [True, False, False, True, True, True] and keep.tolist() == hr.prune_mask(rows).tolist()
    assert kc.tolist() == [2, 1, 2, 4] and kp.tolist() == points[[0, 1, 7, 8, 9, 10, 11, 12, 13]].tolist()
    (_, _), keep = hairreproj.prune_strands((counts, points), rows, drop_unseen=True)
    assert keep.tolist() == [True, False, False, False, True, True]
    assert keep.tolist() == hr.prune_mask(rows, drop_unseen=True).tolist()
    (_, _), keep = hairreproj.prune_strands((counts, points), rows, angle_index=0)
    assert keep.tolist() == [False, False, True, True, True, True] == hr.prune_mask(rows, angle_index=0).tolist()
    (_, _), keep = hairreproj.prune_strands((counts, points), rows, min_visible=4, drop_unseen=True)
    assert keep.tolist() == [True, False, False, False, True, False]
    (_, _), keep = hairreproj.prune_strands((counts, points), rows, min_cover=0.5 + 2.0 ** -50, min_agree=0.5)
    assert not keep[0]
    (kc, kp), keep = hairreproj.prune_strands((np.zeros(0, np.int64), np.zeros((0, 3), F32)), np.zeros((0, 6), np.int64))
    assert kc.shape == (0,) and kp.shape == (0, 3) and keep.shape == (0,)
    with pytest.raises(ValueError):
        hairreproj.prune_strands((counts, points), rows[:3])


def test_report_ratios_come_from_the_integer_counts():
    from monohair_amd import hairreproj

    view = np.array([[10, 8, 4, 1, 1, 2, 4], [0, 0, 0, 0, 0, 0, 0]], np.int64)
    sil = np.array([[6, 2, 4], [0, 0, 0]], np.int64)
    res = hairreproj.build_result((10, 20, 30), 0.15, 1, 0.25, np.zeros((3, 7), np.int64), view, sil, 17)
    assert res["overall"]["coverage"] == 0.8 and res["overall"]["confident_share"] == 0.5
    assert res["overall"]["agreement"] == [0.25, 0.5, 1.0]
    assert res["overall"]["silhouette"] == {"precision": 0.75, "recall": 0.6, "iou": 0.5}
    assert res["per_view"][1]["coverage"] == 0.0 and res["per_view"][1]["silhouette"]["iou"] == 0.0
    assert res["overall"]["counts"] == {"visible": 10, "on_hair": 8, "confident": 4, "dropped_segments": 1,
                                        "agrees": [1, 2, 4], "silhouette": [6, 2, 4]}
    assert res["strands"] == 3 and res["points"] == 17 and res["views"] == 2 and res["conf_min_code"] == 39
    assert len(hairreproj.format_scores(res)) == 3
