"""CPU-only: the numpy restatement of the strand metrics (tests/hair_metrics_np.py) against hand-computed cases and, for its
distance part, against scipy's ball query; the threshold parsing and the report of the command."""
import json

import numpy as np
import pytest

import hair_metrics_np as ref
from monohair_amd import hairmetrics as hm

DEFAULT = hm.DEFAULT_THRESHOLDS


def line(start, direction, n, spacing):
    """n points from `start` along the unit `direction`, float32"""
    k = np.arange(n, dtype=np.float64)[:, None]
    return (np.asarray(start, np.float64) + k * spacing * np.asarray(direction, np.float64)).astype(np.float32)


def wavy_strands(seed, n_strands, n_points, box=0.05, spacing=0.0008):
    """seeded random wavy strands inside a box of `box` metres -> (counts, points float32)"""
    rng = np.random.default_rng(seed)
    pts = []
    for _ in range(n_strands):
        p = rng.uniform(0.0, box, 3)
        d = rng.normal(size=3)
        rows = []
        for _ in range(n_points):
            rows.append(p.copy())
            d = d + 0.35 * rng.normal(size=3)
            d /= np.linalg.norm(d)
            p = p + spacing * d
        pts.append(np.array(rows))
    return [n_points] * n_strands, np.concatenate(pts).astype(np.float32)


def test_default_bounds_match_the_module():
    r2, c = ref.bounds(DEFAULT)
    mr2, mc = hm.threshold_bounds([d for d, _ in DEFAULT], [a for _, a in DEFAULT])
    assert list(r2) == mr2 and list(c) == mc
    assert DEFAULT == ((0.001, 10.0), (0.002, 20.0), (0.003, 30.0))


def test_parallel_strands_1p5_mm_apart():
    """two straight strands 1.5 mm apart: too far for the 1 mm pair, matched by the 2 mm and 3 mm pairs, both ways"""
    a = ([20], line((0, 0, 0), (0, 1, 0), 20, 0.0005))
    b = ([20], line((0.0015, 0, 0), (0, 1, 0), 20, 0.0005))
    counts, flags = ref.score(a, b, DEFAULT)
    assert counts["pred"] == {"matched": [0, 20, 20], "valid": 20, "invalid": 0} == counts["gt"]
    assert (flags["pred"] == 0b110).all() and (flags["gt"] == 0b110).all()
    P, R, F = hm.scores_from_counts(counts["pred"]["matched"], 20, counts["gt"]["matched"], 20)
    assert P == [0.0, 1.0, 1.0] == R == F


def test_strand_against_itself_and_invalid_points():
    """every valid point matches at every pair; a one-point strand and a repeated point have no direction: not scored"""
    counts = [12, 1, 3]
    pts = np.concatenate([line((0, 0, 0), (1, 0, 0), 12, 0.001), [[0.01, 0.01, 0.01]],
                          [[0.02, 0, 0], [0.02, 0, 0], [0.02, 0, 0]]]).astype(np.float32)
    t, valid = ref.tangents(counts, pts)
    assert list(valid) == [1] * 12 + [0] + [0, 0, 0]
    assert np.array_equal(t[:12], np.tile([1.0, 0.0, 0.0], (12, 1))) and not t[12:].any()
    c, flags = ref.score((counts, pts), (counts, pts), DEFAULT)
    assert c["pred"] == {"matched": [12, 12, 12], "valid": 12, "invalid": 4} == c["gt"]
    assert list(flags["pred"]) == [7] * 12 + [0] * 4


def test_perpendicular_strands_that_cross():
    """they touch in a point and still match nowhere: the directions are 90 degrees apart; a cosine bound of 0 admits the
    crossing point and nothing else within half a millimetre"""
    a = ([11], line((-0.005, 0, 0), (1, 0, 0), 11, 0.001))
    b = ([11], line((0, -0.005, 0), (0, 1, 0), 11, 0.001))
    c, _ = ref.score(a, b, DEFAULT)
    assert c["pred"]["matched"] == [0, 0, 0] == c["gt"]["matched"]
    (ta, va), (tb, vb) = ref.tangents(*a), ref.tangents(*b)
    flags = ref.match_flags(a[1], ta, va, b[1], tb, vb, [0.0005 * 0.0005], [0.0])
    assert list(np.nonzero(flags)[0]) == [5]


def test_unsigned_directions_and_inclusive_bounds():
    q = line((0, 0, 0), (1, 0, 0), 3, 2.0 ** -12)
    t = line((2.0 ** -11, 2.0 ** -9, 0), (-1, 0, 0), 3, 2.0 ** -12)      # the same x, run backwards, exactly 2^-9 away
    tq, vq = ref.tangents([3], q)
    tt, vt = ref.tangents([3], t)
    assert np.array_equal(tq, -tt)
    on = ref.match_flags(q, tq, vq, t, tt, vt, [2.0 ** -18], [1.0])
    off = ref.match_flags(q, tq, vq, t, tt, vt, [np.nextafter(2.0 ** -18, 0.0)], [1.0])
    assert list(on) == [1, 1, 1] and list(off) == [0, 0, 0]


def test_resample_by_hand():
    """a 3-4-5 polyline: lengths 5 and 5 (in units of 2^-10), step 2: samples at 0, 2, 4 | 6, 8, 10 -- the last on the end"""
    s = 2.0 ** -10
    pts = (np.array([[0, 0, 0], [3, 4, 0], [3, 4, 5], [3, 4, 5]], np.float64) * s).astype(np.float32)
    counts, out = ref.resample([4], pts, 2 * s)
    assert list(counts) == [6]
    want = np.array([[0, 0, 0], [1.2, 1.6, 0], [2.4, 3.2, 0], [3, 4, 1], [3, 4, 3], [3, 4, 5]], np.float64) * s
    assert np.allclose(out, want, rtol=0, atol=1e-9) and np.array_equal(out[[0, 3, 4, 5]], want[[0, 3, 4, 5]].astype(np.float32))
    # a strand of one point, one of length 0 and one shorter than the step give their first point once
    c, o = ref.resample([1, 2, 2], np.array([[1, 2, 3], [4, 4, 4], [4, 4, 4], [0, 0, 0], [s, 0, 0]], np.float32), 2 * s)
    assert list(c) == [1, 1, 1] and np.array_equal(o, np.array([[1, 2, 3], [4, 4, 4], [0, 0, 0]], np.float32))


def test_distance_part_against_ckdtree():
    """the pairs within each radius are scipy's query_ball_point pairs; no pair lies close enough to a radius (1e-9
    relative) for the two to differ by a rounding"""
    from scipy.spatial import cKDTree

    _, q = wavy_strands(11, 12, 40, box=0.02)
    _, t = wavy_strands(12, 12, 40, box=0.02)
    d2 = ref.squared_distances(q, t)
    tree = cKDTree(t.astype(np.float64))
    total = 0
    for r in (0.001, 0.002, 0.003):
        assert not (np.abs(np.sqrt(d2) - r) <= 1e-9 * r).any()
        balls = tree.query_ball_point(q.astype(np.float64), r)
        for i, ball in enumerate(balls):
            assert sorted(ball) == list(np.nonzero(d2[i] <= np.float64(r) * np.float64(r))[0])
            total += len(ball)
    assert total > 100          # (the clouds do overlap: the comparison is not vacuous)


def test_threshold_parsing():
    assert hm.parse_thresholds("0.001:10,0.002:20,0.003:30") == DEFAULT
    assert hm.parse_thresholds("0.0025:15") == ((0.0025, 15.0),)
    for bad in ("0.001", "0.001:10,", "0:10", "-1:10", "0.001:91", ",".join(["0.001:10"] * 9), "a:b"):
        with pytest.raises(ValueError):
            hm.parse_thresholds(bad)


def test_command_prints_and_writes_the_report(tmp_path, monkeypatch, capsys):
    """the command's host side: one line per pair, the JSON it writes is the dict the API returns (here computed by the
    restatement: no GPU in this test)"""
    a = ([20], line((0, 0, 0), (0, 1, 0), 20, 0.0005))
    b = ([20], line((0.0015, 0, 0), (0, 1, 0), 20, 0.0005))
    seen = {}

    def fake(pred, gt, thresholds, step, device):
        seen.update(pred=pred, gt=gt, thresholds=thresholds, step=step)
        counts, _ = ref.score(a, b, thresholds, step)
        return hm.build_result(thresholds, step, counts, {"pred": 20, "gt": 20}, {"pred": 1, "gt": 1})

    monkeypatch.setattr(hm, "score_strands", fake)
    out = tmp_path / "scores.json"
    assert hm.main(["p.hair", "g.hair", "--thresholds", "0.001:10,0.002:20", "--json", str(out)]) == 0
    assert seen == {"pred": "p.hair", "gt": "g.hair", "thresholds": ((0.001, 10.0), (0.002, 20.0)), "step": None}
    lines = capsys.readouterr().out.strip().splitlines()
    assert len(lines) == 2 and lines[0].startswith("1 mm / 10 deg: precision 0.0000") and "f-score 1.0000" in lines[1]
    got = json.loads(out.read_text())
    assert sorted(got) == ["counts", "f_score", "points", "precision", "recall", "step", "strands", "thresholds"]
    assert got["thresholds"] == [[0.001, 10.0], [0.002, 20.0]] and got["step"] is None
    assert got["precision"] == [0.0, 1.0] == got["recall"] == got["f_score"]
    assert got["counts"] == {"pred": {"matched": [0, 20], "valid": 20, "invalid": 0},
                             "gt": {"matched": [0, 20], "valid": 20, "invalid": 0}}


def test_zero_denominators_score_zero():
    assert hm.scores_from_counts([0, 0], 0, [0, 0], 0) == ([0.0, 0.0], [0.0, 0.0], [0.0, 0.0])
    assert hm.scores_from_counts([3], 4, [0], 5) == ([0.75], [0.0], [0.0])
