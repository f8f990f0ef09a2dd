"""The strand metrics on the GPU (monohair_amd.hairmetrics, csrc/hairmetrics.hip) against their numpy restatement
(tests/hair_metrics_np.py, which tests/test_hair_metrics_host.py holds to hand-computed cases and to scipy's ball query):
exact equality everywhere -- resampled points, tangents, flag bytes, counts."""
import itertools
import json

import numpy as np
import pytest

import hair_metrics_np as ref
from monohair_amd import hairmetrics as hm
from monohair_amd.pmvo_utils import write_strand
from test_hair_metrics_host import line, wavy_strands

pytestmark = pytest.mark.gpu

DEFAULT = hm.DEFAULT_THRESHOLDS
S12 = 2.0 ** -12


def bits(a):
    """bit patterns: equality of these is equality bit for bit (and tells -0 from 0)"""
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def shape_strands():
    """the strands of the resampling and tangent cases -> (counts, points)"""
    rng = np.random.default_rng(5)
    strands = []
    for n in (1, 2, 3, 64, 65, 513):                                   # random walks, segments of about 1 mm
        strands.append(np.cumsum(rng.normal(scale=0.0006, size=(n, 3)), axis=0) + rng.uniform(0, 0.1, 3))
    walk = np.cumsum(rng.normal(scale=0.0006, size=(9, 3)), axis=0)
    strands.append(walk[[0, 0, 0, 1, 2, 3, 4, 5, 6, 7, 8]])              # repeated points at the start,
    strands.append(walk[[0, 1, 2, 3, 3, 3, 4, 5, 5, 6, 7, 8]])           # in the middle
    strands.append(walk[[0, 1, 2, 3, 4, 5, 6, 7, 8, 8, 8]])              # and at the end
    strands.append(walk[[4, 4, 4]])                                      # nothing but one point, three times
    strands.append(np.array([[0.01, 0.02, 0.03], [0.01, 0.02, 0.0302]]))   # shorter than the step
    strands.append(np.zeros((0, 3)))                                     # an empty strand
    strands.append(np.array([[0, 0, 0], [3, 0, 0], [4, 0, 0], [8, 0, 0], [16, 0, 0]]) * S12)      # 4 steps of 2^-10, exactly
    strands.append(np.array([[1, 1, 1], [4, 5, 1], [13, 17, 1], [13, 17, 1]]) * S12)             # 5 steps, zero tail
    return [s.shape[0] for s in strands], np.concatenate(strands).astype(np.float32)


@pytest.mark.parametrize("step", [0.0007, 2.0 ** -10])
def test_resample_equals_the_restatement(step):
    counts, pts = shape_strands()
    want_c, want_p = ref.resample(counts, pts, step)
    got_c, got_p = hm.resample_strands(counts, pts, step)
    assert got_c.dtype == np.int64 and got_p.dtype == np.float32
    assert np.array_equal(got_c, want_c)
    assert np.array_equal(bits(got_p), bits(want_p))
    if step == 2.0 ** -10:           # the last sample of the two exact strands falls on their last point
        assert list(got_c[-2:]) == [5, 6]
        assert np.array_equal(got_p[-1], pts[-1]) and np.array_equal(got_p[-7], np.float32([16 * S12, 0, 0]))


def test_resample_of_nothing():
    c, p = hm.resample_strands([], np.zeros((0, 3), np.float32), 0.001)
    assert c.shape == (0,) and p.shape == (0, 3)
    c, p = hm.resample_strands([0, 0], np.zeros((0, 3), np.float32), 0.001)
    assert list(c) == [0, 0] and p.shape == (0, 3)


def test_tangents_equal_the_restatement():
    counts, pts = shape_strands()
    want_t, want_v = ref.tangents(counts, pts)
    got_t, got_v = hm.strand_tangents(counts, pts)
    assert got_t.dtype == np.float64 and got_v.dtype == np.uint8
    assert np.array_equal(got_v, want_v) and 0 < want_v.sum() < want_v.size
    assert np.array_equal(bits(got_t), bits(want_t))
    t, v = hm.strand_tangents([], np.zeros((0, 3), np.float32))
    assert t.shape == (0, 3) and v.shape == (0,)


# ---------------------------------------------------------------------------------------------------------- match flags
def side(counts, pts):
    """(points, tangents, valid) of a strand set, directions by the restatement: the match tests do not lean on the tangent kernel"""
    pts = np.asarray(pts, np.float32).reshape(-1, 3)
    return (pts,) + ref.tangents(counts, pts)


def check(q, t, thresholds=DEFAULT, r2=None, c=None):
    """flags of the kernel == brute force; -> the flags"""
    if r2 is None:
        r2, c = ref.bounds(thresholds)
    want = ref.match_flags(*q, *t, r2, c)
    got = hm.match_flags(*q, *t, r2=r2, cos=c)
    assert got.dtype == np.uint8 and got.shape == want.shape
    assert np.array_equal(got, want), "flags differ at queries %s" % np.nonzero(got != want)[0][:10]
    return got


_pool = {}


def pool():
    """about 2000 target points and a jittered copy to draw queries from; made once"""
    if not _pool:
        counts, t = wavy_strands(21, 40, 50, box=0.03)
        rng = np.random.default_rng(22)
        q = (t.astype(np.float64) + rng.normal(scale=0.0004, size=t.shape)).astype(np.float32)
        _pool.update(t=side(counts, t), q=side(counts, q))
    return _pool["q"], _pool["t"]


@pytest.mark.parametrize("nt", [0, 1, 2000])
@pytest.mark.parametrize("nq", [0, 1, 63, 64, 65, 257])
def test_flags_by_query_and_target_numbers(nq, nt):
    q, t = pool()
    start = 300                               # (a point inside a strand: its tangent is a central difference)
    got = check(tuple(a[start:start + nq] for a in q), tuple(a[start:start + nt] if nt < 2000 else a for a in t))
    assert got.shape == (nq,)
    if nt == 2000 and nq >= 63:
        assert len(set(got)) > 2              # matched at some pairs, missed at others


def test_flags_with_a_crowded_cell_and_a_grid_of_one_cell():
    """300 targets inside one cell (more than a wave, more than any LDS tile); then those alone: a grid of one cell"""
    rng = np.random.default_rng(31)
    crowd = [np.cumsum(rng.normal(scale=0.00003, size=(50, 3)), axis=0) + 0.0105 for _ in range(6)]
    crowd = ([50] * 6, np.concatenate(crowd))
    assert np.ptp(crowd[1], axis=0).max() < 0.002
    q, t = pool()
    both = ([50] * 6 + [50] * 40, np.concatenate([crowd[1], t[0]]))
    near = ([30] * 20, wavy_strands(32, 20, 30, box=0.004)[1] + np.float32(0.0085))
    got = check(side(*near), side(*both))
    assert len(set(got)) > 2
    got = check(side(*near), side(*crowd))     # one cell: every dimension of the grid is 1
    assert got.any() and not got.all()


def test_flags_of_queries_outside_the_targets_box():
    q, t = pool()
    span = t[0].max(0) - q[0].min(0)
    for axis in range(3):
        for beyond, some in ((-0.01, None), (0.0005, None), (0.004, False), (1.0, False)):
            shift = np.zeros(3, np.float32)
            shift[axis] = span[axis] + beyond          # every query at least `beyond` past the targets' high side
            got = check((q[0] + shift,) + q[1:], t)
            assert some is None or got.any() == some, (axis, beyond)
            shift[axis] = -(q[0].max(0) - t[0].min(0))[axis] - beyond       # ... and past their low side
            got = check((q[0] + shift,) + q[1:], t)
            assert some is None or got.any() == some, (axis, beyond)
    # a query strand 1.2 mm outside the box, next to the target that defines the box's low x and along its direction
    i = int(np.argmin(t[0][:, 0]))
    assert t[2][i] == 1
    mid = t[0][i].astype(np.float64) - [0.0012, 0, 0]
    u = t[1][i] * np.sign(t[1][i][0] or 1.0)
    edge = side([3], np.array([mid - 0.0002 * u - [0.0002, 0, 0], mid, mid + 0.0002 * u - [0.0002, 0, 0]]))
    assert (edge[0][:, 0] < t[0][:, 0].min() - 0.001).all()
    assert check(edge, t)[1] & 0b110 == 0b110


def test_flags_with_eight_pairs_and_with_one():
    q, t = pool()
    eight = tuple((0.0004 * (k + 1), a) for k, a in enumerate((5, 50, 10, 40, 20, 30, 90, 0.5)))
    got = check(q, t, eight)
    assert all(((got >> k) & 1).any() for k in range(7)) and len(set(got)) > 8
    got = check(q, t, ((0.0015, 25.0),))
    assert set(got) == {0, 1}


def test_flags_on_the_bounds_are_inclusive():
    """a target exactly on the radius, then exactly on the angle bound, match; one float64 ulp outside, neither does"""
    q = side([3], line((0, 0, 0), (0, 1, 0), 3, S12))
    t = side([3], line((8 * S12, 0, 0), (0, 1, 0), 3, S12))                 # 2^-9 away across the strand
    c10 = ref.bounds(DEFAULT)[1][:1]
    assert list(check(q, t, r2=[2.0 ** -18], c=c10)) == [1, 1, 1]
    assert list(check(q, t, r2=[np.nextafter(2.0 ** -18, 0.0)], c=c10)) == [0, 0, 0]
    q = side([3], np.float32([[-1, 0, 0], [0, 0, 0], [1, 0, 0]]) * S12)     # direction (1, 0, 0)
    t = side([3], np.float32([[-3, -4, 0], [0, 0, 0], [3, 4, 0]]) * S12)    # direction (0.6, 0.8, 0), crossing at 0
    assert np.array_equal(t[1][1], [0.6, 0.8, 0.0])
    assert list(check(q, t, r2=[(2 * S12) ** 2], c=[0.6])) == [1, 1, 1]
    assert list(check(q, t, r2=[(2 * S12) ** 2], c=[np.nextafter(0.6, 1.0)])) == [0, 0, 0]
    both = check(q, t, r2=[(2 * S12) ** 2, 2.0 ** -40], c=[np.nextafter(0.6, 1.0), 0.6])
    assert list(both) == [0, 2, 0]


def test_flags_across_every_cell_border():
    """query and target on opposite sides of a border of the query's cell, for each of the 26 neighbour cells"""
    tau = DEFAULT[-1][0]
    h, e = tau * 1.01, 0.0004
    inside = {-1: h + e, 0: 1.5 * h, 1: 2 * h - e}
    beyond = {-1: h - e, 0: 1.5 * h, 1: 2 * h + e}
    offsets = [o for o in itertools.product((-1, 0, 1), repeat=3) if o != (0, 0, 0)]
    short = lambda p: line(np.array(p) - [0, 0.00005, 0], (0, 1, 0), 3, 0.00005)          # noqa: E731
    qs = [short([inside[a] for a in o]) for o in offsets]
    ts = [short([0.0, 0.00005, 0.0])] + [short([beyond[a] for a in o]) for o in offsets]       # (the first pins the grid's origin)
    q, t = side([3] * 26, np.concatenate(qs)), side([3] * 27, np.concatenate(ts))
    cells_q = np.floor(q[0].astype(np.float64) / h)
    cells_t = np.floor(t[0][3:].astype(np.float64) / h)
    assert (cells_q == 1).all() and np.array_equal(cells_t[1::3] - 1, np.array(offsets))
    got = check(q, t)
    assert ((got >> 2) & 1).all()
    for o, own in zip(offsets, ts[1:]):       # ... and each against its own neighbour alone
        lone = side([3, 3], np.concatenate([ts[0], own]))
        sel = tuple(a[3 * offsets.index(o):3 * offsets.index(o) + 3] for a in q)
        assert ((check(sel, lone) >> 2) & 1).all(), o


def test_flags_with_invalid_points_and_opposite_directions():
    base = line((0, 0, 0), (1, 0, 0), 10, 0.0005)
    # queries: a strand, a lone point on top of a target, a strand of one repeated point on top of a target
    q = side([10, 1, 3], np.concatenate([base + np.float32([0, 0.0004, 0]), base[4:5], base[[6, 6, 6]]]))
    assert list(q[2]) == [1] * 10 + [0] * 4
    # targets: the same line run backwards, and invalid points right next to the far end of the queries' strand
    far = np.float32([[0.0045, 0.0304, 0]])
    t = side([10, 1, 2], np.concatenate([base[::-1], far, far[[0, 0]]]))
    assert list(t[2]) == [1] * 10 + [0] * 3
    got = check(q, t)
    assert list(got) == [7] * 10 + [0] * 4
    shifted = (q[0] + np.float32([0, 0.03, 0]),) + q[1:]      # now only the invalid targets are within reach
    assert not check(shifted, t).any()


def test_flags_of_a_seeded_sweep():
    """about 20 k points a side at the default thresholds"""
    counts, t = wavy_strands(41, 400, 50, box=0.06)
    rng = np.random.default_rng(42)
    q = (t.astype(np.float64) + rng.normal(scale=0.0004, size=t.shape)).astype(np.float32)
    q[5000:5100] = q[4999]                                    # a run of coincident points: no direction
    got = check(side(counts, q), side(counts, t))
    share = [float(((got >> k) & 1).mean()) for k in range(3)]
    assert 0.02 < share[0] < share[1] < share[2] < 0.98


# --------------------------------------------------------------------------------------------------------------- scores
def test_scores_of_a_file_against_itself(tmp_path):
    counts, pts = wavy_strands(51, 30, 40, box=0.03)
    counts = counts + [1, 3]
    pts = np.concatenate([pts, [[0.5, 0.5, 0.5]], [[0.6, 0.6, 0.6]] * 3]).astype(np.float32)
    path = str(tmp_path / "a.hair")
    write_strand(pts, path, counts)
    r = hm.score_strands(path, path, return_flags=True)
    assert r["precision"] == [1.0] * 3 == r["recall"] == r["f_score"]
    assert r["counts"]["pred"] == {"matched": [1200] * 3, "valid": 1200, "invalid": 4} == r["counts"]["gt"]
    assert r["points"] == {"pred": 1204, "gt": 1204} and r["strands"] == {"pred": 32, "gt": 32}
    assert list(r["flags"]["pred"]) == [7] * 1200 + [0] * 4
    want, _ = ref.score((counts, pts), (counts, pts), DEFAULT)
    assert r["counts"] == want


def test_scores_of_a_shifted_copy_and_of_nothing():
    """strands 1 cm apart against their copy moved 1.5 mm across them: nothing at 1 mm, everything at 2 and 3 mm"""
    pts = np.concatenate([line((0.01 * s, 0, 0), (0, 1, 0), 40, 0.0005) for s in range(8)])
    counts = [40] * 8
    moved = (pts + np.float32([0.0015, 0, 0])).astype(np.float32)
    r = hm.score_strands((counts, pts), (counts, moved))
    assert r["precision"] == [0.0, 1.0, 1.0] == r["recall"] == r["f_score"]
    assert r["counts"]["pred"]["matched"] == [0, 320, 320] == r["counts"]["gt"]["matched"]
    # with resampling the counts are the restatement's on the resampled sets
    r = hm.score_strands((counts, pts), (counts, moved), step=0.0003)
    want, _ = ref.score((counts, pts), (counts, moved), DEFAULT, step=0.0003)
    assert r["counts"] == want and r["points"]["pred"] > 320 and r["precision"] == [0.0, 1.0, 1.0]
    # empty inputs: zero scores, no error
    none = ([], np.zeros((0, 3), np.float32))
    for a, b in ((none, none), (none, (counts, pts)), ((counts, pts), none)):
        r = hm.score_strands(a, b)
        assert r["precision"] == [0.0] * 3 == r["recall"] == r["f_score"]
        assert r["counts"]["pred"]["matched"] == [0] * 3 == r["counts"]["gt"]["matched"]


def test_command_writes_what_the_api_returns(tmp_path, capsys):
    counts, pts = wavy_strands(61, 20, 30, box=0.02)
    rng = np.random.default_rng(62)
    other = (pts.astype(np.float64) + rng.normal(scale=0.0007, size=pts.shape)).astype(np.float32)
    a, b, out = str(tmp_path / "pred.hair"), str(tmp_path / "gt.hair"), str(tmp_path / "s.json")
    write_strand(pts, a, counts)
    write_strand(other, b, counts)
    assert hm.main([a, b, "--step", "0.0005", "--thresholds", "0.001:10,0.002:20", "--json", out]) == 0
    lines = capsys.readouterr().out.strip().splitlines()
    want = hm.score_strands(a, b, ((0.001, 10.0), (0.002, 20.0)), step=0.0005)
    assert lines == hm.format_scores(want) and len(lines) == 2
    assert json.load(open(out)) == json.loads(json.dumps(want))
    assert 0.0 < want["f_score"][0] < want["f_score"][1] < 1.0
