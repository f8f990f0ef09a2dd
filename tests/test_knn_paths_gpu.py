"""GPU: every path of the grid k-NN (GridKNN + csrc/knn.hip) against a float64 brute force, index for index.

The brute force is the reference: scipy's KDTree does not keep index order at exact distance ties (a float32 lattice: 1-5 %
of its rows agree with the stable (d2, index) order), so scipy is only compared where the distances are distinct.  Every
case first asserts that the path it targets ran -- the first attempt's status (query_nosync), `last_retries`,
`last_exhaustive` -- so that a change to how the cell size is picked cannot quietly turn it into a test of the easy path."""
import numpy as np
import pytest
from scipy.spatial import KDTree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def brute_knn(points, queries, k, valid=None):
    """-> (index [Q,k] int64, d2 [Q,k] float64): the k nearest data points of every query in (d2, index) order.
    Data in float64 from float32, queries in their own precision (float32 or float64), d2 = (dx*dx + dy*dy) + dz*dz as the
    kernel and the exhaustive tail compute it; points outside `valid` are at +inf and rows with fewer valid points end in -1."""
    p = np.asarray(points, dtype=np.float32).astype(np.float64)
    q = np.asarray(queries).reshape(-1, 3)
    q = q if q.dtype == np.float64 else q.astype(np.float32).astype(np.float64)
    kk = min(int(k), len(p))
    idx = np.full((len(q), kk), -1, np.int64)
    dist = np.full((len(q), kk), np.inf)
    step = max(1, int(2 ** 24 // max(len(p), 1)))           # [step, M] float64 blocks of at most 128 MB
    for s in range(0, len(q), step):
        qq = q[s:s + step]
        dx = p[None, :, 0] - qq[:, None, 0]
        dy = p[None, :, 1] - qq[:, None, 1]
        dz = p[None, :, 2] - qq[:, None, 2]
        d2 = (dx * dx + dy * dy) + dz * dz
        if valid is not None:
            d2[:, ~np.asarray(valid, bool)] = np.inf
        o = np.argsort(d2, axis=1, kind="stable")[:, :kk]
        dd = np.take_along_axis(d2, o, 1)
        idx[s:s + step] = np.where(np.isinf(dd), -1, o)
        dist[s:s + step] = dd
    return idx, dist


def has_ties(points, queries, k, valid=None):
    """rows whose k nearest (and the next one) hold two equal distances"""
    _, d = brute_knn(points, queries, k + 1, valid)
    return (np.diff(d, axis=1) == 0).any(axis=1)


def check_scipy(points, queries, k, got, valid=None):
    """scipy's KDTree on the valid points (indices mapped back), on the rows where the distances are distinct"""
    sub = np.flatnonzero(valid) if valid is not None else np.arange(len(points))
    kk = min(k, len(sub))
    distinct = ~has_ties(points[sub], queries, kk)
    assert distinct.mean() > 0.5
    _, ref = KDTree(data=points[sub]).query(queries[distinct], kk)
    ref = sub[np.asarray(ref).reshape(-1, kk)]
    assert np.array_equal(got[distinct], ref)


def run(points, queries, k, valid=None, self_query=False, k_hint=None, first_status=None, scipy=False):
    """query() == brute force; query_nosync + finish_nosync == query(); the first attempt's status is as targeted.
    -> (GridKNN, first-attempt status [Q], index [Q,k])"""
    import torch

    from monohair_amd.pmvo_utils import GridKNN

    knn = GridKNN(points, k_hint=k if k_hint is None else k_hint, device=DEV)
    vdev = None if valid is None else torch.from_numpy(np.asarray(valid, np.uint8)).to(DEV)
    idx0, st0 = knn.query_nosync(queries, k, valid_dev=vdev, self_query=self_query)
    st = st0.cpu().numpy()
    first = idx0.cpu().numpy()
    assert set(np.unique(st)) <= {0, 1, 2}
    assert not first[st != 0].any(), "rows the first attempt left unfinished must be zeros"
    if first_status is not None:
        assert (st == first_status).any(), "the first attempt never returned status %d: %s" % (first_status, np.bincount(st))
    got = knn.query(queries, k, self_query=self_query, valid=valid).cpu().numpy()
    retries, exhaustive = knn.last_retries, knn.last_exhaustive
    assert retries == 0 if not st.any() else retries > 0
    # query() clamps k to the number of valid points; query_nosync pads those rows with -1 instead
    ref, _ = brute_knn(points, queries, k, valid)
    kq = min(k, len(points), len(points) if valid is None else int(np.sum(valid)))
    assert got.shape == (len(ref), kq)
    assert np.array_equal(got, ref[:, :kq]) and (ref[:, kq:] == -1).all()
    knn.finish_nosync(queries, k, idx0, st, valid_dev=vdev)
    assert np.array_equal(idx0.cpu().numpy(), ref)
    assert (knn.last_retries, knn.last_exhaustive) == (retries, exhaustive)
    if scipy:
        check_scipy(points, queries, k, got, valid)
    return knn, st, got


# ---------------------------------------------------------------------------------------------------------------- ties
def lattice():
    i = np.arange(20, dtype=np.float32) * np.float32(0.005)
    return np.stack(np.meshgrid(i, i, i, indexing="ij"), -1).reshape(-1, 3).astype(np.float32)


def line():
    return np.stack([np.linspace(0, 1, 3000), np.zeros(3000), np.zeros(3000)], 1).astype(np.float32)


def _first_in_cell(o, h, k):
    """the smallest float32 p whose cell floor((p - o) / h), evaluated in float32, is k: the float below it is in cell k - 1"""
    p = np.float32(o + np.float32(k) * h)
    while np.floor((p - o) / h) < k:
        p = np.nextafter(p, np.float32(np.inf))
    while np.floor((np.nextafter(p, np.float32(-np.inf)) - o) / h) >= k:
        p = np.nextafter(p, np.float32(-np.inf))
    return p


def duplicated():
    rng = np.random.default_rng(3)
    base = rng.random((2500, 3)).astype(np.float32)
    pts = np.concatenate([base, base, base[:1200]])            # every point 2 or 3 times, the copies far apart in index
    return pts[rng.permutation(len(pts))]


@pytest.mark.parametrize("cloud,step,k", [(lattice, 97, 10), (lattice, 97, 27), (line, 29, 50), (duplicated, 31, 10),
                                          (duplicated, 31, 64)])
def test_exact_ties_come_back_in_index_order(cloud, step, k):
    pts = cloud()
    q = pts[::step]
    assert has_ties(pts, q, k).mean() > 0.3                   # the case is about ties
    run(pts, q, k)
    # the self-query: the waves take the points in cell order (qperm), the rows come back in the caller's order
    run(pts, pts, k, self_query=True)


def test_scipy_breaks_lattice_ties_out_of_index_order():
    """why the brute force and not scipy is the reference at ties (docs/PARITY.md)"""
    pts = lattice()
    q = pts[::97]
    ref, _ = brute_knn(pts, q, 10)
    _, kd = KDTree(data=pts).query(q, 10)
    assert (ref == kd).all(1).mean() < 0.5
    assert np.array_equal(np.sort(ref[~has_ties(pts, q, 10)], 1), np.sort(kd[~has_ties(pts, q, 10)], 1))


# ------------------------------------------------------------------------------------------------------------ retries
def test_candidate_overflow_is_retried_on_finer_cells():
    """a dense cluster in a sparse cloud: the first cell size puts thousands of points within reach (status 2)"""
    rng = np.random.default_rng(5)
    clus = rng.normal(0, 0.01, (20000, 3))
    sparse = rng.uniform(-1, 1, (20000, 3))
    pts = np.concatenate([sparse[:10000], clus, sparse[10000:]]).astype(np.float32)
    q = np.concatenate([clus[::97], sparse[::97], clus[:100] + rng.normal(0, 0.002, (100, 3))])
    for k in (16, 100):
        knn, st, _ = run(pts, q.astype(np.float32), k, first_status=2, scipy=True)
        run(pts, q, k, first_status=2)                        # float64 queries


def far_queries(lo, hi, dist):
    """a query beyond every face, edge and corner of the box [lo, hi]"""
    c, half = (lo + hi) / 2, (hi - lo) / 2
    d = np.stack(np.meshgrid([-1, 0, 1], [-1, 0, 1], [-1, 0, 1], indexing="ij"), -1).reshape(-1, 3)
    d = d[np.abs(d).sum(1) > 0]
    return c + d * (half + dist)


@pytest.mark.parametrize("M,k", [(1500, 8), (20000, 8)])
def test_ring_limit_is_retried_on_coarser_cells(M, k):
    """queries far outside the bounding box: no point within six rings of cells (status 1).  With 1500 points the coarser
    cells reach the whole grid and the kernel answers; with 20000 the whole grid overflows and the exhaustive tail does"""
    rng = np.random.default_rng(6)
    pts = rng.random((M, 3)).astype(np.float32)
    q = far_queries(np.zeros(3), np.ones(3), 3.0) + rng.normal(0, 0.01, (26, 3))
    q32 = q.astype(np.float32)
    q64 = q32.astype(np.float64) + 1e-9 * rng.random((26, 3))          # float64 that float32 cannot represent
    assert not np.array_equal(q64, q64.astype(np.float32).astype(np.float64))
    for qq in (q32, q64):
        knn, st, _ = run(pts, qq, k, first_status=1, scipy=True)
        assert st.all()


def test_sparse_outliers_are_retried_on_coarser_cells():
    rng = np.random.default_rng(7)
    out = rng.normal(0, 1, (24, 3))
    out = out / np.linalg.norm(out, axis=1, keepdims=True) * rng.uniform(5, 50, (24, 1))
    pts = np.concatenate([rng.random((20000, 3)), out]).astype(np.float32)
    q = np.concatenate([pts[-24:], pts[-24:].astype(np.float64) + 0.1, pts[:200].astype(np.float64)])
    run(pts, q, 16, first_status=1, scipy=True)


# ------------------------------------------------------------------------------------------------------ exhaustive tail
def copies_cloud(ncopy=2100):
    """a uniform cloud with `ncopy` coincident copies of one point in the middle of its index range"""
    rng = np.random.default_rng(8)
    vol = rng.random((20000, 3)).astype(np.float32)
    c = np.array([0.5, 0.5, 0.5], np.float32)
    pts = np.concatenate([vol[:10000], np.repeat(c[None], ncopy, 0), vol[10000:]])
    q = np.concatenate([c[None].astype(np.float64), c + rng.normal(0, 1e-4, (20, 3)), rng.random((60, 3))])
    return pts, q, np.arange(10000, 10000 + ncopy)


@pytest.mark.parametrize("k", [100, 300])
def test_coincident_copies_reach_the_exhaustive_tail(k):
    """more than 2048 copies of one point: every cell size overflows near them"""
    pts, q, copies = copies_cloud()
    knn, st, got = run(pts, q, k, first_status=2)
    assert knn.last_exhaustive > 0
    assert np.array_equal(got[0], copies[:k])                     # ties among the copies by index
    run(pts, q.astype(np.float32), k, first_status=2)


def test_sparse_query_whose_k_ball_takes_in_a_dense_cluster():
    rng = np.random.default_rng(9)
    clus = rng.normal(0, 1e-3, (5000, 3))
    sparse = rng.uniform(-1, 1, (60, 3))
    pts = np.concatenate([sparse[:30], clus, sparse[30:]]).astype(np.float32)
    q = np.concatenate([rng.uniform(-1, 1, (20, 3)), [[0.9, 0.9, 0.9], [-1.0, 0.3, 0.2]]])
    knn, st, _ = run(pts, q, 100)
    assert st.all() and knn.last_exhaustive > 0


def test_exhaustive_tail_honours_the_validity_mask():
    """copies + a mask that drops some of the copies (the lowest indices among them) and some points nearby: only the
    exhaustive tail answers these queries, so only this reaches its `valid` handling"""
    rng = np.random.default_rng(10)
    pts, q, copies = copies_cloud(2500)
    valid = np.ones(len(pts), bool)
    valid[copies[:300:2]] = False
    valid[copies[-50:]] = False
    near = np.flatnonzero(np.linalg.norm(pts.astype(np.float64) - 0.5, axis=1) < 0.1)
    near = near[(near < copies[0]) | (near > copies[-1])]
    valid[rng.choice(near, len(near) // 3, replace=False)] = False
    assert valid[copies].sum() > 2048
    for k in (100, 300):
        knn, st, got = run(pts, q, k, valid=valid, first_status=2)
        assert knn.last_exhaustive > 0
        assert np.array_equal(got[0], copies[valid[copies]][:k])


# ------------------------------------------------------------------------------------------------------ subset search
def test_subset_search_equals_the_search_of_the_subset():
    """query(valid=mask) on the grid of all points == the brute force (and KDTree) of the masked points, mapped back"""
    rng = np.random.default_rng(11)
    pts = rng.random((20000, 3)).astype(np.float32)
    q = np.concatenate([pts[::71].astype(np.float64), rng.random((200, 3))])
    mask = rng.random(20000) < 0.3
    run(pts, q, 100, valid=mask, scipy=True)
    run(pts, q.astype(np.float32), 100, valid=mask, scipy=True)
    run(pts, pts, 100, valid=mask, self_query=True)
    exact = np.zeros(20000, bool)
    exact[rng.choice(20000, 50, replace=False)] = True             # exactly k valid points
    _, _, got = run(pts, q, 50, valid=exact, scipy=True)
    assert (got >= 0).all() and set(np.unique(got)) == set(np.flatnonzero(exact))
    few = np.zeros(20000, bool)
    few[rng.choice(20000, 20, replace=False)] = True               # fewer than k: query clamps k
    _, _, got = run(pts, q, 50, valid=few, scipy=True)
    assert got.shape == (len(q), 20)
    # kept points much sparser than the grid was laid out for (refine's shell stage): the ring limit
    sparse = np.zeros(20000, bool)
    sparse[rng.choice(20000, 60, replace=False)] = True
    run(pts, q, 30, valid=sparse, first_status=1, scipy=True)


def test_nosync_pads_with_minus_one_when_fewer_points_are_valid_than_k():
    """query_nosync + finish_nosync with valid_dev and fewer valid points than k: the valid neighbours, then -1 -- whether
    the kernel answers (whole grid in reach) or the exhaustive tail does (valid points beyond every cell size's reach)"""
    import torch

    from monohair_amd.pmvo_utils import GridKNN

    rng = np.random.default_rng(12)
    pts = rng.random((3000, 3)).astype(np.float32)
    valid = np.zeros(len(pts), bool)
    valid[rng.choice(len(pts), 10, replace=False)] = True
    q = rng.random((100, 3))
    far = np.concatenate([rng.random((20000, 3)), 100 + rng.random((3, 3))]).astype(np.float32)
    fvalid = np.zeros(len(far), bool)
    fvalid[-3:] = True
    fvalid[:5] = True
    fq = rng.random((40, 3)) * 0.05
    tails = []
    for p, v, qq in ((pts, valid, q), (far, fvalid, fq)):
        knn = GridKNN(p, k_hint=32, device=DEV)
        vdev = torch.from_numpy(v.astype(np.uint8)).to(DEV)
        idx, st = knn.query_nosync(qq, 32, valid_dev=vdev)
        sth = st.cpu().numpy()
        knn.finish_nosync(qq, 32, idx, sth, valid_dev=vdev)
        ref, _ = brute_knn(p, qq, 32, v)
        assert (ref[:, v.sum():] == -1).all() and (ref[:, :v.sum()] >= 0).all()
        assert np.array_equal(idx.cpu().numpy(), ref)
        tails.append(knn.last_exhaustive)
    assert tails[1] > 0


# ------------------------------------------------------------------------------------------------- k and size boundaries
@pytest.mark.parametrize("k", [1, 256, 257, 512, 2048])
def test_k_boundaries(k):
    rng = np.random.default_rng(13)
    pts = rng.random((20000, 3)).astype(np.float32)
    q = np.concatenate([pts[::499], rng.random((40, 3))])
    run(pts, q, k, scipy=k <= 512)
    if k == 2048:                # the whole grid in one buffer: answered by the kernel itself
        small = pts[:2048]
        knn, st, _ = run(small, q, k, scipy=True)
        assert knn.last_exhaustive == 0


def test_candidates_between_512_and_2048_are_answered_by_the_second_launch():
    """for k <= 256 the first launch has a 512-entry buffer; a query with more candidates within reach than that (and at
    most 2048) must be answered by the 2048-entry launch that follows -- not by the retries on other cell sizes.  (A plane of
    points, cells laid out for 600 neighbours, queried for 100 and 200: about 900 points within the first ring's reach.)"""
    rng = np.random.default_rng(17)
    pts = np.concatenate([rng.random((100000, 2)), np.zeros((100000, 1))], 1).astype(np.float32)
    q = np.concatenate([pts[::331], rng.random((100, 3)) * [1.0, 1.0, 0.01]])
    for k in (100, 200):
        knn, st, got = run(pts, q, k, k_hint=600, scipy=True)
        assert knn.last_retries == 0 and not st.any()
    reach = (1.0 - 1.0e-3) * float(knn._grid(knn.h)[0][3])
    p64 = pts.astype(np.float64)
    within = np.array([(((p64 - x) ** 2).sum(1) <= reach * reach).sum() for x in q])
    assert (within > 512).mean() > 0.5 and within.max() <= 2048


def test_k_above_the_buffer_is_refused_and_k_above_m_clamps():
    from monohair_amd._lib import MhError
    from monohair_amd.pmvo_utils import GridKNN

    rng = np.random.default_rng(14)
    pts = rng.random((3000, 3)).astype(np.float32)
    knn = GridKNN(pts, k_hint=100, device=DEV)
    with pytest.raises(MhError):
        knn.query(pts[:10], 2049)
    with pytest.raises(MhError):
        knn.query_nosync(pts[:10], 2049)
    few = pts[:37]
    knn, st, got = run(few, pts[:50], 100)
    assert got.shape == (50, 37)
    one = pts[:1]
    knn, st, got = run(one, pts[:20], 5)
    assert got.shape == (20, 1) and (got == 0).all()


def test_one_cell_and_large_offset():
    """all points inside one cell of the occupancy estimate (h at its ext/480 floor), and coordinates near 1 km with a
    millimetre extent -- float64 queries there are rounded to float32 by more than the reach margin of a cell"""
    rng = np.random.default_rng(15)
    tiny = rng.normal(0, 1e-7, (6000, 3)).astype(np.float32)
    knn, _, _ = run(tiny, tiny[::31], 8)
    assert knn.h == knn._ext / 480.0
    run(tiny, tiny, 8, self_query=True)
    quant = (0.5 + rng.normal(0, 1e-7, (3000, 3))).astype(np.float32)        # a few float32 values per axis: ties
    run(quant, quant[::31], 50)
    run(quant, 0.5 + rng.normal(0, 1e-7, (100, 3)), 50)
    for M in (3000, 20000):
        far = (1000.0 + rng.random((M, 3)) * 1e-3).astype(np.float32)
        q = 1000.0 + rng.random((300, 3)) * 1e-3
        for k in (10, 100):
            run(far, q, k)
            run(far, q.astype(np.float32), k)
            run(far, far[::41], k)


# ---------------------------------------------------------------------------------------------- the grid under the search
@pytest.mark.parametrize("cloud", ["random", "lattice"])
def test_grid_build_equals_numpy(cloud):
    """mh_grid_build: float32 cell keys (x fastest), stable sort, points gathered, first position of every cell.  The cloud
    is joined by points placed for the cell formula (mh_grid_cell) at h = 0.01: exactly on cell boundaries, one float32
    below them, at the grid's origin, and a far corner on a boundary of the float32 formula that the float64 arithmetic
    sizing the grid puts in the cell before -- its cell is the number of cells, where the clamp to dims - 1 decides."""
    from monohair_amd.pmvo_utils import GridKNN

    rng = np.random.default_rng(16)
    pts = lattice() if cloud == "lattice" else rng.normal(0, 0.1, (30000, 3)).astype(np.float32)
    lo, h32 = pts.min(0), np.float32(0.01)
    m = (np.ceil((pts.max(0) - lo) / h32) + 1).astype(int)
    on = np.array([[_first_in_cell(lo[a], h32, k) for a in range(3)] for k in (1, 2, 3, 7)], np.float32)
    far = np.array([next((p for p in (_first_in_cell(lo[a], h32, k) for k in range(m[a], m[a] + 8))
                          if np.floor((np.float64(p) - lo[a]) / float(h32)) < np.floor((p - lo[a]) / h32)),
                         _first_in_cell(lo[a], h32, m[a])) for a in range(3)], np.float32)
    pts = np.concatenate([pts, on, np.nextafter(on, np.float32(-np.inf)), lo[None], far[None]]).astype(np.float32)
    q = np.floor((pts - lo) / h32)                                                        # in float32, as the kernel
    assert np.array_equal(q[-10:-6], q[-6:-2] + 1) and np.array_equal(q[-10:-6, 0], [1, 2, 3, 7]) and not q[-2].any()
    knn = GridKNN(pts, k_hint=27, device=DEV)
    assert np.array_equal(knn._lo, lo) and np.array_equal(knn._hi, far)
    assert (q[-1] == knn._grid(0.01)[1]).any()                        # unclamped, the corner lies one cell too far
    for h in (knn.h, 2 * knn.h, 0.005, 0.01):
        grid, dims, sp, order, start = knn._grid(h)
        o, hh = grid[:3].astype(np.float32), np.float32(grid[3])
        c = np.clip(np.floor((pts - o) / hh), 0, dims.astype(np.float32) - 1).astype(np.int64)     # in float32
        key = (c[:, 2] * int(dims[1]) + c[:, 1]) * int(dims[0]) + c[:, 0]
        ref_order = np.argsort(key, kind="stable")
        ncell = int(dims[0]) * int(dims[1]) * int(dims[2])
        assert np.array_equal(order.cpu().numpy(), ref_order)
        assert np.array_equal(sp.cpu().numpy(), pts[ref_order])
        assert np.array_equal(start.cpu().numpy(), np.searchsorted(key[ref_order], np.arange(ncell + 1)))
