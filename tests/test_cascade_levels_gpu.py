"""GPU: the kernels' hand-written restatements of ATen's cascade sums at the sizes where another level begins -- sums over
255 .. 4095 views (mh_row_sum_views, mh_inner_sum_views, MhCascV and their copies in the search, refine, filter and pieces
kernels) and means over groups of 127 .. 9728 members (MhInnerSum, both launches, the LDS and the staged path).  Every
comparison is plain equality with the reference's own results (tests/golden/cascade_views.npz, consensus_levels.npz,
tools/gen_golden_cascade.py: fixtures the generator proved to change when a level is left out) and with the C oracle."""
import os

import numpy as np
import pytest
import torch

import cascade_cases as cc
import oracle
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
eq = lambda a, b: np.array_equal(a, b, equal_nan=True)       # noqa: E731


def host(t):
    return t.cpu().numpy()


@pytest.fixture(scope="module")
def views_file():
    return cc.load("cascade_views")


@pytest.fixture(scope="module")
def groups_file():
    return cc.load("consensus_levels")


def make_pmvo(maps, rec):
    from monohair_amd.pmvo import PMVO

    d = {k: torch.from_numpy(v).to(DEV) for k, v in maps.items()}
    return PMVO.from_planes(rec, d["depth"], d["ori"], d["conf"], d["mask"], device=DEV, patch_size=cc.PATCH,
                            visible_threshold=cc.VIS_THR, conf_threshold=cc.THR)


@pytest.fixture(scope="module", params=cc.VIEW_COUNTS)
def case(request, views_file):
    meta, z = views_file
    V = request.param
    maps, rec, c = cc.views_case(meta, z, V)
    views = oracle.Views(rec, maps["depth"], maps["ori"], maps["conf"], maps["mask"])
    return V, meta["cases"][V], c, views, make_pmvo(maps, rec)


def test_prj_loss_on_the_recorded_inputs(case):
    """mh_prj_loss: [V, 17 * 90] sums, 47 blocks of 32 columns in cascade order and 26 trailing columns in row_sum order"""
    from monohair_amd import _lib

    V, info, c, views, pm = case
    D, op, cp, vis = cc.loss_inputs(V, info["loss_seed"])
    N, P = cc.N_LOSS, cc.PATCH ** 2
    dev = [torch.from_numpy(a).to(DEV) for a in (D, op, cp, vis)]
    loss = torch.empty((N,), dtype=torch.float32, device=DEV)
    idx = torch.empty((N,), dtype=torch.int64, device=DEV)
    hc = torch.empty((N,), dtype=torch.uint8, device=DEV)
    _lib.check(pm._L.mh_prj_loss(pm._ctx, *[_lib.ptr(t) for t in dev], V, N, cc.S, P, cc.THR, _lib.ptr(loss), _lib.ptr(idx),
                                 _lib.ptr(hc), None, _lib.stream_ptr()), "mh_prj_loss")
    o_loss, o_idx, o_hc = oracle.prj_loss(D, op, cp, vis, cc.THR)
    for want in ((c["loss"], c["idx"], c["hc"]), (o_loss, o_idx, o_hc)):
        assert eq(host(loss), want[0]) and np.array_equal(host(idx), want[1]) and np.array_equal(host(hc).astype(bool), want[2])


@pytest.mark.parametrize("variant,body", [(0, 0), (100, 0), (1256, 0), (0, 1), (0, 2)])
def test_forward_with_the_recorded_base_views(case, variant, body):
    V, info, c, views, pm = case
    offs = np.load(os.path.join(GOLDEN, "depth_offsets.npy"))
    pm.set_option("search_body", body)
    pm.set_option("search_variant", variant)
    try:
        _, ori, loss, hc = pm.forward(c["points"], base_view=(c["base_idx"], c["base_val"]))
        got = (host(loss), host(ori), host(hc))
    finally:
        pm.set_option("search_body", 0)
        pm.set_option("search_variant", 0)
    _, o_ori, o_loss, o_hc = oracle.forward(views, c["points"], cc.PATCH, cc.THR, offs, base_idx=c["base_idx"],
                                            base_val=c["base_val"])
    for want in ((c["fwd_loss"], c["fwd_ori"], c["fwd_hc"]), (o_loss, o_ori, o_hc)):
        assert eq(got[0], want[0]) and eq(got[1], want[1]) and np.array_equal(got[2], want[2])
    if variant == 0 and body == 0:
        # the library's own base-view ranking: up to 1024 views it gives the recorded values (indices of equal values are
        # not compared); above, it refuses and the caller has to bring a ranking
        from monohair_amd import _lib

        if V <= 1024:
            _, ori, loss, hc, ex = pm.forward(c["points"], extras=True)
            assert np.array_equal(host(ex["base_val"]), c["base_val"]) and eq(host(loss), c["fwd_loss"])
        else:
            with pytest.raises(_lib.MhError):
                pm.forward(c["points"])


VOTE_VMAX = 512      # MH_FILTER_VMAX / MH_REFINE_VMAX: the vote and refine-loss kernels keep a point's per-view terms in LDS


def test_filter_votes(case):
    from monohair_amd import _lib

    V, info, c, views, pm = case
    pts = torch.from_numpy(c["vote_points"]).to(DEV).float()
    if V > VOTE_VMAX:
        for call in (pm.filter_points, pm.compute_unvisible_points):
            with pytest.raises(_lib.MhError, match="mh_filter_points: unsupported size/shape"):
                call(pts)
        return
    surf, _, filt = pm.filter_points(pts)
    unv = pm.compute_unvisible_points(pts)
    o_s, o_f, o_u, _ = oracle.filter_votes(views, c["vote_points"], cc.PATCH, cc.THR, cc.VIS_THR)
    for want in ((c["surface_index"], c["filter_index"], c["unvisible_index"]), (o_s, o_f, o_u)):
        assert np.array_equal(host(surf), want[0]) and np.array_equal(host(filt), want[1]) and np.array_equal(host(unv), want[2])


def test_refine_loss_both_entry_points(case):
    """[V, 45] sums: 32 points in cascade order, 13 trailing points in row_sum order.  mh_refine_loss (through PMVO.refine, head
    filter included) and mh_refine_loss_maps up to their limit of 512 views; both refuse more."""
    from scipy.spatial import KDTree

    from monohair_amd import _lib

    V, info, c, views, pm = case
    bust, scalp = cc.toy_head()
    pm.set_head(KDTree(data=bust), KDTree(data=scalp), np.max(scalp, axis=0))
    pts = torch.from_numpy(c["vote_points"]).to(DEV).float()
    dirs = torch.from_numpy(c["dirs"]).to(DEV)
    N = len(pts)
    lm = torch.empty((N,), dtype=torch.float32, device=DEV)
    hm = torch.empty((N,), dtype=torch.uint8, device=DEV)
    if V > VOTE_VMAX:
        with pytest.raises(_lib.MhError, match="unsupported size/shape"):
            pm.refine(pts, dirs)
        pm.Compute_Visible_and_Ori(pts)
        with pytest.raises(_lib.MhError, match="mh_refine_loss: unsupported size/shape"):
            pm.prj_loss_of(pm._points, dirs)
        rc = pm._L.mh_refine_loss_maps(pm._ctx, _lib.ptr(pts), _lib.ptr(dirs), 0.005, 4.0, N, cc.PATCH, cc.THR, _lib.ptr(lm),
                                       _lib.ptr(hm), 0, 0, 0, _lib.stream_ptr())
        assert rc != 0 and b"views exceed the limit of 512" in pm._L.mh_last_error()
        return
    loss = host(pm.refine(pts, dirs))
    assert eq(loss, c["refine_loss"])
    o_loss, o_hc = oracle.refine_loss(views, c["vote_points"], c["dirs"], cc.PATCH, cc.THR)
    keep = c["refine_loss"] != -1
    assert eq(loss[keep], o_loss[keep]) and keep.sum() > 20
    _lib.check(pm._L.mh_refine_loss_maps(pm._ctx, _lib.ptr(pts), _lib.ptr(dirs), 0.005, 4.0, N, cc.PATCH, cc.THR, _lib.ptr(lm),
                                         _lib.ptr(hm), 0, 0, 0, _lib.stream_ptr()), "mh_refine_loss_maps")
    assert eq(host(lm), o_loss) and np.array_equal(host(hm).astype(bool), o_hc)
    assert eq(host(lm)[keep], c["refine_loss"][keep])


def test_the_search_refuses_4096_views(views_file):
    from monohair_amd import _lib

    meta, z = views_file
    base = {k: z["base_" + k] for k in ("depth", "ori", "conf", "mask")}
    _, rec, c = cc.views_case(meta, z, 255)
    nb = len(base["depth"])
    rec = cc.view_records(rec[:nb], 4096)
    pm = make_pmvo(cc.view_maps(base, 4096, 1), rec)
    N = len(c["points"])
    ranking = (np.tile(np.arange(20, dtype=np.int32)[:, None], (1, N)), np.ones((20, N), np.float32))
    for fused in (True, False):
        with pytest.raises(_lib.MhError, match="V >= 4096 needs a fourth cascade level"):
            pm.forward(c["points"], base_view=ranking, fused=fused)
    t = torch.zeros(8, device=DEV)
    assert pm._L.mh_prj_loss(pm._ctx, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 4096, 1, 1, 1, cc.THR,
                             _lib.ptr(t), None, None, None, _lib.stream_ptr()) != 0
    assert b"mh_prj_loss: bad arguments" in pm._L.mh_last_error()


# ------------------------------------------------------------------------------------------------------- member sums
def medoid_call(fn, *args):
    from monohair_amd import _lib
    from monohair_amd.pmvo_utils import _ctx_for

    _lib.check(getattr(_lib.lib(), fn)(_ctx_for(DEV), *args, _lib.stream_ptr()), fn)


@pytest.mark.parametrize("K", cc.GROUP_SIZES)
def test_member_sums_dense_indexed_and_segmented(groups_file, K):
    """one group of K members through mh_medoid_dense, mh_medoid_indexed (identity and a permuted index) and
    mh_medoid_segmented: the launch for fewer than 512 members with 128 and with 256 threads, the four-level launch, the
    LDS path up to 4096 members and the staged path above"""
    from monohair_amd import _lib
    from monohair_amd.pmvo_utils import compute_points_similarity

    meta, z = groups_file
    g = cc.group(K, meta["cases"][K]["seed"])
    want, widx = z["k%d_out" % K], int(z["k%d_index" % K])
    o_out, o_idx = oracle.medoid_dense(g[None])
    assert int(o_idx[0]) == widx and np.array_equal(o_out, want)
    gd = torch.from_numpy(g).to(DEV)
    out, idx = compute_points_similarity(gd[None], return_index=True)
    assert int(idx[0]) == widx and np.array_equal(host(out), want)
    perm = np.random.default_rng(K).permutation(K)
    inv = np.empty(K, np.int64)
    inv[perm] = np.arange(K)
    for rows, index in ((g, np.arange(K)), (g[perm], inv)):           # rows[index] == g
        assert np.array_equal(rows[index], g)
        out = torch.full((1, 3), 7.0, device=DEV)
        idx = torch.full((1,), -1, dtype=torch.int32, device=DEV)
        rows_d, index_d = torch.from_numpy(rows).to(DEV), torch.from_numpy(index.astype(np.int32)).to(DEV)
        medoid_call("mh_medoid_indexed", _lib.ptr(rows_d), _lib.ptr(index_d), 1, K, _lib.ptr(out), _lib.ptr(idx))
        assert int(idx[0]) == widx and np.array_equal(host(out), want)
    out = torch.full((1, 3), 7.0, device=DEV)
    idx = torch.full((1,), -1, dtype=torch.int32, device=DEV)
    seg_d = torch.tensor([0, K], dtype=torch.int32, device=DEV)
    medoid_call("mh_medoid_segmented", _lib.ptr(gd), _lib.ptr(seg_d), 1, K, _lib.ptr(out), _lib.ptr(idx))
    assert int(idx[0]) == widx and np.array_equal(host(out), want)


def test_member_sums_of_every_size_in_one_segmented_call(groups_file):
    """all the fixture's groups, with groups of 1 and 3 members between them, in one mh_medoid_segmented call: every workgroup
    of both launches has to find the form that owns its group"""
    from monohair_amd import _lib

    meta, z = groups_file
    rng = np.random.default_rng(3)
    parts, want, widx, named = [], [], [], []
    for K in cc.GROUP_SIZES:
        for n in (1, 3):
            small = (rng.random((n, 3), dtype=np.float32) - np.float32(0.5)).astype(np.float32)
            o, i = oracle.medoid_dense(small[None])
            parts.append(small), want.append(o[0]), widx.append(int(i[0])), named.append(n)
        parts.append(cc.group(K, meta["cases"][K]["seed"]))
        want.append(z["k%d_out" % K][0]), widx.append(int(z["k%d_index" % K])), named.append(K)
    sizes = [len(p) for p in parts]
    seg = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    ori = np.concatenate(parts).astype(np.float32)
    G = len(sizes)
    out = torch.full((G, 3), 7.0, device=DEV)
    idx = torch.full((G,), -1, dtype=torch.int32, device=DEV)
    ori_d, seg_d = torch.from_numpy(ori).to(DEV), torch.from_numpy(seg).to(DEV)
    medoid_call("mh_medoid_segmented", _lib.ptr(ori_d), _lib.ptr(seg_d), G, max(sizes), _lib.ptr(out), _lib.ptr(idx))
    got_i, got_o = host(idx), host(out)
    bad = [named[k] for k in range(G) if got_i[k] != widx[k] or not np.array_equal(got_o[k], want[k])]
    assert not bad, bad
    o_out, o_idx = oracle.medoid_segmented(ori, seg)
    assert np.array_equal(got_i, o_idx) and np.array_equal(got_o, o_out)
