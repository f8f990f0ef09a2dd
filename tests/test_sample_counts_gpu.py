"""GPU: sample counts other than 90, (a) against the reference itself and (b) in the stand-alone pieces.

(a) tests/golden/pmvo_samples.npz (tools/gen_golden_samples.py) holds the reference's forward() with the default of
sample_next_3d_pos set to S in {1, 16, 60, 100, 102}: PMVO.forward with set_num_sample(S) -- through mh_forward, through
mh_search_prepared with the recorded ranking, and unfused through mh_search_forward -- equals it on every row, bit for bit,
NaN == NaN, with fp32 maps and default options, as the goldens at 90 samples demand; sample_next_3d_pos(points, base, S)
equals the recorded samples.  (tests/test_sample_counts_host.py: the oracle equals the same file.)

(b) mh_sample_next, mh_reproject_ori and mh_prj_loss (loss, index, high_conf and all_loss) against oracle.sample_next,
oracle.reproject_ori and oracle.prj_loss at S in {1, 63, 64, 65, 257, 1000} and at mh_prj_loss's limit 8187 (two floats of LDS
per sample next to 36 bytes: 64 KiB), on 7 and 33 points of pmvo_small: N * S % 32 trailing columns inside a point and
across points, one to 32 rounds of the loss kernel's 256-lane loop, its four-wave argmin.  Exact."""
import ast

import numpy as np
import pytest
import torch

import oracle
from conftest import golden_records, golden_scene, load_golden, rows_equal, scene_views
from test_hip_parity import make_pmvo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SAMPLE_COUNTS = (1, 16, 60, 100, 102)
PRJ_LOSS_MAX_S = 8187        # MH_PRJ_LOSS_MAX_S


def host(t):
    return t.cpu().numpy()


def eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


@pytest.fixture(scope="module", params=["pmvo_small", "pmvo_quant"])
def case(request):
    meta, z = load_golden(request.param)
    scene = golden_scene(meta)
    return request.param, meta, z, make_pmvo(meta, scene, golden_records(z))


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_forward_equals_the_reference_at_other_sample_counts(case, S):
    name, meta, z, pm = case
    g = load_golden("pmvo_samples")[1]
    head = ast.literal_eval(str(g["meta"]))["head"]
    ref = tuple(g["%s__S%d__%s" % (name, S, k)] for k in ("ori", "loss", "hc"))
    pts = z["points"]
    assert len(ref[1]) == len(pts)
    pm.set_num_sample(S)
    try:
        for kw in (dict(), dict(base_view=(z["base_idx"], z["base_val"])), dict(fused=False)):
            got = tuple(host(t) for t in pm.forward(pts, **kw)[1:])
            assert rows_equal(got, ref).all(), sorted(kw)
        samples, surface = pm.sample_next_3d_pos(pts, z["base_idx"][0], S)
        assert eq(host(samples)[:head], g["%s__S%d__samples" % (name, S)]) and samples.shape == (len(pts), S, 3)
    finally:
        pm.set_num_sample(90)


def test_forward_of_one_point_and_one_sample_equals_the_reference(case):
    """N * S = 1 (mh_search_one_column_kernel): every fifth point handed to forward() alone at S = 1, as the reference was"""
    name, meta, z, pm = case
    g = load_golden("pmvo_samples")[1]
    pick = g[name + "__S1__alone_pick"]
    ref = tuple(g["%s__S1__alone_%s" % (name, k)] for k in ("ori", "loss", "hc"))
    assert len(pick) == len(z["points"][::5])
    pm.set_num_sample(1)
    try:
        for kw in (dict(), dict(fused=False)):
            got = [tuple(host(t) for t in pm.forward(z["points"][n:n + 1], **kw)[1:]) for n in pick]
            assert rows_equal(tuple(np.concatenate([r[k] for r in got]) for k in range(3)), ref).all(), sorted(kw)
    finally:
        pm.set_num_sample(90)


# ---- (b) the stand-alone pieces ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def small():
    meta, z = load_golden("pmvo_small")
    scene = golden_scene(meta)
    rec = golden_records(z)
    return meta, z, scene_views(scene, rec), make_pmvo(meta, scene, rec), {}


def pieces_reference(small, N, S):
    """oracle: samples of rank 0, D, (loss, index, high_conf, all_loss) of the first N points at S samples"""
    from monohair_amd.pmvo import depth_offsets

    meta, z, views, pm, cache = small
    if N not in cache:
        cache[N] = oracle.visible_and_ori(views, z["points"][:N], meta["patch"])
    o = cache[N]
    pts, base = z["points"][:N].astype(np.float32), np.ascontiguousarray(z["base_idx"][0][:N])
    offs = depth_offsets(S)
    assert offs.shape == (S,)
    samples = oracle.sample_next(views, pts, base, o["Ori"], offs)
    D = oracle.reproject_ori(views, pts, samples)
    return pts, base, samples, D, oracle.prj_loss(D, o["Ori_patch"], o["Conf_patch"], o["visible"], meta["thr"], want_all=True)


@pytest.mark.parametrize("N", [7, 33])
@pytest.mark.parametrize("S", [1, 63, 64, 65, 257, 1000, PRJ_LOSS_MAX_S])
def test_pieces_at_other_sample_counts(small, S, N):
    from monohair_amd import _lib

    meta, z, views, pm, _ = small
    pts, base, o_samples, o_D, (o_loss, o_idx, o_hc, o_all) = pieces_reference(small, N, S)
    pm.Compute_Visible_and_Ori(pts)
    samples, _ = pm.sample_next_3d_pos(pts, base, S)
    assert eq(host(samples), o_samples)
    D = pm.compute_reproject_ori(pts, samples)
    assert eq(host(D), o_D)
    V, P = D.shape[0], pm.Conf_patch.shape[-1]
    loss = torch.full((N,), -7.0, dtype=torch.float32, device=DEV)
    idx = torch.full((N,), -7, dtype=torch.int64, device=DEV)
    hc = torch.full((N,), 7, dtype=torch.uint8, device=DEV)
    all_loss = torch.full((N, S), -7.0, dtype=torch.float32, device=DEV)
    _lib.check(pm._L.mh_prj_loss(pm._ctx, _lib.ptr(D), _lib.ptr(pm.Ori_patch), _lib.ptr(pm.Conf_patch), _lib.ptr(pm.visible), V,
                                 N, S, P, float(meta["thr"]), _lib.ptr(loss), _lib.ptr(idx), _lib.ptr(hc), _lib.ptr(all_loss),
                                 _lib.stream_ptr()), "mh_prj_loss")
    assert eq(host(loss), o_loss) and np.array_equal(host(idx), o_idx) and np.array_equal(host(hc).astype(bool), o_hc)
    assert eq(host(all_loss), o_all)
    l2, i2, h2 = pm.compute_prj_loss(D)            # (the method: no all_loss)
    assert eq(host(l2), o_loss) and np.array_equal(host(i2), o_idx) and np.array_equal(host(h2), o_hc)
    finite = np.isfinite(o_loss)
    assert finite.sum() >= N // 2 and (o_idx[finite] < S).all()
    if S >= 1000 and N == 33:        # winners in every wave of the 256-lane argmin (at 257 samples: waves 0, 1 and 2)
        assert set((o_idx[finite] % 256) // 64) == {0, 1, 2, 3}


def test_prj_loss_refuses_more_samples_than_its_lds_holds(small):
    from monohair_amd import _lib

    pm = small[3]
    t = torch.full((64,), -7.0, dtype=torch.float32, device=DEV)
    with pytest.raises(_lib.MhError, match="S = 8188 exceeds the limit of 8187 samples"):
        _lib.check(pm._L.mh_prj_loss(pm._ctx, _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), _lib.ptr(t), 1, 1, PRJ_LOSS_MAX_S + 1, 1, 0.1,
                                     _lib.ptr(t), None, None, None, _lib.stream_ptr()), "mh_prj_loss")
    torch.cuda.synchronize()
    assert (t == -7.0).all()
