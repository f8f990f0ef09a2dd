"""GPU: the votes, the refine loss, the front ends and the search on soft hair masks and on compared quantities that equal their
thresholds (tests/softmask_cases.py): mask codes 50 / 51 and the float neighbours of 0.2f as fractions in the sums over 24 and
272 views, confidences on the threshold codes, depth gaps of exactly 0.1f / 0.9f / 1.0 and one ulp either side.  Plain equality
with the reference's own results (tests/golden/pmvo_softmask.npz, tools/gen_golden_softmask.py) and with the C oracle, from
PMVO.from_u8 and from PMVO.from_planes, in every batch composition and with every kernel form forced."""
import ctypes
import os

import numpy as np
import pytest
import torch

import cascade_cases as cc
import oracle
import softmask_cases as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
eq = lambda a, b: np.array_equal(a, b, equal_nan=True)       # noqa: E731
DEFAULTS = dict(search_body=0, search_variant=0, tap_plane=1, tap_codes=1, taps_tile=1, filter_rows=1)


def host(t):
    return t.cpu().numpy()


class Case:
    def __init__(self, z, V):
        self.z, self.V = z, V
        self.case, self.maps, self.rec = sc.case_of(z, V)
        self.views = {p: oracle.Views(self.rec, *[self.maps[p][k] for k in ("depth", "ori", "conf", "mask")]) for p in sc.PALETTES}
        self.comps = sc.compositions(self.case)
        self.scalp = cc.toy_head()
        self._pm = {}

    def pm(self, pal, thr, patch):
        from scipy.spatial import KDTree

        from monohair_amd.camera import cameras_from_list
        from monohair_amd.pmvo import PMVO

        if (pal, thr, patch) not in self._pm:
            kw = dict(device=DEV, patch_size=patch, visible_threshold=sc.VIS_THR, conf_threshold=thr)
            if pal == "u8":
                c = self.case
                pm = PMVO.from_u8(cameras_from_list(sc.camera_list(self.V)), c["depth"], c["k8"], c["c8"], c["m8"],
                                  image_size=[sc.H, sc.W], lut=self.z["lut"], records=self.rec, **kw)
            else:
                d = {k: torch.from_numpy(v).to(DEV) for k, v in self.maps[pal].items()}
                pm = PMVO.from_planes(self.rec, d["depth"], d["ori"], d["conf"], d["mask"], **kw)
            pm.set_head(KDTree(data=self.scalp[0]), KDTree(data=self.scalp[1]), np.max(self.scalp[1], axis=0))
            self._pm[(pal, thr, patch)] = pm
        return self._pm[(pal, thr, patch)]


@pytest.fixture(scope="module")
def fixture_file():
    return sc.load()


@pytest.fixture(scope="module", params=sc.VIEW_COUNTS)
def case(request, fixture_file):
    return Case(fixture_file[1], request.param)


@pytest.mark.parametrize("pal", sc.PALETTES)
def test_votes_in_every_composition_and_kernel_form(case, fixture_file, pal):
    """the batch and the batches of one: mh_filter_kernel (cascade from LDS, row_sum rows, MhBatch); the tiled batch:
    mh_filter_rows_kernel with its trailing rows by the wave-per-point kernel, and the wave-per-point kernel alone"""
    meta, z = fixture_file
    pp = "v%d_%s_" % (case.V, pal)
    for thr in sc.THRS:
        for patch in sc.PATCHES:
            pm = case.pm(pal, thr, patch)
            key = pp + "t%dp%d_" % (sc.thr_code(thr), patch)
            try:
                for name, p in case.comps.items():
                    o = oracle.filter_votes(case.views[pal], p, patch, thr, sc.VIS_THR)
                    d = torch.from_numpy(p).to(DEV)
                    for rows in ((1, 0) if name == "tiled" else (1,)):
                        pm.set_option("filter_rows", rows)
                        surf, _, filt = pm.filter_points(d)
                        unv = pm.compute_unvisible_points(d)
                        for k, got, want in zip(("surface", "filter", "unvisible"), (surf, filt, unv), o):
                            assert np.array_equal(host(got), z[key + k + "_" + name]), (thr, patch, name, rows, k)
                            assert np.array_equal(host(got), want), (thr, patch, name, rows, k)
                        for vt in meta["head_vis"]:      # (the head vote reads neither the patch nor conf_threshold)
                            head = host(pm.filter_head_points(d, vt))
                            o_head = oracle.filter_votes(case.views[pal], p, patch, thr, vt)[3] & ~cc.head_top(p, case.scalp[1])
                            assert np.array_equal(head, z[pp + "head%g_%s" % (vt, name)]), (name, rows, vt)
                            assert np.array_equal(head, o_head), (name, rows, vt)
            finally:
                pm.set_option("filter_rows", 1)


@pytest.mark.parametrize("pal", sc.PALETTES)
def test_votes_with_the_rows_taken_in_another_order(case, fixture_file, pal):
    """mh_filter_points_ordered on the tiled batch, a permuted and the drivers' cell order: the same votes row for row"""
    from monohair_amd import _lib
    from monohair_amd.pmvo_utils import spatial_order

    meta, z = fixture_file
    thr, patch = sc.THRS[0], sc.PATCHES[0]
    pm = case.pm(pal, thr, patch)
    p = case.comps["tiled"]
    n = len(p)
    d = torch.from_numpy(p).to(DEV)
    want = oracle.filter_votes(case.views[pal], p, patch, thr, sc.VIS_THR)
    key = "v%d_%s_t%dp%d_" % (case.V, pal, sc.thr_code(thr), patch)
    perm = torch.from_numpy(np.random.default_rng(case.V).permutation(n).astype(np.int32)).to(DEV)
    for order in (perm, spatial_order(d)):
        assert sorted(host(order).tolist()) == list(range(n))
        outs = [torch.full((n,), 7, dtype=torch.uint8, device=DEV) for _ in range(4)]
        _lib.check(pm._L.mh_filter_points_ordered(pm._ctx, _lib.ptr(d), n, pm._side, thr, sc.VIS_THR, *[_lib.ptr(o) for o in outs],
                                                  0, 0, 0, _lib.ptr(order), _lib.stream_ptr()), "mh_filter_points_ordered")
        for k, got, w in zip(("surface", "filter", "unvisible", "head"), outs, want):
            assert np.array_equal(host(got).astype(bool), w), k
            if k != "head":
                assert np.array_equal(host(got).astype(bool), z[key + k + "_tiled"]), k


@pytest.mark.parametrize("pal", sc.PALETTES)
def test_refine_loss_front_end_and_combine(case, fixture_file, pal):
    """PMVO.refine (head filter included), mh_refine_loss and mh_refine_loss_maps for the batch and the batches of one; the
    API-visible visible / Conf / mask; mh_refine_combine on the recorded head votes"""
    from monohair_amd import _lib

    meta, z = fixture_file
    pp = "v%d_%s_" % (case.V, pal)
    dirs = z["v%d_dirs" % case.V]
    for thr in sc.THRS:
        for patch in sc.PATCHES:
            pm = case.pm(pal, thr, patch)
            for name, p in case.comps.items():
                if name == "tiled":
                    continue
                dr = dirs if name == "batch" else dirs[case.case["singles"][int(name[3:])]][None]
                N = len(p)
                pts, dd = torch.from_numpy(p).to(DEV), torch.from_numpy(np.ascontiguousarray(dr)).to(DEV)
                want = z[pp + "t%dp%d_refine_%s" % (sc.thr_code(thr), patch, name)]
                assert eq(host(pm.refine(pts, dd)), want), (thr, patch, name)
                o_loss, o_hc = oracle.refine_loss(case.views[pal], p, dr, patch, thr)
                loss, hc = pm.prj_loss_of(pm._points, dd)
                assert eq(host(loss), o_loss) and np.array_equal(host(hc), o_hc), (thr, patch, name)
                lm = torch.empty((N,), dtype=torch.float32, device=DEV)
                hm = torch.empty((N,), dtype=torch.uint8, device=DEV)
                _lib.check(pm._L.mh_refine_loss_maps(pm._ctx, _lib.ptr(pts), _lib.ptr(dd), 0.005, 4.0, N, patch, thr, _lib.ptr(lm),
                                                     _lib.ptr(hm), 0, 0, 0, _lib.stream_ptr()), "mh_refine_loss_maps")
                assert eq(host(lm), o_loss) and np.array_equal(host(hm).astype(bool), o_hc), (thr, patch, name)
                keep = want != -1
                assert eq(host(lm)[keep], want[keep])
                if name == "batch":
                    for k in ("visible", "Conf", "mask"):
                        assert eq(host(getattr(pm, k))[-meta["kept_views"]:], z[pp + k]), k
                    # the smoothing loop's combine on the reference's head decisions: -1 rows become 0.5, orientations swap
                    head = torch.from_numpy((want == -1).astype(np.uint8)).to(DEV)
                    top = torch.zeros_like(head)
                    center = torch.from_numpy(cc.directions(N, 7)).to(DEV)
                    ori_new, loss_out = dd.clone(), torch.empty((N,), device=DEV)
                    _lib.check(pm._L.mh_refine_combine(pm._ctx, _lib.ptr(center), _lib.ptr(lm), _lib.ptr(head), _lib.ptr(top), 0.95,
                                                       _lib.ptr(ori_new), _lib.ptr(loss_out), N, _lib.stream_ptr()), "mh_refine_combine")
                    want_ori = np.ascontiguousarray(dr).copy()
                    oracle.replace_dissimilar(host(center), want_ori, 0.95)
                    assert eq(host(loss_out), np.where(want == -1, np.float32(0.5), want)) and eq(host(ori_new), want_ori)


FORMS = [("default", True, {}), ("taps_tile_64", True, dict(taps_tile=64)), ("taps_tile_32", True, dict(taps_tile=32)),
         ("taps_tile_16", True, dict(taps_tile=16)), ("unfused", False, {}), ("tap_plane_off", True, dict(tap_plane=0)),
         ("variant_100", True, dict(search_variant=100)), ("variant_1256", True, dict(search_variant=1256)),
         ("body_1", True, dict(search_body=1)), ("body_2", True, dict(search_body=2)), ("tap_codes_0", True, dict(tap_codes=0))]


FORM_CASES = [(f, pal) for f in FORMS for pal in sc.PALETTES if pal == "u8" or "tap_codes" not in f[2]]     # (tap codes: 8-bit maps)


@pytest.mark.parametrize("form,pal", FORM_CASES, ids=["%s-%s" % (f[0], pal) for f, pal in FORM_CASES])
def test_forward_in_every_form(case, fixture_file, form, pal):
    """both view counts, thresholds and patch sizes: taps whose confidence IS the threshold, patches whose maximum is, and points
    whose summed weight per seeing view is -- the batch in every form of the search, the batches of one in each front end, the
    tiled batch where the reference's result is recorded"""
    meta, z = fixture_file
    name_f, fused, opts = form
    offs = np.load(os.path.join(GOLDEN, "depth_offsets.npy"))
    for thr in sc.THRS:
        for patch in sc.PATCHES:
            pm = case.pm(pal, thr, patch)
            key = "v%d_%s_t%dp%d_" % (case.V, pal, sc.thr_code(thr), patch)
            try:
                for k, v in opts.items():
                    pm.set_option(k, v)
                for name, p in case.comps.items():
                    if key + "fwd_loss_" + name not in z.files:
                        continue
                    if name != "batch" and name_f not in ("default", "unfused", "tap_codes_0"):
                        continue
                    base = (z[key + "base_idx_" + name], z[key + "base_val_" + name])
                    _, ori, loss, hc = pm.forward(p, base_view=base, fused=fused)
                    got = host(ori), host(loss), host(hc)
                    o = oracle.forward(case.views[pal], p, patch, thr, offs, base_idx=base[0], base_val=base[1])[1:]
                    for want in (tuple(z[key + k + "_" + name] for k in ("fwd_ori", "fwd_loss", "fwd_hc")), o):
                        assert eq(got[1], want[1]) and eq(got[0], want[0]) and np.array_equal(got[2], want[2]), (thr, patch, name)
                    if name_f == "default":
                        _, _, loss2, _, ex = pm.forward(p, extras=True)
                        assert np.array_equal(host(ex["base_val"]), base[1]) and eq(host(loss2), got[1]), (thr, patch, name)
            finally:
                for k in opts:
                    pm.set_option(k, DEFAULTS[k])


def test_tap_lists_hold_exactly_the_eligible_taps(case, fixture_file):
    """the eligibility rule of the search (PMVO.py:162, 174-182: tap 0; every tap unless the patch maximum is > conf_threshold;
    else the taps with conf > conf_threshold) on 8-bit codes (mh_project_taps_codes_kernel) and on floats.  The lists hold the
    first eligible tap of every distinct orientation: the code form's length IS the number of distinct orientation codes among
    the eligible taps; the hash form may keep a duplicate and never holds more than the eligible taps.  A `>=` in either rule
    changes the counts on the tie pairs, which the case holds by the hundred."""
    meta, z = fixture_file
    p = case.comps["batch"]
    assert len(np.unique(z["lut"][:, :2], axis=0)) == 256        # distinct codes are distinct orientations
    for thr in sc.THRS:
        for patch in sc.PATCHES:
            pm = case.pm("u8", thr, patch)
            key = "v%d_u8_t%dp%d_" % (case.V, sc.thr_code(thr), patch)
            cnt = {}
            try:
                for use in (1, 0):
                    pm.set_option("tap_codes", use)
                    pm.forward(p, base_view=(z[key + "base_idx_batch"], z[key + "base_val_batch"]))
                    cnt[use] = host(pm.search_work(len(p))[0])
            finally:
                pm.set_option("tap_codes", 1)
            t = sc.pair_terms(case.rec, p, case.case, case.maps["u8"], patch)
            el, distinct = sc.eligible_taps(t, thr)
            vis = host(pm.visible) > -1
            T = sc.thr_code(thr)
            mx = t["ccode"].max(-1)
            ties = vis & ((mx == T) | ((mx > T) & (t["ccode"][..., 1:] == T).any(-1)))
            assert ties.sum() > 100 and (patch != 3 or (vis & (mx == T)).sum() > 0)
            assert np.array_equal(cnt[1], np.where(vis, distinct, 0)), (thr, patch)
            assert (cnt[0] >= np.where(vis, distinct, 0)).all() and (cnt[0] <= np.where(vis, el.sum(-1), 0)).all(), (thr, patch)


