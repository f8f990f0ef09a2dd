"""GPU: every front end that restates the reference's border sequence (PMVO.py:378-397, :482-529: round half to even, out_index
on the rounded integers, centre clamped, every tap of the window clamped, soft depth test) on the case of tests/border_cases.py
-- centres on the image edges, in the corners, one pixel either side of them, on exact rounding ties, behind and in the camera
plane, non-finite and huge -- over maps that are random per pixel.  Plain equality with the reference's own results
(tests/golden/pmvo_border.npz, tools/gen_golden_border.py: a fixture the generator proved to change under seven wrong border
rules) and with the C oracle."""
import os

import numpy as np
import pytest
import torch

import border_cases as bc
import cascade_cases as cc
import oracle
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
eq = lambda a, b: np.array_equal(a, b, equal_nan=True)       # noqa: E731
DEFAULTS = dict(search_body=0, search_variant=0, tap_plane=1, tap_codes=1, taps_tile=1, filter_rows=1)


def host(t):
    return t.cpu().numpy()


class Case:
    def __init__(self):
        self.meta, self.z = bc.load()
        self.codes, self.maps, self.rec, self.pts = bc.case(self.z)
        self.views = oracle.Views(self.rec, *[self.maps[k] for k in ("depth", "ori", "conf", "mask")])
        self.offs = np.load(os.path.join(GOLDEN, "depth_offsets.npy"))
        self.classes = bc.classify(self.rec, self.pts)
        self._pm, self._vo, self._fwd = {}, {}, {}

    def pm(self, patch, u8=False):
        """a context of float planes, or of the same maps as 8-bit codes (decoded through the fixture's table)"""
        from monohair_amd.camera import cameras_from_list
        from monohair_amd.pmvo import PMVO

        if (patch, u8) not in self._pm:
            kw = dict(device=DEV, patch_size=patch, visible_threshold=bc.VIS_THR, conf_threshold=bc.THR)
            if u8:
                k8, c8, m8 = self.codes
                pm = PMVO.from_u8(cameras_from_list(bc.cameras()), self.maps["depth"], k8, c8, m8, image_size=[bc.H, bc.W],
                                  lut=self.z["lut"], records=self.rec, **kw)
            else:
                d = {k: torch.from_numpy(v).to(DEV) for k, v in self.maps.items()}
                pm = PMVO.from_planes(self.rec, d["depth"], d["ori"], d["conf"], d["mask"], **kw)
            self._pm[(patch, u8)] = pm
        return self._pm[(patch, u8)]

    def oracle_patches(self, patch):
        if patch not in self._vo:
            self._vo[patch] = oracle.visible_and_ori(self.views, self.pts, patch)
        return self._vo[patch]

    def oracle_forward(self, patch):
        if patch not in self._fwd:
            pre = "f%d_" % patch
            self._fwd[patch] = oracle.forward(self.views, self.pts, patch, bc.THR, self.offs, base_idx=self.z[pre + "base_idx"],
                                              base_val=self.z[pre + "base_val"])[1:]
        return self._fwd[patch]


@pytest.fixture(scope="module")
def case():
    return Case()


def test_project_points_in_every_view(case):
    z, pm = case.z, case.pm(1)
    o_rc, o_zp, o_oob, _ = bc.project(case.rec, case.pts)
    for v in range(bc.V):
        rc, zp, oob = (host(t) for t in pm.project_points(case.pts, v))
        for want in ((z["uv"][v], z["zp"][v], z["out_index"][v]), (o_rc[v], o_zp[v], o_oob[v])):
            assert np.array_equal(rc, want[0]) and eq(zp, want[1]) and np.array_equal(oob, want[2]), v


@pytest.mark.parametrize("patch", bc.PATCHES)
def test_compute_visible_and_ori(case, patch):
    """mh_project_gather, and the stand-alone gathers of pmvo_pieces.hip on the reference's clamped centres; patch 4 is the
    reference's 5 x 5 window (test_even_patch_size_uses_the_reference_tap_window)"""
    z, pm, o = case.z, case.pm(patch), case.oracle_patches(patch)
    pm.Compute_Visible_and_Ori(case.pts)
    got = {k: host(getattr(pm, k)) for k in bc.RESULT_KEYS}
    assert got["Ori_patch"].shape[2] == bc.side(patch) ** 2
    for k in ("visible", "Ori", "Conf", "mask"):
        assert eq(got[k], z[k]) and eq(got[k], o[k]), k
    pr = z["pairs"]
    for k in ("Ori_patch", "Conf_patch"):
        assert eq(got[k], o[k]), k
        assert eq(got[k][pr[:, 0], pr[:, 1]], z["p%d_%s" % (patch, k)]), k
    for v in (0, bc.HAND):
        uv = torch.from_numpy(z["uv"][v].astype(np.int64))
        assert eq(host(pm.get_ori_patch(uv, v, patch)), o["Ori_patch"][v])
        assert eq(np.clip(host(pm.get_c_patch(uv, v, patch)), np.float32(1e-6), np.float32(1)), o["Conf_patch"][v])
        assert eq(host(pm.get_ori(uv, v)), z["Ori"][v]) and eq(host(pm.get_mask(uv, v)), z["mask"][v])


FORMS = [("default", False, True, {}),
         ("taps_tile_64", False, True, dict(taps_tile=64)),
         ("taps_tile_32", False, True, dict(taps_tile=32)),
         ("taps_tile_16", False, True, dict(taps_tile=16)),
         ("unfused", False, False, {}),
         ("tap_plane_off", False, True, dict(tap_plane=0)),
         ("variant_1256", False, True, dict(search_variant=1256)),
         ("body_1", False, True, dict(search_body=1)),
         ("body_2", False, True, dict(search_body=2)),
         ("u8_codes", True, True, dict(tap_codes=1)),
         ("u8_records", True, True, dict(tap_codes=0))]


@pytest.mark.parametrize("patch", (7, 11))
@pytest.mark.parametrize("form", FORMS, ids=[f[0] for f in FORMS])
def test_forward_in_every_form(case, patch, form):
    """rows 135 (0.125, 0, 1) and 219 (0, 0, 1) lie exactly in the hand-made camera's plane and are seen by one other view: the
    reference adds NaN x weight 0 of the unseen view into its sums (PMVO.py:191-198), so their loss is NaN, first sample of rank 0"""
    name, u8, fused, opts = form
    z, pm, pre = case.z, case.pm(patch, u8), "f%d_" % patch
    try:
        for k, v in opts.items():
            pm.set_option(k, v)
        _, ori, loss, hc = pm.forward(case.pts, base_view=(z[pre + "base_idx"], z[pre + "base_val"]), fused=fused)
        got = (host(ori), host(loss), host(hc))
        front = {k: host(getattr(pm, k)) for k in ("visible", "Ori", "Conf", "mask")}
        own = None
        if name in ("default", "u8_codes"):        # mh_forward: the library's own ranking gives the recorded values
            _, ori2, loss2, hc2, ex = pm.forward(case.pts, extras=True)
            own = host(ex["base_val"]), host(loss2)
    finally:
        for k in opts:
            pm.set_option(k, DEFAULTS[k])
    o_ori, o_loss, o_hc = case.oracle_forward(patch)
    for want in ((z[pre + "fwd_ori"], z[pre + "fwd_loss"], z[pre + "fwd_hc"]), (o_ori, o_loss, o_hc)):
        assert eq(got[1], want[1]) and eq(got[0], want[0]) and np.array_equal(got[2], want[2])
    for k, a in front.items():          # the API-visible centre values, out-of-bounds pairs included
        assert eq(a, z[k]), k
    if own is not None:
        assert np.array_equal(own[0], z[pre + "base_val"])


@pytest.mark.parametrize("patch", (7, 11))
def test_tap_lists_drop_the_repeated_edge_taps(case, patch):
    z, pm, pre = case.z, case.pm(patch, True), "f%d_" % patch
    cnt = {}
    try:
        for use in (1, 0):
            pm.set_option("tap_codes", use)
            pm.forward(case.pts, base_view=(z[pre + "base_idx"], z[pre + "base_val"]))
            cnt[use] = host(pm.search_work(len(case.pts))[0])
    finally:
        pm.set_option("tap_codes", 1)
    assert (cnt[1] <= cnt[0]).all()
    assert np.array_equal(cnt[1] > 0, cnt[0] > 0)
    assert not ((cnt[0] > 0) & (z["visible"] == -1)).any()         # no list for a pair the view does not see
    hp = bc.side(patch) // 2
    clamped = np.zeros_like(case.classes["interior"])
    for k in range(hp):
        for name in ("col_%d", "col_W-1-%d", "row_%d", "row_H-1-%d"):
            clamped |= case.classes[name % k]
    seen = clamped & (cnt[0] > 0)
    assert seen.sum() > 100
    for use in (1, 0):
        assert (cnt[use][seen] < patch * patch).all(), use


def test_votes_wave_per_point_and_lane_per_point(case):
    """296 points: mh_filter_kernel.  The batch tiled 14 times (4144 = 129 * 32 + 16 points): mh_filter_rows_kernel, its
    trailing 16 rows by the wave-per-point kernel; and the wave-per-point kernel alone on the same launch (filter_rows 0)."""
    z, pm = case.z, case.pm(case.meta["vote_patch"])
    patch = case.meta["vote_patch"]
    tiled = np.tile(case.pts, (bc.TILE, 1))
    assert len(tiled) >= 4096
    try:
        for pre, p, rows in (("", case.pts, 1), ("tiled_", tiled, 1), ("tiled_", tiled, 0)):
            pm.set_option("filter_rows", rows)
            d = torch.from_numpy(p).to(DEV)
            surf, _, filt = pm.filter_points(d)
            unv = pm.compute_unvisible_points(d)
            o_s, o_f, o_u, _ = oracle.filter_votes(case.views, p, patch, bc.THR, bc.VIS_THR)
            for want in ((z[pre + "surface_index"], z[pre + "filter_index"], z[pre + "unvisible_index"]), (o_s, o_f, o_u)):
                assert np.array_equal(host(surf), want[0]) and np.array_equal(host(filt), want[1]), (pre, rows)
                assert np.array_equal(host(unv), want[2]), (pre, rows)
    finally:
        pm.set_option("filter_rows", 1)


def test_refine_loss_both_entry_points(case):
    from scipy.spatial import KDTree

    from monohair_amd import _lib

    z, patch = case.z, case.meta["vote_patch"]
    pm = case.pm(patch)
    bust, scalp = cc.toy_head()
    pm.set_head(KDTree(data=bust), KDTree(data=scalp), np.max(scalp, axis=0))
    rows = z["refine_rows"]
    keep = z["refine_loss"] != -1
    assert keep.sum() > 64
    # the finite points with the head filter (PMVO.refine), then without it through mh_refine_loss and mh_refine_loss_maps; then
    # every point, the non-finite ones included (scipy's tree refuses those, so the reference's refine cannot be asked)
    for sel in (rows, np.arange(len(case.pts))):
        p, dr = case.pts[sel], z["dirs"][sel]
        N = len(p)
        pts, dirs = torch.from_numpy(p).to(DEV), torch.from_numpy(dr).to(DEV)
        o_loss, o_hc = oracle.refine_loss(case.views, p, dr, patch, bc.THR)
        if sel is rows:
            assert eq(host(pm.refine(pts, dirs)), z["refine_loss"])
        pm.Compute_Visible_and_Ori(pts)
        loss, hc = pm.prj_loss_of(pm._points, dirs)
        assert eq(host(loss), o_loss) and np.array_equal(host(hc), o_hc)
        lm = torch.empty((N,), dtype=torch.float32, device=DEV)
        hm = torch.empty((N,), dtype=torch.uint8, device=DEV)
        _lib.check(pm._L.mh_refine_loss_maps(pm._ctx, _lib.ptr(pts), _lib.ptr(dirs), 0.005, 4.0, N, patch, bc.THR, _lib.ptr(lm),
                                             _lib.ptr(hm), 0, 0, 0, _lib.stream_ptr()), "mh_refine_loss_maps")
        assert eq(host(lm), o_loss) and np.array_equal(host(hm).astype(bool), o_hc)
        if sel is rows:
            assert eq(host(lm)[keep], z["refine_loss"][keep]) and eq(host(loss)[keep], z["refine_loss"][keep])
