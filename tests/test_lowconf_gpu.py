"""GPU: the search's low-confidence rule `lt(sum(positive_index), 5)` (PMVO.py:198-206) in every place the library writes it out
-- the epilogues of mh_search3_kernel and of the portable mh_search_kernel, mh_prj_loss_kernel, the one-column kernel -- on
points with exactly 0, 1, 4, 5, 6 and 90 positive samples (tests/lowconf_cases.py: 4 and 5 also counted from the far end of the
sweep, where the second lane round of the 64-lane count holds them alone; with patch 7 through the key body; at 4 and 5 samples
in all; with the deciding rank moved by the base-view ranking).  Every output -- orientation, loss, flag, best_s, best_rank -- is
compared exactly with the reference's own run (tests/golden/pmvo_lowconf.npz, tools/gen_golden_lowconf.py) and with the oracle
(tests/test_lowconf_host.py holds the oracle to the same file).  24 views of 240 x 160, 13 points."""
import numpy as np
import pytest
import torch

import lowconf_cases as lc
import oracle
from conftest import rows_equal

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
DEFAULTS = dict(search_body=0, search_variant=0, tap_plane=1, taps_tile=64)
ENTRIES = (("mh_forward", {}), ("prepared", None), ("unfused", dict(fused=False)))        # None: the recorded ranking
FORMS = [dict(search_variant=7), dict(search_variant=100), dict(search_variant=1256), dict(search_body=1), dict(search_body=2),
         dict(tap_plane=0), dict(tap_plane=1), dict(taps_tile=16), dict(taps_tile=32), dict(taps_tile=64),
         dict(search_variant=1256, tap_plane=0), dict(search_body=2, taps_tile=16)]


def host(t):
    return t.cpu().numpy()


def eq(a, b):
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=True)


class Fx:
    def __init__(self):
        from monohair_amd.pmvo import PMVO

        self.meta, self.z = lc.load()
        self.case, self.rec = lc.case_of(self.z)
        self.pts, self.views = self.case["points"], lc.views_of(self.rec, self.case["maps"])
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)       # noqa: E731
        m = self.case["maps"]
        self.pm = {p: PMVO.from_planes(self.rec, t(m["depth"]), t(m["ori"]), t(m["conf"]), t(m["mask"]), device=DEV, patch_size=p,
                                       visible_threshold=1, conf_threshold=lc.THR) for p in (3, 7)}
        self._oracle = {}

    def recorded(self, key):
        return tuple(self.z[key + k] for k in ("fwd_ori", "fwd_loss", "fwd_hc"))

    def oracle_forward(self, patch, S, ranking=None):
        """(ori, loss, hc, best_s, best_rank) of oracle.forward, computed once per (patch, S, ranking)"""
        if (patch, S, ranking) not in self._oracle:
            kw = {} if ranking is None else dict(base_idx=self.z["rk_%s_idx" % ranking], base_val=self.z["rk_%s_val" % ranking])
            _, o, l, h, ex = oracle.forward(self.views, self.pts, patch, lc.THR, lc.offsets(S), extra=True, **kw)
            self._oracle[(patch, S, ranking)] = (o, l, h, ex["best_s"], ex["best_rank"])
        return self._oracle[(patch, S, ranking)]

    def forward(self, patch, S, opts=None, pts=None, **kw):
        pm = self.pm[patch]
        opts = opts or {}
        pm.set_num_sample(S)
        try:
            for k, v in opts.items():
                pm.set_option(k, v)
            _, ori, loss, hc, ex = pm.forward(self.pts if pts is None else pts, extras=True, **kw)
            return host(ori), host(loss), host(hc), host(ex["best_s"]), host(ex["best_rank"])
        finally:
            for k in opts:
                pm.set_option(k, DEFAULTS[k])
            pm.set_num_sample(90)


@pytest.fixture(scope="module")
def fx():
    return Fx()


def check(got, ref, want, what):
    """got = (ori, loss, hc, best_s, best_rank) against the reference's recorded (ori, loss, hc) and the oracle's five"""
    assert rows_equal(got[:3], ref).all(), ("reference", what, np.flatnonzero(~rows_equal(got[:3], ref)))
    assert rows_equal(got[:3], want[:3]).all(), ("oracle", what)
    fin = np.isfinite(want[1])
    assert np.array_equal(got[3][fin], want[3][fin]) and np.array_equal(got[4][fin], want[4][fin]), ("best_s / best_rank", what)


@pytest.mark.parametrize("run", lc.RUNS)
def test_forward_through_every_entry_point(fx, run):
    """mh_forward; mh_forward_prepare + the recorded ranking + mh_search_prepared; the unfused mh_search_forward"""
    patch, S = run
    key = "p%ds%d_" % run
    for name, kw in ENTRIES:
        kw = dict(base_view=(fx.z[key + "base_idx"], fx.z[key + "base_val"])) if kw is None else kw
        check(fx.forward(patch, S, **kw), fx.recorded(key), fx.oracle_forward(patch, S), (run, name))


@pytest.mark.parametrize("opts", FORMS, ids=lambda o: "-".join("%s_%d" % kv for kv in o.items()))
def test_forward_in_every_form_of_the_search(fx, opts):
    """both tap bodies, the portable kernel, the natural point order, the tap plane on and off, 16 / 32 / 64 points per wave of the
    front end: every run of the fixture"""
    for patch, S in lc.RUNS:
        key = "p%ds%d_" % (patch, S)
        check(fx.forward(patch, S, opts), fx.recorded(key), fx.oracle_forward(patch, S), (patch, S))


@pytest.mark.parametrize("name", lc.RANKINGS)
def test_forward_with_the_deciding_rank_moved(fx, name):
    """rank 0 repeated at rank 2 (equal losses: rank 0 stays); the tuned base view at rank 2 with base_val 0 (not taken) and
    with a tiny positive one (taken): the flag comes from the rank that wins"""
    base = (fx.z["rk_%s_idx" % name], fx.z["rk_%s_val" % name])
    for opts in ({}, dict(search_variant=1256), dict(search_body=1), dict(search_body=2), dict(search_variant=7)):
        for kw in (dict(), dict(fused=False)):
            check(fx.forward(3, 90, opts, base_view=base, **kw), fx.recorded("rk_%s_" % name), fx.oracle_forward(3, 90, name),
                  (name, opts, kw))
    if name == "tiny":
        a, b = lc.NAMES.index("k4"), lc.NAMES.index("k5")
        got = fx.forward(3, 90, base_view=base)
        assert (got[4][[a, b]] == 1).all()


@pytest.mark.parametrize("run", lc.RUNS)
def test_prj_loss_alone_on_rank_0(fx, run):
    """the stand-alone compute_prj_loss (mh_prj_loss_kernel) on the rank-0 D: the reference's own (loss, index, flag)"""
    patch, S = run
    key = "p%ds%d_" % run
    pm = fx.pm[patch]
    pm.Compute_Visible_and_Ori(fx.pts)
    samples, _ = pm.sample_next_3d_pos(fx.pts, fx.z[key + "base_idx"][0], S)
    D = pm.compute_reproject_ori(fx.pts, samples)
    assert D.shape == (lc.V, len(fx.pts), S, 2)
    loss, idx, hc = pm.compute_prj_loss(D)
    assert eq(host(loss), fx.z[key + "r0_loss"]) and np.array_equal(host(idx), fx.z[key + "r0_idx"])
    assert np.array_equal(host(hc), fx.z[key + "r0_hc"])
    o, _, _, oD = lc.rank0(fx.views, fx.pts, S, patch)
    assert eq(host(D), oD)
    o_loss, o_idx, o_hc = oracle.prj_loss(oD, o["Ori_patch"], o["Conf_patch"], o["visible"], lc.THR)
    assert eq(host(loss), o_loss) and np.array_equal(host(idx), o_idx) and np.array_equal(host(hc), o_hc)


def test_every_case_point_alone(fx):
    """batches of one point (N = 1), with the case's own sample count and with one sample (N * S = 1: the one-column kernel,
    whose rule is "always low"), against the oracle on the same batch -- the reference's answer holds for its batch only"""
    for ci, (name, patch, S, k, end) in enumerate(lc.CASES):
        p = fx.pts[ci:ci + 1]
        for s in (S, 1):
            _, o, l, h, ex = oracle.forward(fx.views, p, patch, lc.THR, lc.offsets(s), extra=True)
            want = (o, l, h, ex["best_s"], ex["best_rank"])
            for opts, kw in (({}, {}), ({}, dict(fused=False)), (dict(search_variant=1256), {})):
                got = fx.forward(patch, s, opts, pts=p, **kw)
                assert rows_equal(got[:3], want[:3]).all(), (name, s, opts, kw)
                if np.isfinite(l[0]):
                    assert got[3][0] == want[3][0] and got[4][0] == want[4][0], (name, s, opts, kw)


def test_the_code_map_pair(fx):
    """8-bit code maps (PMVO.from_u8): the 4 / 5 pair the generator found on the quantised scene, with the taps gathered as codes
    and as decoded records, both tap bodies and the portable kernel"""
    from monohair_amd.camera import cameras_from_list
    from monohair_amd.pmvo import PMVO

    assert fx.meta["codes"] is not None, "the generator found no 4 / 5 pair on code maps: this test goes with the c8_* records"
    z = fx.z
    cc = lc.codes_case_of(z)
    c, pts = cc["codes"], cc["points"]
    pm = PMVO.from_u8(cameras_from_list(lc.scene_codes()[0]), c["depth"], c["k8"], c["c8"], c["m8"], device=DEV, image_size=[lc.H, lc.W],
                      patch_size=3, visible_threshold=1, conf_threshold=lc.THR, records=fx.rec)
    _, o, l, h, ex = oracle.forward(lc.views_of(fx.rec, lc.decode(c)), pts, 3, lc.THR, lc.offsets(90), extra=True)
    want, ref = (o, l, h, ex["best_s"], ex["best_rank"]), tuple(z["c8_" + k] for k in ("fwd_ori", "fwd_loss", "fwd_hc"))
    for opts in (dict(tap_codes=1), dict(tap_codes=0), dict(search_body=1), dict(search_body=2), dict(search_variant=1256),
                 dict(tap_codes=0, search_body=1)):
        try:
            for k, v in opts.items():
                pm.set_option(k, v)
            for kw in (dict(), dict(base_view=(z["c8_base_idx"], z["c8_base_val"])), dict(fused=False)):
                _, ori, loss, hc, e = pm.forward(pts, extras=True, **kw)
                check((host(ori), host(loss), host(hc), host(e["best_s"]), host(e["best_rank"])), ref, want, (opts, kw))
        finally:
            for k in opts:
                pm.set_option(k, dict(DEFAULTS, tap_codes=1)[k])
    pm.Compute_Visible_and_Ori(pts)
    D = pm.compute_reproject_ori(pts, pm.sample_next_3d_pos(pts, z["c8_base_idx"][0], 90)[0])
    loss, idx, hc = pm.compute_prj_loss(D)
    assert eq(host(loss), z["c8_r0_loss"]) and np.array_equal(host(idx), z["c8_r0_idx"]) and np.array_equal(host(hc), z["c8_r0_hc"])
