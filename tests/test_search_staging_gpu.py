"""GPU: how the shipped search brings a point's tap lists into LDS (csrc/pmvo_search.hip: mh_stage_list and the batches of
mh_search_slices_lds) -- every wave copies the lists it owns with loads that write LDS directly, 64 records per instruction, the
key kernels' neutral records behind a list come from one zero record, and one barrier waits for all of it.  The shapes at which
that can go wrong, and no larger: lists that end around the 64-lane border of one copy instruction (patch 9), points whose
records exceed the staging buffer so that a second batch overwrites it (first batch exactly full, one record short, one
over), a second 64-view block, a point no view sees, a one-tap list, key-body lists of every length mod 4 just above
MH_KEY_MIN_TAPS, one and three points, and contexts of 8-bit codes (the select-only kernel).  Every output of forward() is
compared bit for bit with oracle.forward, for the shipped kernel with the key body and with the select body and for the
portable kernel (search_variant 1256).

The scenes are written by hand so that every list length is known: the depth planes are background (255: every view sees
every point, PMVO.py:525-529) except where a (view, point) pixel is set to 0 (hidden); the orientation of pixel (r, c) has
the angle 0.2 + 0.017 * ((r % 11) * 11 + c % 11) + 0.001 * view, so the taps of any window up to 11 x 11 are distinct; the
confidence is 0.9, and a list is cut to `count` taps by lowering the patch cells behind the first `count` (tap order) to 0.05,
as tests/test_key_seed_gpu.py does.  (At least 20 views: forward() ranks the 20 best views of a point.)"""
import numpy as np
import pytest
import torch

import oracle

gpu = pytest.mark.gpu
DEV = "cuda:0"
THR = 0.15
CAP = 1280                # MH_S3_CAP: float4 records of the staging buffer
KEY_MIN_TAPS = 10         # MH_KEY_MIN_TAPS


def staged_records(c, keys, bigp):
    """records of a list of c taps in the staging buffer: header + taps (+ the key body's neutral taps, mh_key_staged)"""
    if c == 0:
        return 0
    if keys and c > KEY_MIN_TAPS:
        return max((c - (0 if bigp else 1) + 3) & ~3, c) + 1
    return c + 1


def batches(cnt_col, keys, bigp=False):
    """record count of every staging batch of one point (one 64-view block: V <= 64)"""
    out, cur = [], 0
    for c in cnt_col:
        r = staged_records(int(c), keys, bigp)
        if r and cur + r > CAP:
            out.append(cur)
            cur = 0
        cur += r
    return out + [cur]


class Scene:
    def __init__(self, V, H, W, patch, npts, min_dist, codes=False, seed=5):
        from monohair_amd import synth
        from monohair_amd.camera import camera_records, cameras_from_list

        self.V, self.H, self.W, self.patch, self.codes = V, H, W, patch, codes
        self.cams = cameras_from_list(synth.make_cameras(V, H, W, rings=2))
        self.rec = camera_records(self.cams)
        r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
        cell = (r % 11) * 11 + c % 11
        self.depth = np.full((V, H, W), 255.0, np.float32)
        if codes:       # orientation codes 20 .. 140 (+ the view), confidence codes 230 / 13, decoded by the loaders' table
            self.k8 = np.stack([(20 + cell + v % 30).astype(np.uint8) for v in range(V)])
            self.c8 = np.full((V, H, W), 230, np.uint8)
            self.m8 = np.full((V, H, W), 255, np.uint8)
        else:
            ang = np.stack([0.2 + 0.017 * cell + 0.001 * v for v in range(V)])
            self.ori = np.stack([np.sin(ang), np.cos(ang)], axis=-1).astype(np.float32)
            self.conf = np.full((V, H, W), 0.9, np.float32)
            self.mask = np.ones((V, H, W), np.float32)
        # points whose pixel lies inside every image by the patch's half width and apart from the other points' in every view
        cand = synth.candidate_points(res=48, seed=seed).astype(np.float32)
        cand = cand[np.random.default_rng(seed).permutation(len(cand))[:4000]]
        hp = patch // 2
        pix = np.stack([oracle.project_points(self.rec[v], cand, H, W)[0] for v in range(V)]).astype(np.int64)   # [V, M, 2]
        oob = np.stack([oracle.project_points(self.rec[v], cand, H, W)[2] for v in range(V)]).astype(bool)
        inside = (~oob & (pix[..., 0] >= hp) & (pix[..., 0] < H - hp) & (pix[..., 1] >= hp) & (pix[..., 1] < W - hp)).all(0)
        keep = []
        for m in np.nonzero(inside)[0]:
            if all(np.abs(pix[:, m] - pix[:, k]).max(axis=1).min() >= min_dist for k in keep):
                keep.append(m)
                if len(keep) == npts:
                    break
        assert len(keep) == npts, "too few points apart from each other"
        self.pts = np.ascontiguousarray(cand[keep])
        # (a batch of one point is projected by another rule, PMVO.py's single-row matmul: project the batch as a whole)
        self.pix = np.stack([oracle.project_points(self.rec[v], self.pts, H, W)[0] for v in range(V)]).astype(np.int64)

    def hide(self, v, n):
        r, c = self.pix[v, n]
        self.depth[v, r, c] = 0.0

    def cut(self, v, n, count):
        hp, k = self.patch // 2, 0
        r, c = self.pix[v, n]
        for i in range(-hp, hp + 1):
            for j in range(-hp, hp + 1):
                if k >= count:
                    if self.codes:
                        self.c8[v, r + i, c + j] = 13
                    else:
                        self.conf[v, r + i, c + j] = 0.05
                k += 1

    def views(self):
        if not self.codes:
            return oracle.Views(self.rec, self.depth, self.ori, self.conf, self.mask)
        from monohair_amd.pmvo_utils import map_code_lut

        lut = map_code_lut()
        return oracle.Views(self.rec, self.depth, lut[self.k8][..., :2].copy(), lut[self.c8][..., 2].copy(),
                            lut[self.m8][..., 3].copy())

    def context(self):
        from monohair_amd.pmvo import PMVO

        kw = dict(device=DEV, patch_size=self.patch, visible_threshold=1, conf_threshold=THR)
        if self.codes:
            return PMVO.from_u8(self.cams, self.depth, self.k8, self.c8, self.m8, image_size=[self.H, self.W], **kw)
        t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)       # noqa: E731
        return PMVO.from_planes(self.rec, t(self.depth), t(self.ori), t(self.conf), t(self.mask), camera=self.cams, **kw)


def run(scene, offsets, expect=None, runs=((0, 0), (1, 0), (2, 0), (0, 1256)), pts=None, ranks=None, num_sample=None, info=None):
    """forward() with (search_body, search_variant) = default, key body, select body, portable kernel against oracle.forward;
    expect = {(v, n): list length}.  Returns the [V, N] list lengths of the front end.  ranks: another set of base-view ranks
    (PMVO.RANKS of the context, nrank / rank_step of the oracle); num_sample: another sample count (the context's and the
    oracle's offsets become depth_offsets(num_sample)); info: a dict that receives the usable ranks per point the context
    reports (search_work) and the oracle's winners."""
    pts = scene.pts if pts is None else pts
    pm = scene.context()
    okw = {}
    if num_sample is not None:
        from monohair_amd.pmvo import depth_offsets

        offsets = depth_offsets(num_sample)
        assert len(offsets) == num_sample
        pm.set_num_sample(num_sample)
    if ranks is not None:
        pm.RANKS = ranks
        okw = dict(nrank=len(ranks), rank_step=ranks[1] - ranks[0] if len(ranks) > 1 else 1)
    _, o_ori, o_loss, o_hc, o_ex = oracle.forward(scene.views(), pts, scene.patch, THR, offsets, extra=True, **okw)
    ref = (o_ori, o_loss, o_hc, o_ex["best_s"], o_ex["best_rank"])
    cnt = None
    try:
        for body, variant in runs:
            pm.set_option("search_body", body)
            pm.set_option("search_variant", variant)
            _, ori, loss, hc, ex = pm.forward(pts, extras=True)
            got = tuple(x.cpu().numpy() for x in (ori, loss, hc, ex["best_s"], ex["best_rank"]))
            if cnt is None:
                cnt, nvalid = pm.search_work(len(pts), ex["base_val"])
                cnt = cnt.cpu().numpy()
                if info is not None:
                    info.update(nvalid=nvalid.cpu().numpy(), best_s=o_ex["best_s"], best_rank=o_ex["best_rank"])
                for (v, n), c in (expect or {}).items():
                    assert cnt[v, n] == c, (v, n, c, int(cnt[v, n]))
            for a, b in zip(got, ref):
                assert a.shape == b.shape and len(a) == len(pts)
                assert np.array_equal(a, b, equal_nan=(a.dtype.kind == "f")), (body, variant)
    finally:
        pm.set_option("search_body", 0)
        pm.set_option("search_variant", 0)
    return cnt, o_loss


@gpu
def test_lists_end_around_the_64_lane_border_of_one_copy_patch9(depth_offsets):
    """62 .. 65 taps + header = 63 .. 66 records: one lane short of, on, and one and two lanes past the border; the key kernel
    for long lists (BIGP) adds its neutral records across the border (62 taps: records 63, 64 of the list are zero)"""
    sc = Scene(20, 240, 160, 9, 5, min_dist=10)
    expect = {}
    for n, count in enumerate((62, 63, 64, 65)):
        sc.cut(2, n, count)
        expect[(2, n)] = count
    cnt, loss = run(sc, depth_offsets, expect)
    assert (cnt[:, 4] == 81).all() and np.isfinite(loss).all()      # complete lists: 82 records, two copy instructions


@gpu
@pytest.mark.parametrize("codes", [False, True])
def test_a_second_batch_overwrites_the_staging_buffer_patch7(codes, depth_offsets):
    """30 views see every point.  Complete lists take 50 records, 25 of them 1250; the 26th visible view's list of 27 .. 30 taps
    makes the first batch end at 1279 (select body: 1278), 1279, 1280 and -- 1281 (key body: 1283) records do not fit -- 1250 records"""
    sc = Scene(30, 240, 160, 7, 5, min_dist=8, codes=codes)
    expect = {}
    for n, count in enumerate((27, 28, 29, 30)):
        sc.cut(25, n, count)
        expect[(25, n)] = count
    cnt, loss = run(sc, depth_offsets, expect, runs=((0, 0), (2, 0), (0, 1256)) if codes else ((0, 0), (1, 0), (2, 0), (0, 1256)))
    assert np.isfinite(loss).all()
    others = np.delete(cnt, 25, axis=0)
    assert (others == 49).all() and (cnt[25, 4] == 49)
    for keys in (False,) if codes else (True, False):
        first = [batches(cnt[:, n], keys)[0] for n in range(5)]
        assert first == [1279 if keys else 1278, 1279, 1280, 1250, 1250], first
        assert all(len(batches(cnt[:, n], keys)) == 2 for n in range(5))


@gpu
@pytest.mark.parametrize("codes", [False, True])
def test_the_second_64_view_block(codes, depth_offsets):
    """V = 67: the list lengths of views 64 .. 66 are not the ones requested in the kernel's prologue.  Point 0 is seen by all
    views (three batches in the first block, one in the second), point 1 by views 3, 65 and 66, point 2 by view 66 alone, point
    3 by no view of the second block"""
    sc = Scene(67, 96, 64, 7, 4, min_dist=2, codes=codes)
    for v in range(67):
        if v not in (3, 65, 66):
            sc.hide(v, 1)
        if v != 66:
            sc.hide(v, 2)
        if v >= 64:
            sc.hide(v, 3)
    sc.cut(65, 1, 12)
    cnt, loss = run(sc, depth_offsets, {(65, 1): 12, (66, 2): 49, (66, 0): 49},
                    runs=((0, 0), (2, 0), (0, 1256)) if codes else ((0, 0), (1, 0), (2, 0), (0, 1256)))
    assert ((cnt[:, 1] > 0) == np.isin(np.arange(67), (3, 65, 66))).all() and (cnt[:, 2] > 0).sum() == 1
    assert (cnt[:, 0] > 0).all() and (cnt[64:, 3] == 0).all() and (cnt[:64, 3] > 0).all()
    assert np.isfinite(loss[[0, 1, 3]]).all()


@gpu
def test_unseen_point_one_tap_list_and_key_lists_of_every_length_mod_4(depth_offsets):
    """N = 3 + 8.  Point 0: no view sees it.  Point 1: one view, a list of one tap.  Points 3 .. 10: view 1 has a list of 11 .. 18
    taps -- the key body walks them in blocks of four and reads 1, 0, 0, 2, 1, 0, 0, 2 neutral records behind them"""
    sc = Scene(20, 240, 160, 7, 11, min_dist=8)
    for v in range(20):
        sc.hide(v, 0)
        if v != 4:
            sc.hide(v, 1)
    sc.cut(4, 1, 1)
    expect = {(4, 1): 1}
    for k, count in enumerate(range(KEY_MIN_TAPS + 1, KEY_MIN_TAPS + 9)):
        sc.cut(1, 3 + k, count)
        expect[(1, 3 + k)] = count
    assert [staged_records(c, True, False) - c - 1 for c in range(11, 19)] == [1, 0, 0, 2, 1, 0, 0, 2]
    cnt, loss = run(sc, depth_offsets, expect)
    assert (cnt[:, 0] == 0).all() and (cnt[:, 1] > 0).sum() == 1
    # three points and one point (the prologue's and the staging's indexing with N = 3 and N = 1; one point alone is its own batch)
    run(sc, depth_offsets, pts=sc.pts[:3])
    run(sc, depth_offsets, pts=sc.pts[5:6])
