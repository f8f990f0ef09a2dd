"""GPU: the per-(item, view) projection of the shipped search (csrc/pmvo_search.hip: one_view of mh_search_slices_lds;
csrc/mh_device.h: mh_pixel_of_fast1, mh_unit2_fast1, mh_pixel_of_fast2, mh_unit2_fast2) at every item count a wave can hold.  A
wave holds 0 .. 4 item slices and projects its items in every visible view: the key kernels every item on plain fp32 registers,
the select-only kernel two at a time on register pairs and an odd item alone -- the same operations in the same order.  What
this file adds to tests/test_search_layout_gpu.py is the projection itself: waves of 4, 3, 2, 1 and 0 slices in ONE batch, with
  * a sample offset of exactly 0 among its samples: 16 ranks x 64 samples, and depth_offsets(64)[32] == 0.  That sample lies at
    the point's own depth in the base view, two pixels along the base view's orientation at the point (PMVO.py:263-335) -- so
    the offset alone makes no zero-length segment.  With `still`, the orientation at the point's own pixel is (0, 0) in every
    view: the sample at offset 0 is then the point un-projected from its own pixel position, and in many views it projects
    back onto the point's pixel position to the bit -- the segment (row - row0, col - col0) has length 0, the norm falls
    under the 1e-8 clamp of cosine_similarity, the direction is (0, 0) and every tap's loss is 1 (which no key can state: the
    wave evaluates that view again with the select body).  zero_length_segments() finds those (rank, view, point) with the
    oracle, and the case asserts that waves of 4, 3, 2 and 1 slices each hold one.  (8-bit orientation codes decode to unit
    vectors: no `still` there.)
  * a view that sees the point AT the image border (row 0, row 31, column 0 or column 63), where the patch window hangs over
    the edge; for the wave of one slice that view is the only one.
Both on continuous maps (key body, select body, portable kernel) and on a context of 8-bit codes (the select-only kernel).

Every case compares line_ori, min_loss, high_conf, best_s and best_rank bit for bit, NaN == NaN, with oracle.forward, for the
shipped kernel by the maps, with the key body, with the select body and for the portable kernel (search_variant 1256), through
run() of tests/test_search_staging_gpu.py: 22 views of 32 x 64 pixels, patch 7, six points.  With RANKS = range(16) (rank_step 1)
k views give min(16, k) usable ranks of 64 items: k slices, dealt to the four waves in turn.  Each case states the slices it
means to reach as literals and checks them against plan() of tests/test_search_shapes_gpu.py.

The border points: synth.candidate_points() lie within 0.12 of the origin and project onto rows 8 .. 24, columns 24 .. 40 of
these cameras; twice as far out they reach the edges of some views and stay inside all 22 images.

Not here, because existing tests reach those instantiations with waves of one to three slices: the kernel for lists of more
than 64 taps (tests/test_search_leftover_gpu.py::test_patch_3_and_9: 900, 450 and 720 items on patch 9) and the kernels for more
than 256 views (the pmvo_views300 cases of tests/test_hip_parity.py: 900 items are 4, 4, 4, 3 slices there)."""
import numpy as np
import pytest

import oracle
from test_search_layout_gpu import CODES, RUNS
from test_search_leftover_gpu import show_only, spread
from test_search_shapes_gpu import plan
from test_search_staging_gpu import THR, Scene, run

gpu = pytest.mark.gpu
V, H, W, PATCH, S = 22, 32, 64, 7, 64
RANKS = range(16)
ZERO = 32                     # depth_offsets(64)[32] == 0.0
VIS = (16, 15, 10, 5, 2, 1)   # views that see point n
STATED = ((16, 1024, 0, False, (4, 4, 4, 4)), (15, 960, 0, False, (4, 4, 4, 3)), (10, 640, 0, False, (3, 3, 2, 2)),
          (5, 320, 0, False, (2, 1, 1, 1)), (2, 128, 0, False, (1, 1, 0, 0)), (1, 64, 0, False, (1, 0, 0, 0)))


def on_edge(pix):
    return (pix[..., 0] == 0) | (pix[..., 0] == H - 1) | (pix[..., 1] == 0) | (pix[..., 1] == W - 1)


def scene(border, codes, still=False):
    """six points, point n seen by VIS[n] views.  border: every point lies on the edge of the image in one view that sees it;
    still: the orientation at every point's own pixel is (0, 0) in every view"""
    sc = Scene(V, H, W, PATCH, len(VIS), min_dist=2, codes=codes, seed=1)
    if border:
        from monohair_amd import synth

        cand = (2.0 * synth.candidate_points(res=48, seed=1)).astype(np.float32)
        cand = cand[np.random.default_rng(1).permutation(len(cand))[:4000]]
        prj = [oracle.project_points(sc.rec[v], cand, H, W) for v in range(V)]
        pix = np.stack([p[0] for p in prj]).astype(np.int64)
        inside = ~np.stack([p[2] for p in prj]).astype(bool).any(0)
        keep = []
        for m in np.nonzero(inside & on_edge(pix).any(0))[0]:
            if all(np.abs(pix[:, m] - pix[:, k]).max(axis=1).min() >= 2 for k in keep):
                keep.append(m)
                if len(keep) == len(VIS):
                    break
        assert len(keep) == len(VIS)
        sc.pts = np.ascontiguousarray(cand[keep])
        sc.pix = np.stack([oracle.project_points(sc.rec[v], sc.pts, H, W)[0] for v in range(V)]).astype(np.int64)
    shown = []
    for n, k in enumerate(VIS):
        views = spread(V, n, k)
        if border:      # the first view that has the point on its edge is among the k
            e = int(np.nonzero(on_edge(sc.pix[:, n]))[0][0])
            views = sorted([e] + [v for v in views if v != e][:k - 1])
        assert len(views) == k
        show_only(sc, n, views)
        shown.append(views)
    if still:
        for n in range(len(VIS)):
            for v in range(V):
                sc.ori[v, sc.pix[v, n, 0], sc.pix[v, n, 1]] = 0.0
    return sc, shown


def zero_length_segments(sc):
    """[rank, view, point]: the sample at offset 0 of a usable base-view rank has a direction of exactly (0, 0) in a view that
    sees the point -- the oracle's compute_reproject_ori on the oracle's samples"""
    from monohair_amd.pmvo import depth_offsets

    views = sc.views()
    vo = oracle.visible_and_ori(views, sc.pts, PATCH)
    idx, val = oracle.topk_views(vo["visible"], vo["Conf"])
    out = np.zeros((len(RANKS), V, len(sc.pts)), bool)
    for r in RANKS:
        smp = oracle.sample_next(views, sc.pts, idx[r], vo["Ori"], depth_offsets(S))
        D = oracle.reproject_ori(views, sc.pts, smp)
        out[r] = (D[:, :, ZERO] == 0.0).all(-1) & (vo["visible"] > 0) & (val[r] > 0)[None]
    return out


def check(border, codes, still=False):
    from monohair_amd.pmvo import depth_offsets

    offs = depth_offsets(S)
    assert len(offs) == S and offs[ZERO] == 0.0 and (offs != 0.0).sum() == S - 1
    assert [plan(S, list(RANKS), k, V) for k in VIS] == list(STATED)
    assert sorted({s for p in STATED for s in p[4]}) == [0, 1, 2, 3, 4]
    sc, shown = scene(border, codes, still)
    if border:
        for n, views in enumerate(shown):
            assert on_edge(sc.pix[views, n]).any()
        assert on_edge(sc.pix[shown[5], 5]).all()       # the wave of one slice: its only view
    if still:       # the slices of the waves that hold an item with a zero-length segment
        assert sorted({STATED[n][4][r % 4] for r, v, n in zip(*np.nonzero(zero_length_segments(sc)))}) == [1, 2, 3, 4]
    runs = CODES if codes else RUNS
    info = {}
    cnt, loss = run(sc, None, runs=runs, ranks=list(RANKS), num_sample=S, info=info)
    assert [list(np.nonzero(cnt[:, n])[0]) for n in range(len(VIS))] == shown
    assert list(info["nvalid"]) == [p[0] for p in STATED] and np.isfinite(loss).all()
    run(sc, None, runs=runs, ranks=list(RANKS), num_sample=S, pts=sc.pts[:3])


@gpu
@pytest.mark.parametrize("still", [False, True])
@pytest.mark.parametrize("border", [False, True])
def test_every_slice_count_with_a_zero_offset(border, still):
    """continuous maps: the key body (re-evaluated where a zero-length segment's key is out of range), the select body, the
    portable kernel"""
    check(border, codes=False, still=still)


@gpu
@pytest.mark.parametrize("border", [False, True])
def test_every_slice_count_with_a_zero_offset_8bit(border):
    """views uploaded as 8-bit codes: the select-only kernel"""
    check(border, codes=True)
