"""GPU: a patch side the kernels are not built for (13: odd sides 1..11 are) is refused with MhError by every front end before
anything is launched, and the refusal leaves the process fit for work: a PMVO of patch 7 made afterwards answers forward()
with the oracle's bits.  For Compute_Visible_and_Ori, forward (fused and unfused) and filter_points the refusal is the `-1` a
launcher's patch dispatch (mh_dispatch_patch) answers for a side it has no instantiation of.  refine does not get that far:
mh_refine_loss_maps refuses a side above 11 in the C API itself, before its launcher runs, so its case pins that check and
not the dispatcher.

Two views of 16 x 16 and four points.  With fewer than 20 views forward() has no base-view ranking of its own (torch.topk of the
reference raises too, PMVO.py:341; so does mh_topk_views), so both PMVOs and the oracle get the same injected ranking; with a
side of 13 forward() is refused at its first step, the tap lists, whatever the ranking."""
import numpy as np
import pytest
import torch

import oracle
from monohair_amd import _lib, synth
from monohair_amd.camera import camera_records, cameras_from_list
from monohair_amd.pmvo import PMVO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
V, H, W, THR = 2, 16, 16, 0.15


def test_an_unbuilt_patch_side_is_refused_and_a_built_one_still_works(depth_offsets):
    scene = synth.make_scene(V, H, W, seed=3)
    cams = cameras_from_list(scene["cams"])
    maps = synth.scene_to_reference_dicts(scene)
    pts = synth.candidate_points(res=32, seed=2, limit=4)
    assert pts.shape == (4, 3)
    base = (np.tile((np.arange(20) % V)[:, None], (1, 4)).astype(np.int32), np.ones((20, 4), np.float32))
    dev_pts = torch.from_numpy(pts).float().to(DEV)
    dirs = torch.from_numpy(np.tile(np.float32([0.0, 1.0, 0.0]), (4, 1))).to(DEV)

    pm13 = PMVO(cams, *maps, device=DEV, image_size=[H, W], patch_size=13, visible_threshold=1, conf_threshold=THR)
    assert pm13._side == 13
    for call in (lambda: pm13.Compute_Visible_and_Ori(pts), lambda: pm13.forward(pts, base_view=base),
                 lambda: pm13.forward(pts, base_view=base, fused=False), lambda: pm13.filter_points(dev_pts),
                 lambda: pm13.refine(dev_pts, dirs)):
        with pytest.raises(_lib.MhError):
            call()
    torch.cuda.synchronize()

    pm7 = PMVO(cams, *maps, device=DEV, image_size=[H, W], patch_size=7, visible_threshold=1, conf_threshold=THR)
    _, ori, loss, hc = pm7.forward(pts, base_view=base)
    views = oracle.Views(camera_records(cams), scene["depth"].numpy(), scene["ori"].numpy(), scene["conf"].numpy(),
                         scene["mask"].numpy())
    _, o_ori, o_loss, o_hc = oracle.forward(views, pts, 7, THR, depth_offsets, base_idx=base[0], base_val=base[1])
    assert np.isfinite(o_loss).sum() >= 2          # (the tiny scene is seen: the comparison is not one of NaNs alone)
    assert np.array_equal(loss.cpu().numpy(), o_loss, equal_nan=True)
    assert np.array_equal(ori.cpu().numpy(), o_ori, equal_nan=True)
    assert np.array_equal(hc.cpu().numpy(), o_hc)
