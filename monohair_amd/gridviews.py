"""What the tools that vote on voxel centres share (hairfill, haircarve): the validated grid arguments of their entry points and
the depth planes of the bust alone for the views of a PMVO object."""
import math

import numpy as np
import torch

from .hairvolume import grid_dims3


def grid(voxel_min, voxel_size, grid_resolution):
    vmin = np.ascontiguousarray(np.asarray(voxel_min, dtype=np.float64).reshape(-1))
    vs = float(voxel_size)
    if vmin.shape != (3,) or not (np.isfinite(vmin).all() and vs > 0.0 and math.isfinite(vs)):
        raise ValueError("voxel_min is three finite numbers, voxel_size a positive one")
    return vmin, vs, grid_dims3(grid_resolution)


def bust_planes(pmvo, bust):
    """float32 [V,H,W] on the device: the planes themselves, or (vertices, faces) drawn per view of `pmvo` at pixel centre 0"""
    H, W = pmvo.image_size
    if isinstance(bust, (tuple, list)) and len(bust) == 2:
        from .camera import camera_records
        from .render import DepthRenderer

        if pmvo.camera_dict is None:
            raise ValueError("a bust mesh needs the cameras of the PMVO object: pass the planes instead")
        r = DepthRenderer([bust], pmvo.device)
        recs = camera_records(pmvo.camera_dict)
        planes = torch.empty((len(recs), H, W), dtype=torch.float32, device=pmvo.device)
        for i in range(len(recs)):
            r.render(recs[i], H, W, 0.0, out=planes[i])
        torch.cuda.current_stream().synchronize()      # (the renderer's scratch is read asynchronously)
        bust = planes
    if not torch.is_tensor(bust):
        bust = torch.from_numpy(np.ascontiguousarray(bust, dtype=np.float32))
    bust = bust.to(pmvo.device, torch.float32).contiguous()
    if tuple(bust.shape) != (pmvo.num_view, H, W):
        raise ValueError("bust planes %r, the views are %r" % (tuple(bust.shape), (pmvo.num_view, H, W)))
    return bust
