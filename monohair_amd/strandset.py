"""What the strand evaluation tools (synth_hair, hairreproj, hairmetrics, hairvolume) share on the host: a strand set read,
validated and put on the device once, the camera records, and the bust as an occluder plane."""
import numpy as np
import torch

from .camera import camera_records
from .pmvo_utils import load_strand


def _validated(counts, points):
    counts = np.asarray(counts, dtype=np.int64).reshape(-1)
    if (counts < 0).any() or int(counts.sum()) != points.shape[0]:
        raise ValueError("the strand counts sum to %d, there are %d points" % (int(counts.sum()), points.shape[0]))
    if points.shape[0] >= 1 << 31:
        raise ValueError("more than 2^31 - 1 points")
    return counts, points


def load(x):
    """a `.hair` path or (counts, points) -> (counts int64 [S], points float32 [n,3]), contiguous and validated"""
    if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__"):
        x = load_strand(x)      # (load_strand widens the file's float32: exact both ways)
    counts, points = x
    return _validated(counts, np.ascontiguousarray(np.asarray(points, dtype=np.float32).reshape(-1, 3)))


def offsets(counts):
    """int64 [S+1] on the host: strand s is points offsets[s] .. offsets[s+1]"""
    offs = np.zeros(len(counts) + 1, np.int64)
    np.cumsum(counts, out=offs[1:])
    return offs


class StrandSet:
    """A strand set on `device`: counts (host int64 [S]), offsets (device int64 [S+1]), points (device float32 [n,3]), S, n.
    x: what load() takes, or (counts, points tensor) -- a tensor stays on the device.  shift: added on the host,
    float32(float64(x) + shift) per component."""

    def __init__(self, x, device, shift=None):
        if isinstance(x, (tuple, list)) and isinstance(x[1], torch.Tensor):
            self.counts, self.points = _validated(x[0], x[1].to(device=device, dtype=torch.float32).contiguous().reshape(-1, 3))
        else:
            self.counts, pts = load(x)
            if shift is not None:
                pts = np.ascontiguousarray((pts.astype(np.float64) + np.asarray(shift, np.float64).reshape(3)).astype(np.float32))
            self.points = torch.from_numpy(pts).to(device)
        self.offsets = torch.from_numpy(offsets(self.counts)).to(device)
        self.S, self.n = int(self.counts.shape[0]), int(self.points.shape[0])


def records(camera):
    """dict view -> Camera, or [V,48] camera records -> float32 [V,48], contiguous"""
    return np.ascontiguousarray(camera_records(camera) if isinstance(camera, dict) else camera, dtype=np.float32)


class Occluder:
    """bust = (vertices, faces) drawn by render.DepthRenderer at the pixel positions PMVO rounds to; None: no occluder"""

    def __init__(self, bust, device):
        self.renderer = None
        if bust is not None:
            from .render import DepthRenderer

            self.renderer = DepthRenderer([bust], device)

    def plane(self, rec, H, W, pixel_center=0.0):
        """the depth plane float32 [H,W] of one view, or None when there is no bust"""
        return self.renderer.render(rec, H, W, pixel_center) if self.renderer is not None else None
