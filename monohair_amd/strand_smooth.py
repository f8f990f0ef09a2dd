"""Laplacian smoothing of strands -- Utils/Utils.py:1148-1198 (smnooth_strand / smooth_strands) on the GPU.

The reference solves (A^T A) x = A^T b with scipy's spsolve (SuperLU) once per strand and axis; A^T A is pentadiagonal
plus pos^2 I, and csrc/hairconnect.hip solves it with a float64 banded Cholesky in LAPACK's order (scipy's
solveh_banded), one lane per strand.  The two solvers round differently in float64; what is pinned is the float32 `.hair`
file written from the result."""
import numpy as np
import torch

from . import _lib


def strand_offsets(lens):
    """int64 [n+1]: where each of n strands of the given lengths starts in their concatenation, and the total."""
    offs = np.zeros(len(lens) + 1, np.int64)
    np.cumsum(np.asarray(lens, np.int64), out=offs[1:])
    return offs


def pack_strands(strands, dtype, who, finite=False):
    """The form every strand kernel takes: a list of [L,3] arrays (L >= 2) -> (points [T,3] contiguous in `dtype`, offsets
    int64 [n+1]).  MhError in the name of the caller `who`; finite: also refuse NaN and infinities."""
    arrs = [np.asarray(s, dtype=dtype) for s in strands]
    if any(a.ndim != 2 or a.shape[1] != 3 or a.shape[0] < 2 for a in arrs):
        raise _lib.MhError("%s: every strand must be [L,3] with L >= 2" % who)
    pts = np.ascontiguousarray(np.concatenate(arrs, 0)) if arrs else np.zeros((0, 3), dtype)
    if finite and not np.isfinite(pts).all():
        raise _lib.MhError("%s: non-finite strand points" % who)
    return pts, strand_offsets([a.shape[0] for a in arrs])


def split_strands(pts, offs, which=None):
    """pack_strands' way back: the strands (all, or those of the indices `which`) as views of pts."""
    return [pts[offs[i]:offs[i + 1]] for i in (range(len(offs) - 1) if which is None else which)]


def smooth_strands(strands, lap_constraint=2.0, pos_constraint=1.0, fix_tips=False, device="cuda:0"):
    """Utils.py:1191-1198: replaces every strands[i] ([L,3], L >= 2) by its smoothed copy, in place on the list (with
    fix_tips, strands[i][1:-1] is overwritten instead), and returns the list."""
    if not strands:
        return strands
    if not torch.cuda.is_available():
        raise _lib.MhError("smooth_strands needs a ROCm GPU (no CPU fallback)")
    arrs = [np.asarray(s) for s in strands]
    # b[num_pts:] = smoothed_strand[:, axis] * pos_constraint, evaluated in the strand's dtype like the reference
    rhs, offs = pack_strands([a * pos_constraint for a in arrs], np.float64, "smooth_strands")
    dev = torch.device(device)
    pts = torch.from_numpy(rhs).to(dev)
    offs_d = torch.from_numpy(offs).to(dev)
    work = torch.empty((3 * int(offs[-1]),), dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().mh_smooth_strands(_lib.bare_ctx(dev), _lib.ptr(pts), _lib.ptr(offs_d), len(arrs),
                                                float(lap_constraint), float(pos_constraint), _lib.ptr(work),
                                                _lib.stream_ptr()), "mh_smooth_strands")
    for i, (a, x) in enumerate(zip(arrs, split_strands(pts.cpu().numpy(), offs))):
        if fix_tips:
            a[1:-1] = x[1:-1]
            strands[i] = a
        else:
            sm = np.copy(a)
            sm[:] = x
            strands[i] = sm
    return strands
