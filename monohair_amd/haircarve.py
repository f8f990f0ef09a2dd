"""Coarse geometry from the hair masks: a classical stand-in for the two inputs of PMVO.py that the reference takes from
instant-ngp, the coarse surface `ours/colmap_points.obj` that candidates are sampled around and the depth maps
`render_depth/<view>.npy` behind every visibility decision.  From what a capture has at that point (cameras, hair masks, the
fitted bust) it carves the visual hull: every voxel centre of the candidate grid is voted on by the views (a view in which the
bust does not hide the voxel must see hair there), the voxels that pass are INSIDE, and the boundary of the INSIDE set is written
as a closed triangle mesh in an order fixed by the rule.  The depth maps are that mesh and the bust drawn by the depth
rasteriser.  The reference has no counterpart, so the specification is the rule written out in include/mh_pmvo.h ("Silhouette
carve") and restated in numpy by tests/hair_carve_np.py.  A hull lies on or outside the true surface: what that costs is
measured, not assumed (docs/PARITY.md, f11).

    python -m monohair_amd.haircarve --yaml=configs/reconstruct/<case> [--voxel-size 0.00125] [--min-free 2] [--max-miss 0]
                                     [--depth-bias-mm 0] [--force]

reads hair_mask/, ours/cam_params.json and the bust, and writes ours/colmap_points.obj and render_depth/<view>.npy; PMVO.py
then runs as it does on instant-ngp's files.  The kernels are csrc/haircarve.hip.  There is no CPU path."""
import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _lib, gridviews
from ._lib import host_ptr

# the grid PMVO.py's main hands to load_colmap_points (with args.bbox_min): voxel 0.005 / 4, 512 x 512 x 384
CARVE_VOXEL_SIZE = 0.005 / 4
CARVE_GRID = (512, 512, 384)


def carve_grid(voxel_size=CARVE_VOXEL_SIZE):
    """dims (X, Y, Z) of the candidate grid's extent (0.64 x 0.64 x 0.48) at another voxel size, rounded up"""
    vs = float(voxel_size)
    if not (vs > 0.0 and math.isfinite(vs)):
        raise ValueError("voxel_size must be positive, got %r" % voxel_size)
    return tuple(int(math.ceil(g * CARVE_VOXEL_SIZE / vs - 1e-9)) for g in CARVE_GRID)


def _limits(min_free, max_miss):
    min_free, max_miss = int(min_free), int(max_miss)
    if min_free < 1 or max_miss < 0:
        raise ValueError("min_free must be >= 1 and max_miss >= 0, got %r and %r" % (min_free, max_miss))
    return min_free, max_miss


# ------------------------------------------------------------------------------------------------- 1. votes, the inside flag
def carve_votes(pmvo, bust_planes, grid_resolution=CARVE_GRID, voxel_min=None, voxel_size=CARVE_VOXEL_SIZE):
    """The three vote counts of every voxel centre over the views of `pmvo` (a PMVO object of fp32 planes or 8-bit codes; only
    its cameras and masks are read).  bust_planes: float32 [V,H,W], the depth of the bust alone in PMVO's convention, 255 where
    there is none (or (vertices, faces), drawn here).  -> int32 [X,Y,Z,3] = n_in, n_free, n_miss."""
    vmin, vs, dims = gridviews.grid(_vmin(voxel_min), voxel_size, grid_resolution)
    nvox = int(np.prod(dims.astype(np.int64)))
    with torch.cuda.device(pmvo.device):
        bust = gridviews.bust_planes(pmvo, bust_planes)
        counts = torch.empty((nvox, 3), dtype=torch.int32, device=pmvo.device)
        _lib.check(_lib.lib().mh_carve_votes(pmvo._ctx, _lib.ptr(bust), host_ptr(vmin), vs, host_ptr(dims), _lib.ptr(counts),
                                             _lib.stream_ptr()), "mh_carve_votes")
        return counts.cpu().numpy().reshape(int(dims[0]), int(dims[1]), int(dims[2]), 3)


def _vmin(voxel_min):
    from .pmvo_utils import VOXEL_MIN

    return VOXEL_MIN if voxel_min is None else voxel_min


def _inside_dev(pmvo, bust, vmin, vs, dims, min_free, max_miss):
    nvox = int(np.prod(dims.astype(np.int64)))
    flags = torch.empty(nvox, dtype=torch.uint8, device=pmvo.device)
    _lib.check(_lib.lib().mh_carve_inside(pmvo._ctx, _lib.ptr(bust), host_ptr(vmin), vs, host_ptr(dims), min_free, max_miss,
                                          _lib.ptr(flags), _lib.stream_ptr()), "mh_carve_inside")
    return flags


def carve_inside(pmvo, bust_planes, grid_resolution=CARVE_GRID, voxel_min=None, voxel_size=CARVE_VOXEL_SIZE, min_free=2,
                 max_miss=0):
    """The INSIDE flag of every voxel: n_free >= min_free and n_miss <= max_miss.  -> uint8 [X,Y,Z]."""
    vmin, vs, dims = gridviews.grid(_vmin(voxel_min), voxel_size, grid_resolution)
    min_free, max_miss = _limits(min_free, max_miss)
    with torch.cuda.device(pmvo.device):
        flags = _inside_dev(pmvo, gridviews.bust_planes(pmvo, bust_planes), vmin, vs, dims, min_free, max_miss)
        return flags.cpu().numpy().reshape(int(dims[0]), int(dims[1]), int(dims[2]))


# ------------------------------------------------------------------------------------------------- 2. the hull as a mesh
def _mesh_dev(flags, vmin, vs, dims, device):
    """flags: uint8 device tensor [X*Y*Z] -> (vertices float32 [Nv,3], faces int32 [Nt,3]) on the device"""
    L, st = _lib.lib(), _lib.stream_ptr()
    need = int(L.mh_carve_mesh_scratch_bytes(host_ptr(dims)))
    if need == 0:
        raise ValueError("a hull mesh needs X*Y*Z and (X+1)*(Y+1)*(Z+1) below 2^31, got %r" % (tuple(int(d) for d in dims),))
    ctx = _lib.bare_ctx(device)
    scratch = torch.empty(need, dtype=torch.uint8, device=device)
    counts = torch.empty(2, dtype=torch.int64, device=device)
    _lib.check(L.mh_carve_mesh_count(ctx, _lib.ptr(flags), host_ptr(dims), _lib.ptr(counts), _lib.ptr(scratch), need, st),
               "mh_carve_mesh_count")
    nv, nt = (int(c) for c in counts.cpu().numpy())
    vertices = torch.empty((nv, 3), dtype=torch.float32, device=device)
    faces = torch.empty((nt, 3), dtype=torch.int32, device=device)
    _lib.check(L.mh_carve_mesh(ctx, _lib.ptr(flags), host_ptr(vmin), vs, host_ptr(dims), nv, nt,
                               _lib.ptr(vertices) if nv else None, _lib.ptr(faces) if nt else None, _lib.ptr(scratch), need, st),
               "mh_carve_mesh")
    return vertices, faces


def hull_mesh(flags, voxel_min=None, voxel_size=CARVE_VOXEL_SIZE, device="cuda:0"):
    """The boundary of the INSIDE voxels as a closed triangle mesh.  flags: [X,Y,Z], non-zero = INSIDE (numpy or a tensor).
    -> (vertices float32 [Nv,3] in world coordinates, faces int32 [Nt,3]): the used grid corners ascending, two triangles per
    exposed face in voxel order and direction order -x, +x, -y, +y, -z, +z, counter-clockwise seen from outside."""
    if torch.is_tensor(flags):
        shape, f = tuple(flags.shape), (flags != 0).to(device=device, dtype=torch.uint8).contiguous().reshape(-1)
    else:
        a = np.asarray(flags)
        shape, f = a.shape, None
    if len(shape) != 3:
        raise ValueError("flags are [X,Y,Z], got shape %r" % (shape,))
    vmin, vs, dims = gridviews.grid(_vmin(voxel_min), voxel_size, shape)
    if int(_lib.lib().mh_carve_mesh_scratch_bytes(host_ptr(dims))) == 0:      # (before anything of that size is made)
        raise ValueError("a hull mesh needs X*Y*Z and (X+1)*(Y+1)*(Z+1) below 2^31, got %r" % (shape,))
    with torch.cuda.device(device):
        if f is None:
            f = torch.from_numpy(np.ascontiguousarray(a != 0).view(np.uint8).reshape(-1)).to(device)
        v, t = _mesh_dev(f, vmin, vs, dims, torch.device(device))
        return v.cpu().numpy(), t.cpu().numpy()


# ------------------------------------------------------------------------------------------------- the pieces together
def mask_context(masks, cameras, image_size=None, device="cuda:0"):
    """A PMVO context of the hair masks and the cameras alone: masks is a dict view -> uint8 [H,W] (or [V,H,W] in view order);
    the depth, orientation and confidence planes a context holds are constants (255, code 0, code 0) that the carve never
    reads."""
    from .pmvo import PMVO

    keys = list(cameras.keys())
    first = masks[keys[0]] if isinstance(masks, dict) else masks[0]
    H, W = (int(image_size[0]), int(image_size[1])) if image_size is not None else tuple(first.shape[:2])
    depth = np.full((H, W), 255.0, np.float32)
    zero = np.zeros((H, W), np.uint8)
    V = len(keys)
    return PMVO.from_u8(cameras, [depth] * V, [zero] * V, [zero] * V, masks, device=device, image_size=[H, W], patch_size=3)


def carve(pmvo_or_masks, cameras, bust, voxel_size=CARVE_VOXEL_SIZE, min_free=2, max_miss=0, voxel_min=None,
          grid_resolution=None, image_size=None, device="cuda:0"):
    """The hull of the hair masks outside the head.  pmvo_or_masks: a PMVO object (cameras may then be None), or the hair
    masks as mask_context takes them with `cameras` a dict view -> Camera; bust: (vertices, faces) in world coordinates, or
    float32 [V,H,W] planes of the bust alone.  The grid is PMVO.py's candidate grid (voxel_min, its extent at voxel_size)
    unless grid_resolution is given.  -> (vertices float32 [Nv,3] world, faces int32 [Nt,3], flags uint8 [X,Y,Z])."""
    pmvo = pmvo_or_masks if hasattr(pmvo_or_masks, "_ctx") else mask_context(pmvo_or_masks, cameras, image_size, device)
    grid = carve_grid(voxel_size) if grid_resolution is None else grid_resolution
    vmin, vs, dims = gridviews.grid(_vmin(voxel_min), voxel_size, grid)
    min_free, max_miss = _limits(min_free, max_miss)
    with torch.cuda.device(pmvo.device):
        flags = _inside_dev(pmvo, gridviews.bust_planes(pmvo, bust), vmin, vs, dims, min_free, max_miss)
        v, t = _mesh_dev(flags, vmin, vs, dims, pmvo.device)
        return v.cpu().numpy(), t.cpu().numpy(), flags.cpu().numpy().reshape(int(dims[0]), int(dims[1]), int(dims[2]))


def depth_bias(bias_mm):
    """the float32 constant a depth bias in millimetres adds to a hull pixel: depth planes hold -z_camera / 2 * 255"""
    return np.float32(float(bias_mm) / 1000.0 / 2.0 * 255.0)


def carve_depth(pmvo, vertices, faces, bust, bias_mm=0.0):
    """The depth maps of the hull and the bust for the views of `pmvo` (its cameras): each drawn alone by the depth rasteriser
    at the pixel positions PMVO rounds to, depth_bias(bias_mm) added to the hull plane where it is not 255, then the per-pixel
    minimum.  bust: (vertices, faces) in world coordinates.  -> float32 [V,H,W]."""
    with torch.cuda.device(pmvo.device):
        hull = gridviews.bust_planes(pmvo, (vertices, faces)) if len(faces) else \
            torch.full((pmvo.num_view,) + tuple(pmvo.image_size), 255.0, dtype=torch.float32, device=pmvo.device)
        head = gridviews.bust_planes(pmvo, bust)
        hull = torch.where(hull != 255.0, hull + float(depth_bias(bias_mm)), hull)
        return torch.minimum(hull, head).cpu().numpy()


def write_obj(path, vertices, faces, rows=1 << 18):
    """`v` and `f` records (1-based) of a triangle mesh, written `rows` records at a time"""
    v, t = np.asarray(vertices, np.float64).reshape(-1, 3), np.asarray(faces, np.int64).reshape(-1, 3) + 1
    with open(path, "w") as f:
        for k in range(0, len(v), rows):
            f.write("".join("v %.9f %.9f %.9f\n" % (p[0], p[1], p[2]) for p in v[k:k + rows].tolist()))
        for k in range(0, len(t), rows):
            f.write("".join("f %d %d %d\n" % (q[0], q[1], q[2]) for q in t[k:k + rows].tolist()))


def load_masks(cameras, mask_path):
    """hair_mask/<view> as PMVO reads it: channel 0 of the BGR image, uint8 [H,W] per view"""
    from .pmvo_utils import _find, _imread_bgr

    return {view: np.ascontiguousarray(_imread_bgr(_find(mask_path, view))[..., 0]) for view in cameras.keys()}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m monohair_amd.haircarve", allow_abbrev=False,
                                 description="write data/<case>/ours/colmap_points.obj and render_depth/<view>.npy from the "
                                             "hair masks, the cameras and the bust; every other option (--yaml=..., --a.b=v) "
                                             "is PMVO.py's")
    ap.add_argument("--voxel-size", type=float, default=CARVE_VOXEL_SIZE, help="voxel of the carve (default 0.00125)")
    ap.add_argument("--min-free", type=int, default=2, help="views that must see the voxel past the bust (default 2)")
    ap.add_argument("--max-miss", type=int, default=0, help="of those, views that may see no hair there (default 0)")
    ap.add_argument("--depth-bias-mm", type=float, default=0.0, help="added to the hull's depth, in millimetres (default 0)")
    ap.add_argument("--force", action="store_true", help="overwrite an existing colmap_points.obj")
    own, rest = ap.parse_known_args(sys.argv[1:] if argv is None else list(argv))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import PMVO as pmvo_cli
    from .camera import load_cam, parsing_camera
    from .pmvo_utils import load_bust

    args = pmvo_cli.config_parser(rest)
    obj = args.data.raw_points_path
    if os.path.exists(obj) and not own.force:
        raise SystemExit("haircarve: %s exists -- it may be the output of instant-ngp; pass --force to overwrite it" % obj)
    camera = parsing_camera(load_cam(args.image_camera_path), os.path.join(args.data.root, "capture_images"))
    pmvo = mask_context(load_masks(camera, args.data.mask_path), camera, args.data.image_size, args.device)
    bv, bf, _ = load_bust(args.data.bust_path)
    bust = (bv + args.bust_to_origin, bf)
    vertices, faces, flags = carve(pmvo, None, bust, own.voxel_size, own.min_free, own.max_miss, voxel_min=args.bbox_min)
    depth = carve_depth(pmvo, vertices, faces, bust, own.depth_bias_mm)
    os.makedirs(os.path.dirname(obj), exist_ok=True)
    write_obj(obj, vertices.astype(np.float64) - args.bust_to_origin, faces)      # (load_colmap_points adds the offset back)
    os.makedirs(args.data.depth_path, exist_ok=True)
    for i, view in enumerate(camera.keys()):
        np.save(os.path.join(args.data.depth_path, view + ".npy"), np.repeat(depth[i][..., None], 3, axis=2))
    print("haircarve: %d INSIDE voxels of %s at %g, %d vertices, %d triangles -> %s" %
          (int(np.count_nonzero(flags)), "x".join(str(d) for d in flags.shape), own.voxel_size, len(vertices), len(faces), obj))
    print("haircarve: %d depth maps -> %s" % (len(depth), args.data.depth_path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
