"""A second carve pass by photo-consistency: the silhouette hull of haircarve lies on or outside the true surface, cannot see
concavities and reaches towards every camera; the capture's photographs (capture_images/) are the one depth cue a capture has at
that point.  Along each view's rays the candidate voxel whose neighbourhood looks most alike in the neighbouring views (census
codes of the reduced gray images, Hamming distances) is the view's winner; winners that several views agree on are confirmed;
candidates that lie in front of a confirmed winner in enough views are removed.  The refined flags go through haircarve's mesher
and depth rasteriser, so PMVO.py reads the same two inputs as before.  The reference has no counterpart: the specification is
the rule written out in include/mh_pmvo.h ("Photo-consistent carve") and restated in numpy by tests/hair_stereo_np.py; what it
gains or costs is measured, not assumed (docs/PARITY.md, f12).

    python -m monohair_amd.hairstereo --yaml=configs/reconstruct/<case> [--voxel-size 0.00125] [--min-free 2] [--max-miss 0]
                                      [--depth-bias-mm 0] [--neighbours 2] [--keep 2] [--radius 2] [--cell 0] [--max-cost 192]
                                      [--margin-vox 2] [--min-agree 2] [--min-through 2] [--force]

reads what haircarve reads and capture_images/, and writes ours/colmap_points.obj and render_depth/<view>.npy.  --cell 0 takes
auto_cell.  The kernels are csrc/hairstereo.hip.  There is no CPU path."""
import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _lib, gridviews, haircarve
from ._lib import host_ptr

MAX_NEIGHBOURS = 8
MAX_CELL = 256
# max_cost and min_agree: the pair with the best F-score at 3 mm / 30 degrees of the six measured (docs/PARITY.md f12)
DEFAULTS = dict(neighbours=2, keep=2, radius=2, cell=0, max_cost=192, margin_vox=2.0, min_agree=2, min_through=2)


# ------------------------------------------------------------------------------------------------- host-side inputs
def gray_planes(images):
    """uint8 [V,H,W]: the luma (29 B + 150 G + 77 R + 128) >> 8 of BGR images [H,W,3], the value itself of gray images [H,W];
    images: a list, or a dict in view order"""
    out = []
    for im in (images.values() if isinstance(images, dict) else images):
        a = np.asarray(im)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3):
            raise ValueError("an image is uint8 [H,W] or [H,W,3] (BGR), got %s %r" % (a.dtype, a.shape))
        if a.ndim == 3:
            b = a.astype(np.int32)
            a = ((29 * b[..., 0] + 150 * b[..., 1] + 77 * b[..., 2] + 128) >> 8).astype(np.uint8)
        out.append(a)
    if not out or any(a.shape != out[0].shape for a in out):
        raise ValueError("the images must be of one size")
    return np.ascontiguousarray(np.stack(out))


def load_gray(cameras, image_path):
    """capture_images/<view> of every camera as gray_planes takes them"""
    from .pmvo_utils import _find, _imread_bgr

    return gray_planes([_imread_bgr(_find(image_path, view)) for view in cameras.keys()])


def _records(cameras):
    from .camera import camera_records

    return np.asarray(cameras if isinstance(cameras, np.ndarray) else camera_records(cameras), np.float64)


def camera_centres(cameras):
    """float64 [V,3]: -R^-1 t of every world-to-camera pose [R | t]"""
    rec = _records(cameras)
    pose = rec[:, :16].reshape(-1, 4, 4)
    return np.stack([-np.linalg.solve(p[:3, :3], p[:3, 3]) for p in pose])


def neighbour_table(cameras, k=2):
    """int32 [V,k]: per view the k views whose camera centres are nearest, ties by view index; -1 where there are fewer"""
    k = int(k)
    if not 1 <= k <= MAX_NEIGHBOURS:
        raise ValueError("1 <= k <= %d, got %r" % (MAX_NEIGHBOURS, k))
    c = camera_centres(cameras)
    V = len(c)
    out = np.full((V, k), -1, np.int32)
    for r in range(V):
        d = ((c - c[r]) ** 2).sum(1)
        order = sorted((float(d[n]), n) for n in range(V) if n != r)[:k]
        out[r, :len(order)] = [n for _, n in order]
    return out


def auto_cell(cameras, voxel_size, voxel_min, dims, image_size):
    """The cell, in pixels, that one voxel covers: at the grid's centre c = voxel_min + (dims - 1) / 2 * voxel_size (y and z
    negated: the world point of that voxel position) a length voxel_size seen at depth d_v = -(pose_v c).z covers
    voxel_size * max(|proj_v[0,0]| * W, |proj_v[1,1]| * H) / (2 d_v) pixels in view v (ndc spans 2 over W and over H pixels);
    the cell is the maximum over the views with d_v > 0, rounded up, at least 1 and at most 256."""
    rec = _records(cameras)
    vmin, vs, dims = gridviews.grid(voxel_min, voxel_size, dims)
    H, W = int(image_size[0]), int(image_size[1])
    c = vmin + (dims.astype(np.float64) - 1.0) / 2.0 * vs
    c = np.array([c[0], -c[1], -c[2], 1.0])
    best = 0.0
    for r in rec:
        pose, proj = r[:16].reshape(4, 4), r[16:32].reshape(4, 4)
        d = -float(pose[2] @ c)
        if d > 0.0:
            best = max(best, vs * max(abs(proj[0, 0]) * W, abs(proj[1, 1]) * H) / (2.0 * d))
    return int(min(MAX_CELL, max(1, math.ceil(best - 1e-9))))


def margin255(margin_vox, voxel_size):
    """the float32 margin on the scale of the depth planes (-z_camera / 2 * 255) of a margin in voxels"""
    return np.float32(float(margin_vox) * float(voxel_size) / 2.0 * 255.0)


def _bounds(V, K, cell, radius, keep):
    cell, radius, keep = int(cell), int(radius), int(keep)
    if not 1 <= cell <= MAX_CELL:
        raise ValueError("1 <= cell <= %d, got %r" % (MAX_CELL, cell))
    if radius not in (1, 2, 3):
        raise ValueError("radius is 1, 2 or 3, got %r" % radius)
    if not 1 <= keep <= K:
        raise ValueError("1 <= keep <= the table's %d neighbours, got %r" % (K, keep))
    return cell, radius, keep


def _table(neighbours, V):
    nb = np.ascontiguousarray(neighbours.cpu().numpy() if torch.is_tensor(neighbours) else neighbours, dtype=np.int32)
    if nb.ndim != 2 or nb.shape[0] != V or not 1 <= nb.shape[1] <= MAX_NEIGHBOURS:
        raise ValueError("the neighbour table is int [V,K] with 1 <= K <= %d, got %r for %d views"
                         % (MAX_NEIGHBOURS, nb.shape, V))
    if ((nb < -1) | (nb >= V)).any() or (nb == np.arange(V)[:, None]).any():
        raise ValueError("a neighbour row holds views of [0, %d) other than its own, or -1" % V)
    return nb


# ------------------------------------------------------------------------------------------------- the stages on the device
def _census_dev(gray, cell, radius, device):
    """gray: uint8 [V,H,W] (numpy or tensor) -> (reduced uint8 [V,Hc,Wc], census int64 [V,Hc,Wc] holding the uint64 bits)"""
    g = gray if torch.is_tensor(gray) else torch.from_numpy(np.ascontiguousarray(gray, dtype=np.uint8))
    if g.dtype != torch.uint8 or g.dim() != 3:
        raise ValueError("gray is uint8 [V,H,W]")
    g = g.to(device).contiguous()
    V, H, W = (int(s) for s in g.shape)
    Hc, Wc = -(-H // cell), -(-W // cell)
    reduced = torch.empty((V, Hc, Wc), dtype=torch.uint8, device=device)
    census = torch.empty((V, Hc, Wc), dtype=torch.int64, device=device)
    _lib.check(_lib.lib().mh_stereo_census(_lib.bare_ctx(device), _lib.ptr(g), V, H, W, cell, radius, _lib.ptr(reduced),
                                           _lib.ptr(census), _lib.stream_ptr()), "mh_stereo_census")
    return reduced, census


def _candidates_dev(flags, device):
    """uint8 [n] device flags -> int32 [C] device: the indices of the non-zero ones, ascending (mh_select_rows)"""
    L, n = _lib.lib(), int(flags.numel())
    index = torch.empty(max(n, 1), dtype=torch.int32, device=device)
    count = torch.empty(1, dtype=torch.int32, device=device)
    scratch = torch.empty(int(L.mh_select_scratch_bytes(n)), dtype=torch.uint8, device=device)
    _lib.check(L.mh_select_rows(_lib.bare_ctx(device), _lib.ptr(flags), None, 0, n, None, None, None, None, _lib.ptr(index), None,
                                _lib.ptr(count), _lib.ptr(scratch), scratch.numel(), _lib.stream_ptr()), "mh_select_rows")
    return index[:int(count.cpu()[0])]


def _winners_dev(pmvo, bust, vmin, vs, dims, cand, census, nb, cell, radius, keep):
    keys = torch.empty(tuple(census.shape), dtype=torch.int64, device=pmvo.device)
    _lib.check(_lib.lib().mh_stereo_winners(pmvo._ctx, _lib.ptr(bust), host_ptr(vmin), vs, host_ptr(dims),
                                            _lib.ptr(cand) if cand.numel() else None, int(cand.numel()), _lib.ptr(census),
                                            _lib.ptr(nb), int(nb.shape[1]), cell, radius, keep, _lib.ptr(keys),
                                            _lib.stream_ptr()), "mh_stereo_winners")
    return keys


def _agree_dev(pmvo, bust, vmin, vs, dims, flags, keys, cell, max_cost, m255):
    agree = torch.empty(int(flags.numel()), dtype=torch.int32, device=pmvo.device)
    _lib.check(_lib.lib().mh_stereo_agree(pmvo._ctx, _lib.ptr(bust), host_ptr(vmin), vs, host_ptr(dims), _lib.ptr(flags),
                                          _lib.ptr(keys), cell, int(max_cost), float(m255), _lib.ptr(agree), _lib.stream_ptr()),
               "mh_stereo_agree")
    return agree


def _refine_dev(pmvo, bust, vmin, vs, dims, flags, keys, agree, cell, max_cost, m255, min_agree, min_through):
    refined = torch.empty(int(flags.numel()), dtype=torch.uint8, device=pmvo.device)
    depth = torch.empty(tuple(keys.shape), dtype=torch.float32, device=pmvo.device)
    _lib.check(_lib.lib().mh_stereo_refine(pmvo._ctx, _lib.ptr(bust), host_ptr(vmin), vs, host_ptr(dims), _lib.ptr(flags),
                                           _lib.ptr(keys), _lib.ptr(agree), cell, int(max_cost), float(m255), int(min_agree),
                                           int(min_through), _lib.ptr(refined), _lib.ptr(depth), _lib.stream_ptr()),
               "mh_stereo_refine")
    return refined, depth


def _flags_dev(flags, dims, device):
    n = int(np.prod(dims.astype(np.int64)))
    if torch.is_tensor(flags):
        f = (flags != 0).to(device=device, dtype=torch.uint8).contiguous().reshape(-1)
    else:
        f = torch.from_numpy(np.ascontiguousarray(np.asarray(flags) != 0).view(np.uint8).reshape(-1)).to(device)
    if int(f.numel()) != n:
        raise ValueError("flags hold %d voxels, the grid %d" % (int(f.numel()), n))
    return f


def _keys_dev(keys, device):
    if torch.is_tensor(keys):
        return keys.to(device=device, dtype=torch.int64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(keys, dtype=np.uint64).view(np.int64)).to(device)


class _Setup:
    """the validated arguments every stage shares"""

    def __init__(self, pmvo, bust, flags, grid_resolution, voxel_min, voxel_size, cell):
        self.vmin, self.vs, self.dims = gridviews.grid(haircarve._vmin(voxel_min), voxel_size, grid_resolution)
        self.cell = int(cell)
        if not 1 <= self.cell <= MAX_CELL:
            raise ValueError("1 <= cell <= %d, got %r" % (MAX_CELL, cell))
        self.bust = gridviews.bust_planes(pmvo, bust)
        self.flags = _flags_dev(flags, self.dims, pmvo.device)
        H, W = pmvo.image_size
        self.cells = (pmvo.num_view, -(-int(H) // self.cell), -(-int(W) // self.cell))
        self.shape = tuple(int(d) for d in self.dims)

    def keys(self, keys, device):
        k = _keys_dev(keys, device)
        if tuple(k.shape) != self.cells:
            raise ValueError("keys are [V,Hc,Wc] = %r for this cell, got %r" % (self.cells, tuple(k.shape)))
        return k


def _limits(max_cost, m255, min_agree=1, min_through=1):
    if int(max_cost) < 0 or not (math.isfinite(float(m255)) and float(m255) >= 0.0) or int(min_agree) < 1 or int(min_through) < 1:
        raise ValueError("max_cost >= 0, a finite margin >= 0, min_agree >= 1 and min_through >= 1")


# ------------------------------------------------------------------------------------------------- the stages, one by one
def stereo_census(gray, cell, radius, device="cuda:0"):
    """gray uint8 [V,H,W] -> (reduced uint8 [V,Hc,Wc], census uint64 [V,Hc,Wc]) as numpy"""
    cell, radius, _ = _bounds(1, 1, cell, radius, 1)
    with torch.cuda.device(device):
        g, c = _census_dev(gray, cell, radius, torch.device(device))
        return g.cpu().numpy(), c.cpu().numpy().view(np.uint64)


def stereo_winners(pmvo, bust, flags, gray, neighbours, grid_resolution, voxel_min=None, voxel_size=haircarve.CARVE_VOXEL_SIZE,
                   cell=1, radius=2, keep=2):
    """The winner key of every (view, cell) over the candidates `flags` ([X,Y,Z], non-zero = candidate).  -> uint64 [V,Hc,Wc]:
    (cost << 32) | linear voxel index, all ones where no candidate has a cost."""
    nb = _table(neighbours, pmvo.num_view)
    cell, radius, keep = _bounds(pmvo.num_view, nb.shape[1], cell, radius, keep)
    with torch.cuda.device(pmvo.device):
        s = _Setup(pmvo, bust, flags, grid_resolution, voxel_min, voxel_size, cell)
        _, census = _census_dev(gray, cell, radius, pmvo.device)
        if tuple(census.shape) != s.cells:
            raise ValueError("gray is %r, the views are %r" % (tuple(gray.shape), (pmvo.num_view,) + tuple(pmvo.image_size)))
        keys = _winners_dev(pmvo, s.bust, s.vmin, s.vs, s.dims, _candidates_dev(s.flags, pmvo.device), census,
                            torch.from_numpy(nb).to(pmvo.device), cell, radius, keep)
        return keys.cpu().numpy().view(np.uint64)


def stereo_agree(pmvo, bust, flags, keys, grid_resolution, voxel_min=None, voxel_size=haircarve.CARVE_VOXEL_SIZE, cell=1,
                 max_cost=192, m255=0.0):
    """-> int32 [X,Y,Z]: per candidate the views that take part in it and whose winner of its cell lies within m255 of it"""
    _limits(max_cost, m255)
    with torch.cuda.device(pmvo.device):
        s = _Setup(pmvo, bust, flags, grid_resolution, voxel_min, voxel_size, cell)
        a = _agree_dev(pmvo, s.bust, s.vmin, s.vs, s.dims, s.flags, s.keys(keys, pmvo.device), s.cell, max_cost, m255)
        return a.cpu().numpy().reshape(s.shape)


def stereo_refine(pmvo, bust, flags, keys, agree, grid_resolution, voxel_min=None, voxel_size=haircarve.CARVE_VOXEL_SIZE,
                  cell=1, max_cost=192, m255=0.0, min_agree=2, min_through=2):
    """-> (refined uint8 [X,Y,Z], depth float32 [V,Hc,Wc]): the candidates that lie in front of a confirmed winner in fewer
    than min_through views; the depth of each cell's confirmed winner, 255 where there is none"""
    _limits(max_cost, m255, min_agree, min_through)
    with torch.cuda.device(pmvo.device):
        s = _Setup(pmvo, bust, flags, grid_resolution, voxel_min, voxel_size, cell)
        a = agree if torch.is_tensor(agree) else torch.from_numpy(np.ascontiguousarray(agree, dtype=np.int32))
        a = a.to(device=pmvo.device, dtype=torch.int32).contiguous().reshape(-1)
        if int(a.numel()) != int(s.flags.numel()):
            raise ValueError("agree holds %d voxels, the grid %d" % (int(a.numel()), int(s.flags.numel())))
        r, d = _refine_dev(pmvo, s.bust, s.vmin, s.vs, s.dims, s.flags, s.keys(keys, pmvo.device), a, s.cell, max_cost, m255,
                           min_agree, min_through)
        return r.cpu().numpy().reshape(s.shape), d.cpu().numpy()


# ------------------------------------------------------------------------------------------------- the pieces together
def _stereo_dev(pmvo, bust, flags, gray, nb, vmin, vs, dims, cell, radius, keep, max_cost, m255, min_agree, min_through):
    """every stage on device tensors -> (refined uint8 [X*Y*Z], depth float32 [V,Hc,Wc], keys, agree)"""
    _, census = _census_dev(gray, cell, radius, pmvo.device)
    keys = _winners_dev(pmvo, bust, vmin, vs, dims, _candidates_dev(flags, pmvo.device), census, nb, cell, radius, keep)
    agree = _agree_dev(pmvo, bust, vmin, vs, dims, flags, keys, cell, max_cost, m255)
    refined, depth = _refine_dev(pmvo, bust, vmin, vs, dims, flags, keys, agree, cell, max_cost, m255, min_agree, min_through)
    return refined, depth, keys, agree


def stereo(pmvo_or_masks, cameras, gray, bust, flags, voxel_size=haircarve.CARVE_VOXEL_SIZE, voxel_min=None, neighbours=2,
           keep=2, radius=2, cell=0, max_cost=192, margin_vox=2.0, min_agree=2, min_through=2, image_size=None, device="cuda:0"):
    """The refinement of candidate flags [X,Y,Z] (the grid is their shape).  pmvo_or_masks, cameras and bust as for
    haircarve.carve; gray: uint8 [V,H,W] (gray_planes); neighbours: a number (neighbour_table of the cameras) or a table
    [V,K]; cell 0: auto_cell.  -> (refined uint8 [X,Y,Z], depth float32 [V,Hc,Wc])."""
    pmvo = pmvo_or_masks if hasattr(pmvo_or_masks, "_ctx") else haircarve.mask_context(pmvo_or_masks, cameras, image_size, device)
    cams = cameras if cameras is not None else pmvo.camera_dict
    shape = tuple(flags.shape)
    if len(shape) != 3:
        raise ValueError("flags are [X,Y,Z], got shape %r" % (shape,))
    vmin, vs, dims = gridviews.grid(haircarve._vmin(voxel_min), voxel_size, shape)
    if np.ndim(neighbours) == 0:
        if cams is None:
            raise ValueError("a number of neighbours needs the cameras: pass them, or a table")
        neighbours = neighbour_table(cams, neighbours)
    nb = _table(neighbours, pmvo.num_view)
    if int(cell) == 0:
        if cams is None:
            raise ValueError("cell 0 needs the cameras: pass them, or a cell")
        cell = auto_cell(cams, vs, vmin, dims, pmvo.image_size)
    cell, radius, keep = _bounds(pmvo.num_view, nb.shape[1], cell, radius, keep)
    m255 = margin255(margin_vox, vs)
    _limits(max_cost, m255, min_agree, min_through)
    with torch.cuda.device(pmvo.device):
        s = _Setup(pmvo, bust, flags, shape, vmin, vs, cell)
        refined, depth, _, _ = _stereo_dev(pmvo, s.bust, s.flags, gray, torch.from_numpy(nb).to(pmvo.device), vmin, vs, dims,
                                           cell, radius, keep, max_cost, m255, min_agree, min_through)
        return refined.cpu().numpy().reshape(shape), depth.cpu().numpy()


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m monohair_amd.hairstereo", allow_abbrev=False,
                                 description="write data/<case>/ours/colmap_points.obj and render_depth/<view>.npy from the "
                                             "hair masks, the cameras, the bust and the photographs; every other option "
                                             "(--yaml=..., --a.b=v) is PMVO.py's")
    ap.add_argument("--voxel-size", type=float, default=haircarve.CARVE_VOXEL_SIZE, help="voxel of the carve (default 0.00125)")
    ap.add_argument("--min-free", type=int, default=2, help="views that must see the voxel past the bust (default 2)")
    ap.add_argument("--max-miss", type=int, default=0, help="of those, views that may see no hair there (default 0)")
    ap.add_argument("--depth-bias-mm", type=float, default=0.0, help="added to the hull's depth, in millimetres (default 0)")
    ap.add_argument("--neighbours", type=int, default=DEFAULTS["neighbours"], help="neighbour views per view (default 2)")
    ap.add_argument("--keep", type=int, default=DEFAULTS["keep"], help="of those, the best that make the cost (default 2)")
    ap.add_argument("--radius", type=int, default=DEFAULTS["radius"], help="census window radius in cells, 1..3 (default 2)")
    ap.add_argument("--cell", type=int, default=DEFAULTS["cell"], help="pixels per cell; 0 = one voxel's size (default 0)")
    ap.add_argument("--max-cost", type=int, default=DEFAULTS["max_cost"], help="largest cost of a winner, of 1024 (default 192)")
    ap.add_argument("--margin-vox", type=float, default=DEFAULTS["margin_vox"], help="depth margin in voxels (default 2)")
    ap.add_argument("--min-agree", type=int, default=DEFAULTS["min_agree"], help="views that confirm a winner (default 2)")
    ap.add_argument("--min-through", type=int, default=DEFAULTS["min_through"],
                    help="views in which a voxel lies in front of a confirmed winner before it goes (default 2)")
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
        raise SystemExit("hairstereo: %s exists -- it may be the output of instant-ngp; pass --force to overwrite it" % obj)
    images = os.path.join(args.data.root, "capture_images")
    camera = parsing_camera(load_cam(args.image_camera_path), images)
    pmvo = haircarve.mask_context(haircarve.load_masks(camera, args.data.mask_path), camera, args.data.image_size, args.device)
    gray = load_gray(camera, images)
    bv, bf, _ = load_bust(args.data.bust_path)
    bust = (bv + args.bust_to_origin, bf)
    grid = haircarve.carve_grid(own.voxel_size)
    vmin, vs, dims = gridviews.grid(args.bbox_min, own.voxel_size, grid)
    min_free, max_miss = haircarve._limits(own.min_free, own.max_miss)
    nb = neighbour_table(camera, own.neighbours)
    cell = own.cell if own.cell else auto_cell(camera, vs, vmin, dims, pmvo.image_size)
    cell, radius, keep = _bounds(pmvo.num_view, nb.shape[1], cell, own.radius, own.keep)
    m255 = margin255(own.margin_vox, vs)
    _limits(own.max_cost, m255, own.min_agree, own.min_through)
    with torch.cuda.device(pmvo.device):
        planes = gridviews.bust_planes(pmvo, bust)
        hull = haircarve._inside_dev(pmvo, planes, vmin, vs, dims, min_free, max_miss)
        refined, depth_cells, _, _ = _stereo_dev(pmvo, planes, hull, gray, torch.from_numpy(nb).to(pmvo.device), vmin, vs, dims,
                                                 cell, radius, keep, own.max_cost, m255, own.min_agree, own.min_through)
        n_hull, n_refined = int(hull.sum(dtype=torch.int64).item()), int(refined.sum(dtype=torch.int64).item())
        n_confirmed, n_cells = int((depth_cells != 255.0).sum().item()), int(depth_cells.numel())
        v, t = haircarve._mesh_dev(refined, vmin, vs, dims, pmvo.device)
        vertices, faces = v.cpu().numpy(), t.cpu().numpy()
    depth = haircarve.carve_depth(pmvo, vertices, faces, bust, own.depth_bias_mm)
    os.makedirs(os.path.dirname(obj), exist_ok=True)
    haircarve.write_obj(obj, vertices.astype(np.float64) - args.bust_to_origin, faces)
    os.makedirs(args.data.depth_path, exist_ok=True)
    for i, view in enumerate(camera.keys()):
        np.save(os.path.join(args.data.depth_path, view + ".npy"), np.repeat(depth[i][..., None], 3, axis=2))
    print("hairstereo: %d INSIDE voxels of %s at %g, cell %d: the refinement removed %d, %d remain; %d of %d cells have a "
          "confirmed winner" % (n_hull, "x".join(str(int(d)) for d in dims), own.voxel_size, cell, n_hull - n_refined, n_refined,
                                n_confirmed, n_cells))
    print("hairstereo: %d vertices, %d triangles -> %s; %d depth maps -> %s" % (len(vertices), len(faces), obj, len(depth),
                                                                              args.data.depth_path))
    return 0


if __name__ == "__main__":
    sys.exit(main())
