"""The hair interior filled without the network: a classical stand-in for DeepMVSHair's `ours/raw.npy`, which the second PMVO
pass merges into the `full/` volume (PMVO.py:733-751).  Two steps: the voxels that lie inside the hair, outside the head and are
seen by almost no view (integer votes of every voxel centre over the views, against the depth maps, a depth plane of the bust
alone and the hair masks), and the exterior volume's orientations carried inward to them (direction tensors averaged over the
six face neighbours for a given number of sweeps, then the principal axis per voxel).  The reference has no counterpart, so the
specification is the rule written out in include/mh_pmvo.h ("Inner fill") and restated in numpy by tests/hair_fill_np.py:
float32 comparisons as the vote kernels make them, float64 + and / in a fixed order.

    python -m monohair_amd.hairfill --yaml=configs/reconstruct/<case> [--name=...] [--sweeps 64] [--min-coh 0] [--max-bad 0] [--force]

reads output/<name>/refine/{Occ3D,Ori3D}.mat and the maps PMVO.py reads, draws the bust per view, and writes
data/<case>/ours/raw.npy; `python infer_inner.py --yaml=... --infer_inner.render_data=` and `python HairGrow.py --yaml=...
--PMVO.infer_inner` then run as they do on a network's output.  The kernels are csrc/hairfill.hip.  There is no CPU path."""
import argparse
import math
import os
import sys

import numpy as np
import torch

from . import _lib, gridviews
from ._lib import host_ptr
from .hairvolume import load_side
from .pmvo_utils import GRID_RESOLUTION, VOXEL_MIN, VOXEL_SIZE
from .timing import stage

MAX_SWEEPS = 1024


def _voxel_list(voxels):
    v = np.ascontiguousarray(np.asarray(voxels, dtype=np.int64).reshape(-1, 3))
    if v.shape[0] >= 1 << 31:
        raise ValueError("more than 2^31 - 1 voxels")
    return v


# ------------------------------------------------------------------------------------------------- 1. domain votes
def _votes_dev(pmvo, bust, vmin, vs, dims):
    nvox = int(np.prod(dims.astype(np.int64)))
    counts = torch.empty((nvox, 4), dtype=torch.int32, device=pmvo.device)
    _lib.check(_lib.lib().mh_inner_votes(pmvo._ctx, _lib.ptr(bust), host_ptr(vmin), vs, host_ptr(dims), _lib.ptr(counts),
                                         _lib.stream_ptr()), "mh_inner_votes")
    return counts


def inner_votes(pmvo, bust_planes, grid_resolution=GRID_RESOLUTION, voxel_min=VOXEL_MIN, voxel_size=VOXEL_SIZE):
    """The four vote counts of every voxel centre over the views of `pmvo` (a PMVO object of fp32 planes or 8-bit codes).
    bust_planes: float32 [V,H,W], the depth of the bust alone in PMVO's convention, 255 where there is none (or (vertices,
    faces), drawn here).  -> int32 [X,Y,Z,4] = n_in, n_vis, n_front, n_bad."""
    vmin, vs, dims = gridviews.grid(voxel_min, voxel_size, grid_resolution)
    with torch.cuda.device(pmvo.device):
        counts = _votes_dev(pmvo, gridviews.bust_planes(pmvo, bust_planes), vmin, vs, dims)
        return counts.cpu().numpy().reshape(int(dims[0]), int(dims[1]), int(dims[2]), 4)


def _domain_dev(pmvo, counts, ext_voxels, dims, max_bad):
    """-> (domain voxels int64 [D,3] on the device, ascending by (x*Y + y)*Z + z)"""
    L, device, st = _lib.lib(), pmvo.device, _lib.stream_ptr()
    nvox = int(np.prod(dims.astype(np.int64)))
    max_bad = int(max_bad)
    if max_bad < 0:
        raise ValueError("max_bad must be >= 0, got %r" % max_bad)
    ext_index = None
    ext = _voxel_list(ext_voxels if ext_voxels is not None else np.zeros((0, 3), np.int64))
    if ext.shape[0]:
        ev = torch.from_numpy(ext).to(device)
        ext_index = torch.empty(nvox, dtype=torch.int32, device=device)
        status = torch.empty(2, dtype=torch.int32, device=device)
        _lib.check(L.mh_volume_index(pmvo._ctx, _lib.ptr(ev), ext.shape[0], host_ptr(dims), _lib.ptr(ext_index),
                                     _lib.ptr(status), st), "mh_volume_index")
        outside, twice = (int(s) for s in status.cpu().numpy())
        if outside or twice:
            raise ValueError("the exterior voxels must be unique and inside the grid: %d outside, %d listed again"
                             % (outside, twice))
    flags = torch.empty(nvox, dtype=torch.uint8, device=device)
    _lib.check(L.mh_inner_domain(pmvo._ctx, _lib.ptr(counts), _lib.ptr(ext_index), host_ptr(dims), max_bad, _lib.ptr(flags), st),
               "mh_inner_domain")
    index = torch.empty(nvox, dtype=torch.int32, device=device)
    count = torch.empty(1, dtype=torch.int32, device=device)
    scratch = torch.empty(int(L.mh_select_scratch_bytes(nvox)), dtype=torch.uint8, device=device)
    _lib.check(L.mh_select_rows(pmvo._ctx, _lib.ptr(flags), None, 0, nvox, None, None, None, None, _lib.ptr(index), None,
                                _lib.ptr(count), _lib.ptr(scratch), scratch.numel(), st), "mh_select_rows")
    D = int(count.cpu()[0])
    lin = index[:D].to(torch.int64)
    Y, Z = int(dims[1]), int(dims[2])
    return torch.stack([lin // (Y * Z), (lin // Z) % Y, lin % Z], 1).contiguous()      # (index arithmetic on integers)


def inner_domain(pmvo, bust_planes, ext_voxels=None, grid_resolution=GRID_RESOLUTION, voxel_min=VOXEL_MIN,
                 voxel_size=VOXEL_SIZE, max_bad=0):
    """The voxels to fill: n_in >= 1, n_vis <= 2, n_front >= 1, n_bad <= max_bad and not one of ext_voxels (int [G,3], unique,
    inside the grid).  -> int64 [D,3] (x, y, z) ascending by (x*Y + y)*Z + z."""
    vmin, vs, dims = gridviews.grid(voxel_min, voxel_size, grid_resolution)
    with torch.cuda.device(pmvo.device):
        bust = gridviews.bust_planes(pmvo, bust_planes)
        with stage("hairfill: votes", pmvo.device):
            counts = _votes_dev(pmvo, bust, vmin, vs, dims)
        with stage("hairfill: domain", pmvo.device):
            return _domain_dev(pmvo, counts, ext_voxels, dims, max_bad).cpu().numpy()


# ------------------------------------------------------------------------------------------------- 2. sweeps, 3. resolve
def diffuse_orientation(ext_voxels, ext_ori, domain_voxels, grid_resolution=GRID_RESOLUTION, sweeps=64, min_coh=0.0,
                        return_details=False, voxel_min=VOXEL_MIN, voxel_size=VOXEL_SIZE, device="cuda:0"):
    """The exterior's orientations carried to the domain rows: `sweeps` (0..1024) Jacobi sweeps over the six face neighbours,
    then the principal axis of every known row.  ext_voxels int [G,3] with ext_ori float32 [G,3]; domain_voxels int [D,3] in any
    order (the result follows it); the two lists unique, inside the grid and disjoint.  -> float32 [M,7] = world centre,
    direction, 1.0 of the emitted rows (known, trace > 0, coh >= min_coh) in domain order; with return_details also a dict of
    tensor float64 [D,6], known uint8 [D], depth int32 [D], coh float64 [D], ori float32 [D,3], world float32 [D,3], emit
    uint8 [D], ext_tensor float64 [G,6], ext_source uint8 [G]."""
    vmin, vs, dims = gridviews.grid(voxel_min, voxel_size, grid_resolution)
    ev, dv = _voxel_list(ext_voxels), _voxel_list(domain_voxels)
    eo = np.ascontiguousarray(np.asarray(ext_ori, dtype=np.float32).reshape(-1, 3))
    if ev.shape[0] != eo.shape[0]:
        raise ValueError("%d exterior voxels, %d directions" % (ev.shape[0], eo.shape[0]))
    sweeps, min_coh = int(sweeps), float(min_coh)
    if not 0 <= sweeps <= MAX_SWEEPS:
        raise ValueError("sweeps must be 0..%d, got %r" % (MAX_SWEEPS, sweeps))
    if math.isnan(min_coh):
        raise ValueError("min_coh is NaN")
    G, D = int(ev.shape[0]), int(dv.shape[0])
    nvox = int(np.prod(dims.astype(np.int64)))
    L = _lib.lib()
    with torch.cuda.device(device):
        ctx, st = _lib.bare_ctx(device), _lib.stream_ptr()
        evd, eod, dvd = (torch.from_numpy(a).to(device) for a in (ev, eo, dv))
        vmap = torch.empty(nvox, dtype=torch.int32, device=device)
        ext_t = torch.empty((G, 6), dtype=torch.float64, device=device)
        ext_s = torch.empty(G, dtype=torch.uint8, device=device)
        cell = torch.empty(D, dtype=torch.int32, device=device)
        t_a, t_b = (torch.empty((D, 6), dtype=torch.float64, device=device) for _ in range(2))
        k_a, k_b = (torch.empty(D, dtype=torch.uint8, device=device) for _ in range(2))
        depth = torch.empty(D, dtype=torch.int32, device=device)
        status = torch.empty(2, dtype=torch.int32, device=device)
        with stage("hairfill: sweeps", device):
            _lib.check(L.mh_inner_diffuse(ctx, _lib.ptr(evd), _lib.ptr(eod), G, _lib.ptr(dvd), D, host_ptr(dims), sweeps,
                                          _lib.ptr(vmap), _lib.ptr(ext_t), _lib.ptr(ext_s), _lib.ptr(cell), _lib.ptr(t_a),
                                          _lib.ptr(t_b), _lib.ptr(k_a), _lib.ptr(k_b), _lib.ptr(depth), _lib.ptr(status), st),
                       "mh_inner_diffuse")
        outside, twice = (int(s) for s in status.cpu().numpy())
        if outside or twice:
            raise ValueError("the exterior and domain voxels must be unique, disjoint and inside the grid: %d voxels outside, "
                             "%d cells listed again" % (outside, twice))
        world, ori = (torch.empty((D, 3), dtype=torch.float32, device=device) for _ in range(2))
        coh = torch.empty(D, dtype=torch.float64, device=device)
        emit = torch.empty(D, dtype=torch.uint8, device=device)
        _lib.check(L.mh_inner_resolve(ctx, _lib.ptr(dvd), D, _lib.ptr(t_a), _lib.ptr(k_a), host_ptr(vmin), vs, host_ptr(dims),
                                      min_coh, _lib.ptr(world), _lib.ptr(ori), _lib.ptr(coh), _lib.ptr(emit), st),
                   "mh_inner_resolve")
        w_out, o_out = (torch.empty((D, 3), dtype=torch.float32, device=device) for _ in range(2))
        count = torch.zeros(1, dtype=torch.int32, device=device)
        if D:
            scratch = torch.empty(int(L.mh_select_scratch_bytes(D)), dtype=torch.uint8, device=device)
            _lib.check(L.mh_select_rows(ctx, _lib.ptr(emit), None, 0, D, _lib.ptr(world), _lib.ptr(ori), _lib.ptr(w_out),
                                        _lib.ptr(o_out), None, None, _lib.ptr(count), _lib.ptr(scratch), scratch.numel(), st),
                       "mh_select_rows")
        M = int(count.cpu()[0])
        rows = np.ones((M, 7), np.float32)
        rows[:, 0:3] = w_out[:M].cpu().numpy()
        rows[:, 3:6] = o_out[:M].cpu().numpy()
        if not return_details:
            return rows
        details = {"tensor": t_a, "known": k_a, "depth": depth, "coh": coh, "ori": ori, "world": world, "emit": emit,
                   "ext_tensor": ext_t, "ext_source": ext_s}
        return rows, {k: v.cpu().numpy() for k, v in details.items()}


def fill_inner(pmvo, bust, ext_volume, sweeps=64, min_coh=0.0, max_bad=0, voxel_min=VOXEL_MIN, voxel_size=VOXEL_SIZE,
               return_details=False):
    """The rows of raw.npy for the views of `pmvo`: the domain of inner_domain against the exterior volume, filled by
    diffuse_orientation.  bust: float32 [V,H,W] planes of the bust alone, or (vertices, faces) in world coordinates;
    ext_volume: a directory of Occ3D.mat / Ori3D.mat, or (grid_resolution, voxels, ori).  -> float32 [M,7]; with
    return_details also a dict: diffuse_orientation's, and domain int64 [D,3]."""
    grid, ev, eo = load_side(ext_volume)
    domain = inner_domain(pmvo, bust, ev, grid, voxel_min, voxel_size, max_bad)
    rows, details = diffuse_orientation(ev, eo, domain, grid, sweeps, min_coh, True, voxel_min, voxel_size, pmvo.device)
    if not return_details:
        return rows
    details["domain"] = domain
    return rows, details


def depth_histogram(depth):
    """{sweep at which a row became known: rows}, 0 = never reached"""
    values, counts = np.unique(np.asarray(depth, dtype=np.int64), return_counts=True)
    return {int(v): int(c) for v, c in zip(values, counts)}


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m monohair_amd.hairfill", allow_abbrev=False,
                                 description="write data/<case>/ours/raw.npy from the exterior volume of refine; every other "
                                             "option (--yaml=..., --name=..., --a.b=v) is PMVO.py's")
    ap.add_argument("--sweeps", type=int, default=64, help="Jacobi sweeps, 0..%d (default 64)" % MAX_SWEEPS)
    ap.add_argument("--min-coh", type=float, default=0.0, help="rows below this coherence are not written (default 0)")
    ap.add_argument("--max-bad", type=int, default=0,
                    help="views in which a voxel may lie in front of the bust on a pixel that is not hair (default 0)")
    ap.add_argument("--force", action="store_true", help="overwrite an existing raw.npy")
    own, rest = ap.parse_known_args(sys.argv[1:] if argv is None else list(argv))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    import PMVO as pmvo_cli
    from .camera import load_cam, parsing_camera
    from .pmvo_utils import load_bust

    args = pmvo_cli.config_parser(rest)
    raw = os.path.join(args.data.root, "ours", "raw.npy")
    if os.path.exists(raw) and not own.force:
        raise SystemExit("hairfill: %s exists -- it may be the output of DeepMVSHair; pass --force to overwrite it" % raw)
    refine = os.path.join(args.output_path, "refine")
    for f in ("Occ3D.mat", "Ori3D.mat"):
        if not os.path.exists(os.path.join(refine, f)):
            raise SystemExit("hairfill: %s is missing -- run PMVO.py first" % os.path.join(refine, f))
    camera = parsing_camera(load_cam(args.image_camera_path), os.path.join(args.data.root, "capture_images"))
    pmvo = pmvo_cli.load_views(camera, args)
    vertices, faces, _ = load_bust(args.data.bust_path)
    rows, details = fill_inner(pmvo, (vertices + args.bust_to_origin, faces), refine, own.sweeps, own.min_coh, own.max_bad,
                               return_details=True)
    os.makedirs(os.path.dirname(raw), exist_ok=True)
    np.save(raw, rows)
    print("hairfill: %d domain voxels, %d rows written -> %s" % (len(details["domain"]), len(rows), raw))
    print("hairfill: rows by the sweep that reached them (0 = never): %s" % depth_histogram(details["depth"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
