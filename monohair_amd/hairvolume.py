"""The inverse of HairGrow and a score one level below hairmetrics: a strand set turned into the volume the fit of refine
would ideally produce (occupied voxels with one direction each, in PMVO's voxel conventions and file layout), and one sparse
volume scored against another (precision / recall / F-score of the voxels under a Chebyshev reach and a direction bound).
The reference has no counterpart -- its get_ground_truth_3D_occ / _ori only read such volumes and its OccMetric
(Utils/Utils.py:336-363) is training code the pipeline never calls -- so the specification is the one written out in
include/mh_pmvo.h ("Strand volume", "Volume scores") and restated in numpy by tests/hair_volume_np.py: float64 arithmetic on
float32 values, + - * / sqrt in a fixed order, integer per-voxel sums.

    python -m monohair_amd.hairvolume voxelize STRANDS.hair --out DIR [--bust_to_origin x y z] [--grid X Y Z] [--vsize v] [--sub k]
    python -m monohair_amd.hairvolume score PRED_DIR GT_DIR [--thresholds 0:-,1:-,1:30,1:20,1:10] [--json OUT]

`voxelize` writes DIR/Occ3D.mat and DIR/Ori3D.mat, what `python HairGrow.py --name=...` reads.  The kernels are
csrc/hairvolume.hip.  There is no CPU path."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import _lib
from ._lib import host_ptr
from .hairmetrics import flag_counts, scores_from_counts
from .pmvo_utils import (GRID_RESOLUTION, VOXEL_MIN, VOXEL_SIZE, get_ground_truth_3D_occ, get_ground_truth_3D_ori,
                         save_ori_occ_mat_sparse)
from .strandset import StrandSet, load

DEFAULT_THRESHOLDS = ((0, None), (1, None), (1, 30.0), (1, 20.0), (1, 10.0))   # (reach in voxels, degrees or None)
MAX_PAIRS = 8          # one bit of the flag byte each
MAX_REACH = 4
MAX_COUNT = 1 << 29    # samples of one voxel: up to here its six sums convert to float64 exactly


def grid_dims3(grid_resolution):
    """int32 [3] = (X, Y, Z): three positive sizes with fewer than 2^31 voxels"""
    g = np.ascontiguousarray(np.asarray(grid_resolution).reshape(-1), dtype=np.int64)
    if g.shape != (3,) or (g < 1).any() or int(np.prod(g)) >= 1 << 31:
        raise ValueError("grid_resolution %r: three positive sizes with fewer than 2^31 voxels" % (grid_resolution,))
    return g.astype(np.int32)


# ------------------------------------------------------------------------------------------------- strands -> volume
def voxelize_strands(strands, bust_to_origin=(0.0, 0.0, 0.0), voxel_min=VOXEL_MIN, voxel_size=VOXEL_SIZE,
                     grid_resolution=GRID_RESOLUTION, sub=2, device="cuda:0", return_details=False):
    """strands: a `.hair` path or (counts, points [n,3] in `.hair` coordinates = world minus bust_to_origin).  -> dict:
    voxels int64 [G,3] (x,y,z) ascending by (x*Y + y)*Z + z, ori float32 [G,3] (world directions, y <= 0), cnt int32 [G],
    coh float64 [G], dropped_segments, outside_samples, samples (the kept ones), grid_resolution; with return_details also
    sums int64 [G,6] (xx, yy, zz, xy, xz, yz of the quantised directions)."""
    strands = load(strands)
    sub = int(sub)
    if not 1 <= sub <= 16:
        raise ValueError("sub must be 1..16, got %r" % sub)
    bust = np.ascontiguousarray(np.asarray(bust_to_origin, dtype=np.float64).reshape(-1))
    vmin = np.ascontiguousarray(np.asarray(voxel_min, dtype=np.float64).reshape(-1))
    vs = float(voxel_size)
    if bust.shape != (3,) or vmin.shape != (3,) or not (np.isfinite(bust).all() and np.isfinite(vmin).all()
                                                         and vs > 0.0 and math.isfinite(vs)):
        raise ValueError("bust_to_origin and voxel_min are three finite numbers, voxel_size a positive one")
    dims = grid_dims3(grid_resolution)
    nvox = int(np.prod(dims.astype(np.int64)))
    L = _lib.lib()
    with torch.cuda.device(device):
        ctx, st = _lib.bare_ctx(device), _lib.stream_ptr()
        s = StrandSet(strands, device)
        S = s.S
        acc = torch.empty((nvox, 8), dtype=torch.int64, device=device)
        occ = torch.empty(nvox, dtype=torch.uint8, device=device)
        counters = torch.empty(2, dtype=torch.int64, device=device)
        _lib.check(L.mh_strand_volume_accumulate(ctx, _lib.ptr(s.points), _lib.ptr(s.offsets), S, s.n, host_ptr(bust), host_ptr(vmin), vs,
                                                 host_ptr(dims), sub, _lib.ptr(acc), _lib.ptr(occ), _lib.ptr(counters), st),
                   "mh_strand_volume_accumulate")
        index = torch.empty(nvox, dtype=torch.int32, device=device)
        count = torch.empty(1, dtype=torch.int32, device=device)
        scratch = torch.empty(int(L.mh_select_scratch_bytes(nvox)), dtype=torch.uint8, device=device)
        _lib.check(L.mh_select_rows(ctx, _lib.ptr(occ), None, 0, nvox, None, None, None, None, _lib.ptr(index), None,
                                    _lib.ptr(count), _lib.ptr(scratch), scratch.numel(), st), "mh_select_rows")
        G = int(count.cpu()[0])                                       # (the one synchronisation)
        dropped, outside = (int(v) for v in counters.cpu().numpy())
        voxels = torch.empty((G, 3), dtype=torch.int64, device=device)
        ori = torch.empty((G, 3), dtype=torch.float32, device=device)
        cnt = torch.empty(G, dtype=torch.int32, device=device)
        coh = torch.empty(G, dtype=torch.float64, device=device)
        sums = torch.empty((G, 6), dtype=torch.int64, device=device) if return_details else None
        refused = torch.empty(1, dtype=torch.int32, device=device)
        _lib.check(L.mh_strand_volume_resolve(ctx, _lib.ptr(acc), _lib.ptr(index), G, host_ptr(dims), _lib.ptr(voxels),
                                              _lib.ptr(ori), _lib.ptr(cnt), _lib.ptr(coh), _lib.ptr(sums), _lib.ptr(refused),
                                              st), "mh_strand_volume_resolve")
        if int(refused.cpu()[0]):
            raise ValueError("%d voxels hold more than 2^29 samples: their sums would not convert to float64 exactly"
                             % int(refused.cpu()[0]))
        out = {"voxels": voxels.cpu().numpy(), "ori": ori.cpu().numpy(), "cnt": cnt.cpu().numpy(), "coh": coh.cpu().numpy(),
               "dropped_segments": dropped, "outside_samples": outside, "samples": int(cnt.sum(dtype=torch.int64).cpu()),
               "strands": S, "grid_resolution": [int(v) for v in dims]}
        if return_details:
            out["sums"] = sums.cpu().numpy()
    return out


def write_volume(dir, grid_resolution, voxels, ori):
    """Occ3D.mat / Ori3D.mat under `dir`, byte for byte the layout PMVO writes (save_ori_occ_mat_sparse)."""
    os.makedirs(dir, exist_ok=True)
    save_ori_occ_mat_sparse(dir, grid_dims3(grid_resolution), voxels, ori)


def load_volume(dir):
    """-> (grid_resolution int32 [3] = (X,Y,Z), voxels int64 [G,3] (x,y,z) ascending by (x*Y + y)*Z + z, ori float32 [G,3]) of
    dir/Occ3D.mat and dir/Ori3D.mat, read by the readers HairGrow uses; a voxel is occupied where Occ > 0."""
    occ = get_ground_truth_3D_occ(os.path.join(dir, "Occ3D.mat"))[..., 0]      # [Z,Y,X]
    ori = get_ground_truth_3D_ori(os.path.join(dir, "Ori3D.mat"))              # [Z,Y,X,3]
    Z, Y, X = occ.shape
    if ori.shape != (Z, Y, X, 3):
        raise ValueError("Ori3D.mat %r does not belong to Occ3D.mat %r" % (ori.shape, occ.shape))
    x, y, z = np.nonzero(np.ascontiguousarray(occ.transpose(2, 1, 0)) > 0)      # [X,Y,Z]: C order = ascending key
    voxels = np.stack([x, y, z], 1).astype(np.int64).reshape(-1, 3)
    return np.array([X, Y, Z], np.int32), voxels, np.ascontiguousarray(ori[z, y, x]).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------- volume against volume
def parse_thresholds(text):
    """'0:-,1:30' -> ((0, None), (1, 30.0)): REACH:ANGLE in voxels and degrees, '-' for no direction test"""
    pairs = []
    for item in text.split(","):
        r, sep, a = item.partition(":")
        if not sep:
            raise ValueError("threshold %r is not REACH:ANGLE" % item)
        pairs.append((int(r), None if a.strip() == "-" else float(a)))
    return _check_thresholds(pairs)


def _check_thresholds(pairs):
    pairs = tuple((int(r), None if a is None else float(a)) for r, a in pairs)
    if not 1 <= len(pairs) <= MAX_PAIRS:
        raise ValueError("between 1 and %d threshold pairs, got %d" % (MAX_PAIRS, len(pairs)))
    for r, a in pairs:
        if not (0 <= r <= MAX_REACH and (a is None or 0.0 <= a <= 90.0)):
            raise ValueError("threshold (%r voxels, %r deg): the reach must be 0..%d, the angle within [0, 90] or None"
                             % (r, a, MAX_REACH))
    return pairs


def threshold_bounds(thresholds):
    """What the kernel compares against: (reach, cos2) with cos2 = c * c, c = cos(angle * (pi / 180)); -1 for no angle."""
    cos2 = []
    for _, a in thresholds:
        c = -1.0 if a is None else math.cos(float(a) * (math.pi / 180.0))
        cos2.append(-1.0 if a is None else c * c)
    return [int(r) for r, _ in thresholds], cos2


class _Volume:
    """One side of a comparison on the device: the voxel list, its directions and its dense index volume."""

    def __init__(self, voxels, ori, dims, device):
        v = np.ascontiguousarray(np.asarray(voxels, dtype=np.int64).reshape(-1, 3))
        o = np.ascontiguousarray(np.asarray(ori, dtype=np.float32).reshape(-1, 3))
        if v.shape[0] != o.shape[0]:
            raise ValueError("%d voxels, %d directions" % (v.shape[0], o.shape[0]))
        self.n = int(v.shape[0])
        self.voxels = torch.from_numpy(v).to(device)
        self.ori = torch.from_numpy(o).to(device)
        self.index = torch.empty(int(np.prod(dims.astype(np.int64))), dtype=torch.int32, device=device)
        status = torch.empty(2, dtype=torch.int32, device=device)
        _lib.check(_lib.lib().mh_volume_index(_lib.bare_ctx(device), _lib.ptr(self.voxels), self.n, host_ptr(dims),
                                              _lib.ptr(self.index), _lib.ptr(status), _lib.stream_ptr()), "mh_volume_index")
        outside, twice = (int(s) for s in status.cpu().numpy())
        if outside or twice:
            raise ValueError("a voxel list must be unique and inside the grid: %d voxels outside, %d listed again"
                             % (outside, twice))


def _match_dev(q, t, dims, reach, cos2, device):
    out = torch.zeros(q.n, dtype=torch.uint8, device=device)
    if q.n == 0:
        return out
    r, c = np.ascontiguousarray(reach, dtype=np.int32), np.ascontiguousarray(cos2, dtype=np.float64)
    _lib.check(_lib.lib().mh_volume_match(_lib.bare_ctx(device), _lib.ptr(q.voxels), _lib.ptr(q.ori), q.n, _lib.ptr(t.index),
                                          _lib.ptr(t.ori), host_ptr(dims), host_ptr(r), host_ptr(c), int(r.shape[0]),
                                          _lib.ptr(out), _lib.stream_ptr()), "mh_volume_match")
    return out


def _bounds(reach, cos2):
    reach, cos2 = [int(r) for r in np.atleast_1d(reach)], [float(c) for c in np.atleast_1d(cos2)]
    if not (1 <= len(reach) <= MAX_PAIRS and len(cos2) == len(reach) and all(0 <= r <= MAX_REACH for r in reach)
            and not any(math.isnan(c) for c in cos2)):
        raise ValueError("between 1 and %d (reach 0..%d, cos2) pairs" % (MAX_PAIRS, MAX_REACH))
    return reach, cos2


def match_volume_flags(q_voxels, q_ori, t_voxels, t_ori, grid_resolution, reach, cos2, device="cuda:0"):
    """uint8 [Gq]: bit k of a query voxel is set iff some target voxel lies within Chebyshev distance reach[k] of it whose
    direction b passes cos2[k] < 0 or (a.b)^2 >= cos2[k] * (|a|^2 |b|^2) with |a|^2, |b|^2 > 0 (float64, bound included).
    cos2 is handed to the kernel as it is."""
    reach, cos2 = _bounds(reach, cos2)
    dims = grid_dims3(grid_resolution)
    with torch.cuda.device(device):
        q, t = _Volume(q_voxels, q_ori, dims, device), _Volume(t_voxels, t_ori, dims, device)
        return _match_dev(q, t, dims, reach, cos2, device).cpu().numpy()


def load_side(x):
    """a directory of Occ3D.mat / Ori3D.mat, or (grid_resolution, voxels, ori)"""
    if isinstance(x, (str, bytes)) or hasattr(x, "__fspath__"):
        return load_volume(x)
    return x


def build_result(thresholds, counts, grid_resolution):
    """The report: the host arithmetic on the integer counts ({"pred" / "gt": {"matched": [K], "voxels"}})."""
    P, R, F = scores_from_counts(counts["pred"]["matched"], counts["pred"]["voxels"], counts["gt"]["matched"],
                                 counts["gt"]["voxels"])
    return {"thresholds": [[int(r), None if a is None else float(a)] for r, a in thresholds],
            "grid_resolution": [int(v) for v in grid_resolution], "precision": P, "recall": R, "f_score": F, "counts": counts}


def score_volumes(pred, gt, thresholds=DEFAULT_THRESHOLDS, device="cuda:0", return_flags=False):
    """Precision (predicted voxels that have a ground-truth voxel within the bounds), recall (the roles swapped) and F-score
    per threshold pair (reach in voxels, degrees or None).  pred / gt: a directory holding Occ3D.mat and Ori3D.mat, or
    (grid_resolution, voxels [G,3], ori [G,3]); both on one grid.  -> dict; with return_flags also result["flags"] = {"pred":
    uint8 [G_pred], "gt": uint8 [G_gt]} (bit k: matched at pair k), in the order of the voxel lists."""
    thresholds = _check_thresholds(thresholds)
    K = len(thresholds)
    reach, cos2 = threshold_bounds(thresholds)
    (gp, vp, op), (gg, vg, og) = load_side(pred), load_side(gt)
    dims = grid_dims3(gp)
    if [int(v) for v in dims] != [int(v) for v in grid_dims3(gg)]:
        raise ValueError("the volumes are on different grids: %r and %r" % (list(gp), list(gg)))
    with torch.cuda.device(device):
        sides = {"pred": _Volume(vp, op, dims, device), "gt": _Volume(vg, og, dims, device)}
        flags, counts = {}, {}
        for name, other in (("pred", "gt"), ("gt", "pred")):
            flags[name] = _match_dev(sides[name], sides[other], dims, reach, cos2, device)
            c = flag_counts(flags[name], torch.ones_like(flags[name]), device)
            counts[name] = {"matched": c[:K], "voxels": c[8]}
    result = build_result(thresholds, counts, dims)
    if return_flags:
        result["flags"] = {name: flags[name].cpu().numpy() for name in flags}
    return result


def format_scores(result):
    """One line per threshold pair."""
    return ["reach %d / %s: precision %.4f  recall %.4f  f-score %.4f" % (r, "any direction" if a is None else "%g deg" % a,
                                                                         p, q, f)
            for (r, a), p, q, f in zip(result["thresholds"], result["precision"], result["recall"], result["f_score"])]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m monohair_amd.hairvolume",
                                 description="strands -> Occ3D.mat / Ori3D.mat, and one such volume scored against another")
    sp = ap.add_subparsers(dest="command", required=True)
    vx = sp.add_parser("voxelize", help="write the volume a strand set would ideally be fitted as")
    vx.add_argument("strands", help="STRANDS.hair")
    vx.add_argument("--out", required=True, help="directory of Occ3D.mat and Ori3D.mat")
    vx.add_argument("--bust_to_origin", type=float, nargs=3, default=(0.0, 0.0, 0.0), metavar=("X", "Y", "Z"))
    vx.add_argument("--grid", type=int, nargs=3, default=[int(v) for v in GRID_RESOLUTION], metavar=("X", "Y", "Z"))
    vx.add_argument("--vsize", type=float, default=VOXEL_SIZE, help="voxel size in metres (default %g)" % VOXEL_SIZE)
    vx.add_argument("--sub", type=int, default=2, help="samples per voxel of travel, 1..16 (default 2)")
    vx.add_argument("--device", default="cuda:0")
    sc = sp.add_parser("score", help="precision / recall / F-score of PRED_DIR against GT_DIR")
    sc.add_argument("pred")
    sc.add_argument("gt")
    sc.add_argument("--thresholds", type=parse_thresholds, default=DEFAULT_THRESHOLDS,
                    help="REACH:ANGLE pairs in voxels and degrees, - for any direction (default 0:-,1:-,1:30,1:20,1:10)")
    sc.add_argument("--json", default=None, help="write the result here")
    sc.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    if args.command == "voxelize":
        r = voxelize_strands(args.strands, args.bust_to_origin, VOXEL_MIN, args.vsize, args.grid, args.sub, args.device)
        write_volume(args.out, args.grid, r["voxels"], r["ori"])
        print("%d strands, %d samples -> %d voxels; %d segments dropped, %d samples outside the grid -> %s"
              % (r["strands"], r["samples"], len(r["voxels"]), r["dropped_segments"], r["outside_samples"], args.out))
        return 0
    result = score_volumes(args.pred, args.gt, args.thresholds, args.device)
    print("%d predicted voxels, %d ground-truth voxels" % (result["counts"]["pred"]["voxels"], result["counts"]["gt"]["voxels"]))
    for line in format_scores(result):
        print(line)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
