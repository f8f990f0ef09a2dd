"""Scoring one strand set against another: point-wise precision / recall / F-score under joint distance-and-direction
bounds (Nam et al., "Strand-accurate multi-view hair capture", CVPR 2019: a point counts when SOME point of the other set
lies within tau_d of it and runs within tau_a of its direction).  The reference has no counterpart -- its only metric class,
OccMetric (Utils/Utils.py:336-363), is training code the pipeline never calls -- so the specification is the one written out
in include/mh_pmvo.h and restated in numpy by tests/hair_metrics_np.py: float64 arithmetic on the float32 coordinates of a
`.hair` file, + - * / sqrt in a fixed order, both bounds inclusive, directions unsigned.

    python -m monohair_amd.hairmetrics PRED.hair GT.hair [--step 0.001] [--thresholds 0.001:10,0.002:20,0.003:30] [--json OUT]

The kernels are csrc/hairmetrics.hip; the targets' grid is mh_grid_build's (csrc/sortgroup.hip) with the cell rule of
hairgrow.grid_dims.  There is no CPU path."""
import argparse
import json
import math
import sys

import numpy as np
import torch

from . import _lib
from ._lib import host_ptr
from .hairgrow import grid_dims
from .strandset import StrandSet

DEFAULT_THRESHOLDS = ((0.001, 10.0), (0.002, 20.0), (0.003, 30.0))   # (metres, degrees)
MAX_PAIRS = 8                                                        # one bit of the flag byte each
_SLACK = 1.01          # cell = largest radius * slack: the float32 rounding of a cell index stays far below the 1 % it leaves
_MAX_DIM = 1 << 14     # ... as long as an index stays below this (its rounding error is index * 2^-23 cells)


def parse_thresholds(text):
    """'0.001:10,0.002:20' -> ((0.001, 10.0), (0.002, 20.0))"""
    pairs = []
    for item in text.split(","):
        d, sep, a = item.partition(":")
        if not sep:
            raise ValueError("threshold %r is not DIST:ANGLE" % item)
        pairs.append((float(d), float(a)))
    return _check_thresholds(pairs)


def _check_thresholds(pairs):
    pairs = tuple((float(d), float(a)) for d, a in pairs)
    if not 1 <= len(pairs) <= MAX_PAIRS:
        raise ValueError("between 1 and %d threshold pairs, got %d" % (MAX_PAIRS, len(pairs)))
    for d, a in pairs:
        if not (d > 0.0 and math.isfinite(d) and 0.0 <= a <= 90.0):
            raise ValueError("threshold (%r m, %r deg): the distance must be positive, the angle within [0, 90]" % (d, a))
    return pairs


def threshold_bounds(dist, angle_deg):
    """What the kernel compares against: r2 = tau_d * tau_d and c = cos(tau_a * (pi / 180)), float64."""
    return [float(d) * float(d) for d in dist], [math.cos(float(a) * (math.pi / 180.0)) for a in angle_deg]


def _dev(a, dtype, device):
    if isinstance(a, torch.Tensor):
        return a.to(device=device, dtype=dtype).contiguous()
    return torch.from_numpy(np.ascontiguousarray(a, dtype={torch.float32: np.float32, torch.float64: np.float64,
                                                           torch.uint8: np.uint8}[dtype])).to(device)


def _resample_dev(s, step, device):
    """the strand set resampled -> (counts int64 [S] host, offsets int64 [S+1] device, points float32 [m,3] device)"""
    counts, offs, pts, S = s.counts, s.offsets, s.points, s.S
    step = float(step)
    if not (step > 0.0 and math.isfinite(step)):
        raise ValueError("step must be a positive length, got %r" % step)
    if pts.shape[0] == 0:
        return counts, offs, pts
    L, ctx, st = _lib.lib(), _lib.bare_ctx(device), _lib.stream_ptr()
    cum = torch.empty(max(pts.shape[0], 1), dtype=torch.float64, device=device)
    m = torch.empty(S, dtype=torch.int64, device=device)
    _lib.check(L.mh_strand_arclen(ctx, _lib.ptr(pts), _lib.ptr(offs), S, step, _lib.ptr(cum), _lib.ptr(m), st),
               "mh_strand_arclen")
    soffs = torch.zeros(S + 1, dtype=torch.int64, device=device)
    torch.cumsum(m, 0, out=soffs[1:])
    total = int(soffs[-1])
    if not 0 <= total < 1 << 31:
        raise ValueError("step %g gives %d samples: more than 2^31 - 1" % (step, total))
    out = torch.empty((total, 3), dtype=torch.float32, device=device)
    _lib.check(L.mh_strand_resample(ctx, _lib.ptr(pts), _lib.ptr(offs), _lib.ptr(cum), _lib.ptr(soffs), S, total, step,
                                    _lib.ptr(out), st), "mh_strand_resample")
    return m.cpu().numpy(), soffs, out


def _tangents_dev(counts, offs, pts, device):
    n = pts.shape[0]
    tan = torch.empty((n, 3), dtype=torch.float64, device=device)
    valid = torch.empty(n, dtype=torch.uint8, device=device)
    _lib.check(_lib.lib().mh_strand_tangents(_lib.bare_ctx(device), _lib.ptr(pts), _lib.ptr(offs), counts.shape[0], n,
                                             _lib.ptr(tan), _lib.ptr(valid), _lib.stream_ptr()), "mh_strand_tangents")
    return tan, valid


def resample_strands(counts, points, step, device="cuda:0"):
    """Every strand resampled on its own at arc-length spacing `step` (metres) -> (counts int64 [S], points float32 [m,3])."""
    with torch.cuda.device(device):
        c, _, p = _resample_dev(StrandSet((counts, points), device), step, device)
        return c, p.cpu().numpy()


def strand_tangents(counts, points, device="cuda:0"):
    """-> (unit tangents float64 [n,3], valid uint8 [n]): central differences inside a strand, one-sided at its ends; a point
    of a one-point strand, or between coincident neighbours, has no direction (tangent 0, valid 0)."""
    with torch.cuda.device(device):
        s = StrandSet((counts, points), device)
        tan, valid = _tangents_dev(s.counts, s.offsets, s.points, device)
        return tan.cpu().numpy(), valid.cpu().numpy()


class _Targets:
    """The valid targets binned for radius `reach`: what one side of a comparison is matched against."""

    def __init__(self, pts, tan, valid, reach, device):
        keep = valid != 0
        pts, tan = pts[keep].contiguous(), tan[keep].contiguous()
        self.n = M = int(pts.shape[0])
        if M == 0:
            return
        L, ctx, st = _lib.lib(), _lib.bare_ctx(device), _lib.stream_ptr()
        box = torch.empty(6, dtype=torch.float32, device=device)
        _lib.check(L.mh_points_bbox(ctx, _lib.ptr(pts), M, _lib.ptr(box), st), "mh_points_bbox")
        box = box.cpu().numpy()
        if not np.isfinite(box).all():
            raise ValueError("a strand point is not finite")
        h, dims = grid_dims((box[3:] - box[:3]).astype(np.float64), max(reach, 1e-6), _SLACK, M)
        while max(dims) > _MAX_DIM:
            h *= 2.0
            dims = [int(d) for d in np.floor((box[3:] - box[:3]).astype(np.float64) / h).astype(np.int64) + 1]
        self.grid = np.array([box[0], box[1], box[2], h], np.float32)
        self.dims = np.array(dims, np.int32)
        self.scratch = torch.empty(int(L.mh_grid_scratch_bytes(M)), dtype=torch.uint8, device=device)
        self.pts = torch.empty((M, 3), dtype=torch.float32, device=device)
        order = torch.empty(M, dtype=torch.int32, device=device)
        self.cstart = torch.empty(int(np.prod(dims)) + 1, dtype=torch.int32, device=device)
        _lib.check(L.mh_grid_build(ctx, host_ptr(self.grid), host_ptr(self.dims), _lib.ptr(pts), M, _lib.ptr(self.scratch),
                                   self.scratch.numel(), _lib.ptr(self.pts), _lib.ptr(order), _lib.ptr(self.cstart), None,
                                   st), "mh_grid_build")
        self.tan = tan[order.long()].contiguous()


def _match_dev(q_pts, q_tan, q_valid, targets, r2, cos, device):
    nq = int(q_pts.shape[0])
    out = torch.zeros(nq, dtype=torch.uint8, device=device)
    if nq == 0 or targets.n == 0:
        return out
    L, ctx, st = _lib.lib(), _lib.bare_ctx(device), _lib.stream_ptr()
    scratch = torch.empty(int(L.mh_grid_scratch_bytes(nq)), dtype=torch.uint8, device=device)
    q_order = torch.empty(nq, dtype=torch.int32, device=device)
    _lib.check(L.mh_grid_build(ctx, host_ptr(targets.grid), host_ptr(targets.dims), _lib.ptr(q_pts), nq, _lib.ptr(scratch),
                               scratch.numel(), None, _lib.ptr(q_order), None, None, st), "mh_grid_build")
    r2h, ch = np.asarray(r2, np.float64), np.asarray(cos, np.float64)
    _lib.check(L.mh_strand_match(ctx, _lib.ptr(q_pts), _lib.ptr(q_tan), _lib.ptr(q_valid), _lib.ptr(q_order), nq,
                                 _lib.ptr(targets.pts), _lib.ptr(targets.tan), targets.n, _lib.ptr(targets.cstart),
                                 host_ptr(targets.grid), host_ptr(targets.dims), host_ptr(r2h), host_ptr(ch), int(r2h.shape[0]),
                                 _lib.ptr(out), st), "mh_strand_match")
    return out


def _bounds(dist, angle_deg, r2, cos):
    if r2 is None:
        r2, cos = threshold_bounds(np.atleast_1d(dist), np.atleast_1d(angle_deg))
    r2, cos = [float(v) for v in np.atleast_1d(r2)], [float(v) for v in np.atleast_1d(cos)]
    if not (1 <= len(r2) <= MAX_PAIRS and len(cos) == len(r2) and all(v >= 0.0 and math.isfinite(v) for v in r2)):
        raise ValueError("between 1 and %d (distance, angle) pairs with finite distances" % MAX_PAIRS)
    return r2, cos


def match_flags(q_pts, q_tan, q_valid, t_pts, t_tan, t_valid, dist=None, angle_deg=None, device="cuda:0", r2=None,
                cos=None):
    """uint8 [Nq]: bit k of a valid query is set iff some valid target lies within dist[k] of it with a direction within
    angle_deg[k] of its own (unsigned, both bounds included).  r2 / cos hand the kernel's float64 bounds over directly
    (squared distances, cosines) instead of dist / angle_deg."""
    r2, cos = _bounds(dist, angle_deg, r2, cos)
    with torch.cuda.device(device):
        qp, qt, qv = _dev(q_pts, torch.float32, device).reshape(-1, 3), _dev(q_tan, torch.float64, device).reshape(-1, 3), \
            _dev(q_valid, torch.uint8, device).reshape(-1)
        tp, tt, tv = _dev(t_pts, torch.float32, device).reshape(-1, 3), _dev(t_tan, torch.float64, device).reshape(-1, 3), \
            _dev(t_valid, torch.uint8, device).reshape(-1)
        if not (qp.shape[0] == qt.shape[0] == qv.shape[0] and tp.shape[0] == tt.shape[0] == tv.shape[0]):
            raise ValueError("points, tangents and valid flags of a side differ in length")
        targets = _Targets(tp, tt, tv, math.sqrt(max(r2)), device)
        return _match_dev(qp, qt, qv, targets, r2, cos, device).cpu().numpy()


def flag_counts(flags, valid, device):
    """the nine numbers of mh_flag_counts as ints: per bit k < 8 the flag bytes that have it, then the non-zero bytes of `valid`"""
    out = torch.empty(9, dtype=torch.int64, device=device)
    _lib.check(_lib.lib().mh_flag_counts(_lib.bare_ctx(device), _lib.ptr(flags), _lib.ptr(valid), int(flags.shape[0]),
                                         _lib.ptr(out), _lib.stream_ptr()), "mh_flag_counts")
    return [int(v) for v in out.cpu().numpy()]


def _ratio(a, b):
    return a / b if b else 0.0


def scores_from_counts(pred_matched, pred_valid, gt_matched, gt_valid):
    """(precision, recall, f_score) lists from the integer counts; a ratio with a zero denominator is 0."""
    P = [_ratio(m, pred_valid) for m in pred_matched]
    R = [_ratio(m, gt_valid) for m in gt_matched]
    return P, R, [_ratio(2.0 * p * r, p + r) for p, r in zip(P, R)]


def build_result(thresholds, step, counts, points, strands):
    """The report: the host arithmetic on the integer counts ({"pred" / "gt": {"matched": [K], "valid", "invalid"}})."""
    P, R, F = scores_from_counts(counts["pred"]["matched"], counts["pred"]["valid"], counts["gt"]["matched"],
                                 counts["gt"]["valid"])
    return {"thresholds": [[float(d), float(a)] for d, a in thresholds], "step": None if step is None else float(step),
            "precision": P, "recall": R, "f_score": F, "counts": counts, "points": points, "strands": strands}


def score_strands(pred, gt, thresholds=DEFAULT_THRESHOLDS, step=None, device="cuda:0", return_flags=False):
    """Precision (predicted points that have a ground-truth point within the bounds), recall (the roles swapped) and F-score
    per threshold pair (metres, degrees).  pred / gt: a `.hair` path or (counts, points).  step: resample both sets at this
    arc-length spacing first (None: the points as they are).  -> dict; with return_flags also result["flags"] = {"pred": uint8
    [n_pred], "gt": uint8 [n_gt]} (bit k: matched at pair k) over the points that were scored."""
    thresholds = _check_thresholds(thresholds)
    K = len(thresholds)
    r2, cos = threshold_bounds([d for d, _ in thresholds], [a for _, a in thresholds])
    reach = max(d for d, _ in thresholds)
    sides = {}
    with torch.cuda.device(device):
        for name, src in (("pred", pred), ("gt", gt)):
            s = StrandSet(src, device)
            c, o, p = (s.counts, s.offsets, s.points) if step is None else _resample_dev(s, step, device)
            tan, valid = _tangents_dev(c, o, p, device)
            sides[name] = (c, p, tan, valid)
        flags = {}
        for name, other in (("pred", "gt"), ("gt", "pred")):
            _, p, tan, valid = sides[name]
            _, op, otan, ovalid = sides[other]
            flags[name] = _match_dev(p, tan, valid, _Targets(op, otan, ovalid, reach, device), r2, cos, device)
        counts = {}
        for name in ("pred", "gt"):
            c = flag_counts(flags[name], sides[name][3], device)
            n = int(sides[name][1].shape[0])
            counts[name] = {"matched": c[:K], "valid": c[8], "invalid": n - c[8]}
    result = build_result(thresholds, step, counts, {name: int(sides[name][1].shape[0]) for name in sides},
                          {name: int(sides[name][0].shape[0]) for name in sides})
    if return_flags:
        result["flags"] = {name: flags[name].cpu().numpy() for name in flags}
    return result


def format_scores(result):
    """One line per threshold pair."""
    return ["%g mm / %g deg: precision %.4f  recall %.4f  f-score %.4f" % (d * 1000.0, a, p, r, f)
            for (d, a), p, r, f in zip(result["thresholds"], result["precision"], result["recall"], result["f_score"])]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m monohair_amd.hairmetrics",
                                 description="precision / recall / F-score of PRED.hair against GT.hair")
    ap.add_argument("pred")
    ap.add_argument("gt")
    ap.add_argument("--step", type=float, default=None, help="resample both at this spacing in metres (default: as stored)")
    ap.add_argument("--thresholds", type=parse_thresholds, default=DEFAULT_THRESHOLDS,
                    help="DIST:ANGLE pairs in metres and degrees (default 0.001:10,0.002:20,0.003:30)")
    ap.add_argument("--json", default=None, help="write the result here")
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    result = score_strands(args.pred, args.gt, args.thresholds, args.step, args.device)
    for line in format_scores(result):
        print(line)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
