"""Scoring and pruning a strand set against the 2D maps of the capture it was reconstructed from: the strands are projected
into every view, the samples in front are kept, and their 2D direction is compared with the observed orientation code and
their footprint with the observed hair mask -- per view and per strand.  It needs no ground truth, so it works on a real
capture, where hairmetrics and `hairvolume score` have nothing to compare with.

    python -m monohair_amd.hairreproj score --yaml=configs/reconstruct/<case> [--strands PATH] [--json OUT] [--a.b=v]
    python -m monohair_amd.hairreproj prune --yaml=configs/reconstruct/<case> --out PATH [--strands PATH] [--min-cover 0.5]
                                            [--min-agree 0.5] [--angle 30] [--drop-unseen] [--a.b=v]

The reference has no counterpart.  The rule is written out in include/mh_pmvo.h ("Capture agreement") and restated in numpy
by tests/hair_reproj_np.py; the kernels are csrc/hairreproj.hip on top of the capture's projection and front pass
(csrc/haircapture.hip).  Every counter is an integer sum, so a run leaves the same numbers whatever order the GPU worked in.
There is no CPU path."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import _lib
from ._lib import host_ptr
from .pmvo_utils import map_code_lut, save_hair_strands, write_strand
from .strandset import Occluder, StrandSet, load, records
from .synth_hair import code_table

COLS = 4                     # visible, on hair, confident, dropped segments; then one column per angle
MAX_ANGLES = 8
DEFAULT_ANGLES = (10.0, 20.0, 30.0)


def conf_min_code(conf_threshold):
    """The smallest 8-bit confidence code PMVO counts as confident: the smallest c with map_code_lut()[c, 2] >
    float32(conf_threshold), PMVO's own comparison on the loaders' decode; 256 when there is none."""
    above = np.nonzero(map_code_lut()[:, 2] > np.float32(conf_threshold))[0]
    return int(above[0]) if above.size else 256


def angle_bounds(angles_deg):
    """What the kernel compares against: 4096 * cos(2 * angle), float64 -- a segment's (qc, qs) is 4096 times the unit
    double-angle vector, the table's entry a unit one, their dot product 4096 * cos(2 * difference)."""
    angles = [float(a) for a in np.atleast_1d(angles_deg)]
    if not 1 <= len(angles) <= MAX_ANGLES or not all(0.0 <= a <= 90.0 for a in angles):
        raise ValueError("between 1 and %d angles within [0, 90] degrees" % MAX_ANGLES)
    return angles, np.array([4096.0 * math.cos(2.0 * (a * (math.pi / 180.0))) for a in angles], np.float64)


def _plane(a, device):
    if isinstance(a, dict):
        a = np.stack([np.asarray(v) for v in a.values()])
    if isinstance(a, torch.Tensor):
        t = a.to(device=device)
    else:
        t = torch.from_numpy(np.ascontiguousarray(a)).to(device)
    if t.dtype != torch.uint8 or t.dim() != 3:
        raise ValueError("the observed planes are uint8 [V,H,W] pixel codes")
    return t.contiguous()


def support_counts(strands, camera, planes, bust=None, bust_to_origin=(0.0, 0.0, 0.0), angles_deg=DEFAULT_ANGLES,
                   conf_threshold=0.15, radius=1, tol=0.25, device="cuda:0", return_details=False, pixel_center=0.0,
                   timing=None):
    """strands: (counts, points) or a `.hair` path, stored relative to bust_to_origin (added on the host, float32(float64(x) +
    b) per component); camera: dict view -> Camera (or [V,48] camera records); planes = (ori_u8, conf_u8, mask_u8): uint8
    [V,H,W] device tensors or numpy arrays (or the dicts of load_maps_u8), what PMVO.from_u8 takes; bust = (vertices, faces) in
    world coordinates: the occluder, drawn by render.DepthRenderer as synth_hair.capture_planes draws it.
    -> (strand_counts int64 [S, 4 + K], view_counts int64 [V, 4 + K], silhouette int64 [V, 3]) numpy arrays, the rows and
    columns of "Capture agreement" in include/mh_pmvo.h: {visible, on hair, confident, dropped segments, agrees at
    angles_deg[0..K)} and {predicted and observed, predicted only, observed only}.  With return_details a fourth value, int64
    [V, S, 4 + K]: the per-strand rows of every view on its own (a second, zeroed buffer per view; their sum is asserted equal
    to the accumulated rows).  timing: a dict that receives "support_views_ms", device events around the per-view calls."""
    if not torch.cuda.is_available():
        raise _lib.MhError("monohair_amd.hairreproj needs a ROCm GPU: the scorer has no CPU fallback")
    device = torch.device(device)
    radius = int(radius)
    s = StrandSet(strands, device, shift=bust_to_origin)
    S, n, pts, offs = s.S, s.n, s.points, s.offsets
    recs = records(camera)
    V = recs.shape[0]
    _, bounds = angle_bounds(angles_deg)
    K = int(bounds.shape[0])
    cmin = conf_min_code(conf_threshold)
    table = code_table()
    L, ctx = _lib.lib(), _lib.bare_ctx(device)
    with torch.cuda.device(device):
        st = _lib.stream_ptr()
        ori, conf, mask = (_plane(a, device) for a in planes)
        if not (ori.shape == conf.shape == mask.shape and ori.shape[0] == V):
            raise ValueError("the observed planes must share one shape [V,H,W] with V = %d views" % V)
        H, W = int(ori.shape[1]), int(ori.shape[2])
        need = int(L.mh_support_scratch_bytes(n, H, W))
        if need == 0:
            raise ValueError("support_counts: H * W < 2^31")
        scratch = torch.empty(need, dtype=torch.uint8, device=device)
        strand = torch.zeros((max(S, 1), COLS + K), dtype=torch.int64, device=device)
        view = torch.zeros((V, COLS + K), dtype=torch.int64, device=device)
        sil = torch.zeros((V, 3), dtype=torch.int64, device=device)
        details = torch.zeros((V, max(S, 1), COLS + K), dtype=torch.int64, device=device) if return_details else None
        occluder = Occluder(bust, device)
        depth0 = [occluder.plane(recs[v], H, W, pixel_center) for v in range(V)]
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        for v in range(V):
            for rows in ([strand] if details is None else [strand, details[v]]):
                _lib.check(L.mh_support_view(ctx, host_ptr(recs[v]), _lib.ptr(pts), _lib.ptr(offs), S, n, H, W, radius, float(tol),
                                             _lib.ptr(depth0[v]), _lib.ptr(ori[v]), _lib.ptr(conf[v]), _lib.ptr(mask[v]), cmin,
                                             host_ptr(table), host_ptr(bounds), K, _lib.ptr(scratch), scratch.numel(),
                                             _lib.ptr(rows), _lib.ptr(view[v]), _lib.ptr(sil[v]), st), "mh_support_view")
        t1.record()
        torch.cuda.current_stream().synchronize()      # (the occluder planes and the scratch are read asynchronously)
        if timing is not None:
            timing["support_views_ms"] = float(t0.elapsed_time(t1))
        out = (strand[:S].cpu().numpy(), view.cpu().numpy(), sil.cpu().numpy())
        if details is not None:
            det = details[:, :S].cpu().numpy()
            assert np.array_equal(det.sum(0), out[0]), "the per-view rows do not sum to the accumulated ones"
            out += (det,)
    return out


def _ratio(a, b):
    return float(a) / float(b) if b else 0.0


def _scores(row, sil):
    """the ratios of one counter row and one silhouette triple"""
    row, sil = [int(x) for x in row], [int(x) for x in sil]
    vis, hair, confd, dropped, agrees = row[0], row[1], row[2], row[3], row[COLS:]
    both, pred_only, obs_only = sil
    return {"coverage": _ratio(hair, vis), "confident_share": _ratio(confd, hair),
            "agreement": [_ratio(a, confd) for a in agrees],
            "silhouette": {"precision": _ratio(both, both + pred_only), "recall": _ratio(both, both + obs_only),
                           "iou": _ratio(both, both + pred_only + obs_only)},
            "counts": {"visible": vis, "on_hair": hair, "confident": confd, "dropped_segments": dropped, "agrees": agrees,
                       "silhouette": sil}}


def build_result(angles_deg, conf_threshold, radius, tol, strand_counts, view_counts, silhouette, n_points):
    """The report: the host arithmetic on the integer counts.  coverage = on hair / visible, confident_share = confident / on
    hair, agreement[k] = agrees[k] / confident, the silhouette's precision / recall / IoU over pixels; a ratio with a zero
    denominator is 0.  "overall" sums the views."""
    view_counts, silhouette = np.asarray(view_counts, np.int64), np.asarray(silhouette, np.int64)
    return {"angles_deg": [float(a) for a in angles_deg], "conf_threshold": float(conf_threshold),
            "conf_min_code": conf_min_code(conf_threshold), "radius": int(radius), "tol": float(tol),
            "strands": int(np.shape(strand_counts)[0]), "points": int(n_points), "views": int(view_counts.shape[0]),
            "overall": _scores(view_counts.sum(0), silhouette.sum(0)),
            "per_view": [_scores(r, s) for r, s in zip(view_counts, silhouette)]}


def score_support(strands, camera, planes, bust=None, bust_to_origin=(0.0, 0.0, 0.0), angles_deg=DEFAULT_ANGLES,
                  conf_threshold=0.15, radius=1, tol=0.25, device="cuda:0", return_counts=False, timing=None):
    """support_counts and the ratios made of it -> dict (build_result); with return_counts also the per-strand rows."""
    angles, _ = angle_bounds(angles_deg)
    counts, points = load(strands)
    sc, vc, sil = support_counts((counts, points), camera, planes, bust, bust_to_origin, angles, conf_threshold, radius, tol,
                                 device, timing=timing)
    result = build_result(angles, conf_threshold, radius, tol, sc, vc, sil, points.shape[0])
    return (result, sc) if return_counts else result


def format_scores(result):
    """One line for the whole capture, one per view."""
    def line(name, s):
        agree = "  ".join("%g deg %.4f" % (a, v) for a, v in zip(result["angles_deg"], s["agreement"]))
        sl = s["silhouette"]
        return "%-8s coverage %.4f  confident %.4f  agreement %s  silhouette precision %.4f recall %.4f iou %.4f" % (
            name, s["coverage"], s["confident_share"], agree, sl["precision"], sl["recall"], sl["iou"])

    return [line("overall", result["overall"])] + [line("view %d" % v, s) for v, s in enumerate(result["per_view"])]


def prune_strands(strands, counts, min_cover=0.5, min_agree=0.5, angle_index=-1, min_visible=1, drop_unseen=False):
    """Drop the strands the images do not support.  counts: the per-strand rows of support_counts.  A strand with fewer than
    min_visible visible samples was not seen: it is kept unless drop_unseen is set.  A strand that was seen is kept iff
    on_hair >= min_cover * visible and agrees[angle_index] >= min_agree * confident (float64 products, both bounds included).
    -> ((counts, points) of the kept strands, the boolean mask [S]).  The default thresholds are inputs, not claims."""
    n_pts, points = load(strands)
    rows = np.asarray(counts, np.int64)
    if rows.ndim != 2 or rows.shape[0] != n_pts.shape[0] or rows.shape[1] <= COLS:
        raise ValueError("one counter row of at least %d columns per strand" % (COLS + 1))
    vis, hair, confd = (rows[:, k].astype(np.float64) for k in range(3))
    agrees = rows[:, COLS:][:, angle_index].astype(np.float64)
    seen = rows[:, 0] >= int(min_visible)
    supported = (hair >= float(min_cover) * vis) & (agrees >= float(min_agree) * confd)
    keep = np.where(seen, supported, not drop_unseen)
    return (n_pts[keep], points[np.repeat(keep, n_pts)]), keep


# ------------------------------------------------------------------------------------------------------------ command line
def _case(rest):
    """The case as PMVO.py loads it: cameras, 8-bit maps, bust, thresholds and the default strands path."""
    from . import options
    from .camera import load_cam, parsing_camera
    from .pmvo_utils import load_maps_u8, read_obj

    args = options.set(opt_cmd=options.parse_arguments(rest))
    root = os.path.join(args.data.root, args.data.case)
    out = os.path.join(root, args.output_root, args.name)
    b2o = np.array(args.bust_to_origin, np.float64)
    camera = parsing_camera(load_cam(os.path.join(root, args.image_camera_path)), os.path.join(root, "capture_images"))
    planes = load_maps_u8(camera, os.path.join(root, args.data.Ori2D_path), os.path.join(root, args.data.Conf_path),
                          os.path.join(root, args.data.mask_path))
    vertices, faces = read_obj(os.path.join(root, args.data.bust_path))
    strands = os.path.join(out, "full" if args.PMVO.infer_inner else "refine", "connected_strands.hair")
    return dict(camera=camera, planes=planes, bust=(vertices + b2o, faces), bust_to_origin=b2o,
                conf_threshold=float(args.PMVO.conf_threshold), device=args.device, strands=strands)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m monohair_amd.hairreproj",
                                 description="score or prune strands against the capture's own 2D maps; options of the "
                                             "case (--yaml=..., --a.b=v) are passed on to the pipeline's option parser")
    sp = ap.add_subparsers(dest="command", required=True)
    sc = sp.add_parser("score", help="coverage, agreement and silhouette of a strand file, per view and overall")
    pr = sp.add_parser("prune", help="write the strands the images support")
    for p in (sc, pr):
        p.add_argument("--strands", default=None, help="STRANDS.hair (default: the run's connected_strands.hair)")
        p.add_argument("--angles", type=lambda t: [float(a) for a in t.split(",")], default=list(DEFAULT_ANGLES),
                       help="agreement angles in degrees (default 10,20,30)")
        p.add_argument("--radius", type=int, default=1)
        p.add_argument("--tol", type=float, default=0.25)
    sc.add_argument("--json", default=None, help="write the result here")
    pr.add_argument("--out", required=True, help="the pruned .hair file")
    pr.add_argument("--min-cover", type=float, default=0.5)
    pr.add_argument("--min-agree", type=float, default=0.5)
    pr.add_argument("--angle", type=float, default=None, help="the agreement angle to prune at (default: the last of --angles)")
    pr.add_argument("--min-visible", type=int, default=1)
    pr.add_argument("--drop-unseen", action="store_true")
    args, rest = ap.parse_known_args(sys.argv[1:] if argv is None else argv)
    case = _case(rest)
    default = case.pop("strands")
    path = args.strands or default
    if args.command == "prune":
        if os.path.exists(args.out) and os.path.samefile(args.out, path):
            raise SystemExit("hairreproj prune: --out is the input file %s" % path)
        if args.angle is not None and args.angle not in args.angles:
            args.angles = args.angles + [args.angle]
    timing = {}
    result, rows = score_support(path, angles_deg=args.angles, radius=args.radius, tol=args.tol, return_counts=True,
                                 timing=timing, **case)
    print("%s: %d strands, %d points, %d views; the views took %.3f ms on the device"
          % (path, result["strands"], result["points"], result["views"], timing["support_views_ms"]))
    for line in format_scores(result):
        print(line)
    if args.command == "score":
        if args.json:
            with open(args.json, "w") as f:
                json.dump(result, f, indent=1)
        return 0
    index = -1 if args.angle is None else args.angles.index(args.angle)
    (n_pts, points), keep = prune_strands(path, rows, args.min_cover, args.min_agree, index, args.min_visible,
                                          args.drop_unseen)
    if len(n_pts):       # (the file's points are relative to bust_to_origin already: nothing to translate)
        save_hair_strands(args.out, [points[e - c:e] for c, e in zip(n_pts, np.cumsum(n_pts))], case["bust_to_origin"],
                          translate=False)
    else:
        write_strand(points, args.out, [])
    print("kept %d of %d strands -> %s" % (int(keep.sum()), int(keep.shape[0]), args.out))
    return 0


if __name__ == "__main__":
    sys.exit(main())
