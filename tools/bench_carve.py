"""Times of the silhouette carve (docs/PARITY.md f11): the default synthetic capture (24 views of 480 x 270,
2 000 strands) carved on PMVO.py's candidate grid (512 x 512 x 384 at 1.25 mm), device events around each call, warm, the
median of five -- mh_carve_inside in both forms of the kernel (the lab switch "carve_early_exit": the one decision these
numbers carry), mh_carve_mesh_count, mh_carve_mesh, and the 24 depth renders of the hull and of the bust.  Prints one JSON
line; profiles/carve_timing.json is the record of a run.

    python tools/bench_carve.py [--voxel-size 0.00125] [--min-free 2] [--max-miss 0 3] [--rounds 5]"""
import argparse
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monohair_amd import _lib, gridviews, haircarve, synth_hair          # noqa: E402
from monohair_amd.camera import camera_records, load_cam, parsing_camera          # noqa: E402
from monohair_amd.pmvo_utils import VOXEL_MIN, load_bust          # noqa: E402
from monohair_amd.render import DepthRenderer          # noqa: E402


def timed(fn, rounds):
    """-> (median ms, [ms]) of `rounds` calls after one warm-up call"""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(rounds):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(round(a.elapsed_time(b), 4))
    return dict(median_ms=float(np.median(ms)), ms=ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-size", type=float, default=haircarve.CARVE_VOXEL_SIZE)
    ap.add_argument("--min-free", type=int, default=2)
    ap.add_argument("--max-miss", type=int, nargs="+", default=[0, 3])
    ap.add_argument("--rounds", type=int, default=5)
    args = ap.parse_args()
    data = tempfile.mkdtemp(prefix="bench_carve_")
    try:
        base = synth_hair.write_case(data, "synthetic_hair")          # its defaults: 24 views of 480 x 270, 2 000 strands
        camera = parsing_camera(load_cam(os.path.join(base, "ours", "cam_params.json")), os.path.join(base, "capture_images"))
        masks = haircarve.load_masks(camera, os.path.join(base, "hair_mask"))
        bv, bf, _ = load_bust(os.path.join(base, "ours", "bust_long_tsfm.obj"))
    finally:
        shutil.rmtree(data, ignore_errors=True)
    H, W = next(iter(masks.values())).shape
    pmvo = haircarve.mask_context(masks, camera, [H, W])
    bust = gridviews.bust_planes(pmvo, (bv, bf))
    vmin, vs, dims = gridviews.grid(VOXEL_MIN, args.voxel_size, haircarve.carve_grid(args.voxel_size))
    out = dict(views=len(camera), H=H, W=W, dims=[int(d) for d in dims], voxel_size=vs, min_free=args.min_free, inside={})
    for max_miss in args.max_miss:
        for early in (1, 0):
            pmvo.set_lab_option("carve_early_exit", early)
            out["inside"]["max_miss%d_early_exit%d" % (max_miss, early)] = timed(
                lambda: haircarve._inside_dev(pmvo, bust, vmin, vs, dims, args.min_free, max_miss), args.rounds)
    pmvo.set_lab_option("carve_early_exit", 1)
    flags = haircarve._inside_dev(pmvo, bust, vmin, vs, dims, args.min_free, args.max_miss[0])
    L, st, p = _lib.lib(), _lib.stream_ptr(), _lib.ptr
    need = int(L.mh_carve_mesh_scratch_bytes(_lib.host_ptr(dims)))
    ctx = _lib.bare_ctx("cuda:0")
    scratch = torch.empty(need, dtype=torch.uint8, device="cuda")
    counts = torch.empty(2, dtype=torch.int64, device="cuda")
    out["mesh_count"] = timed(lambda: _lib.check(L.mh_carve_mesh_count(ctx, p(flags), _lib.host_ptr(dims), p(counts), p(scratch),
                                                                       need, st)), args.rounds)
    nv, nt = (int(c) for c in counts.cpu().numpy())
    v = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    t = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
    out["mesh"] = timed(lambda: _lib.check(L.mh_carve_mesh(ctx, p(flags), _lib.host_ptr(vmin), vs, _lib.host_ptr(dims), nv, nt,
                                                           p(v), p(t), p(scratch), need, st)), args.rounds)
    out.update(n_inside=int(flags.sum().item()), n_vertices=nv, n_triangles=nt, scratch_bytes=need)
    recs = camera_records(camera)
    planes = torch.empty((len(recs), H, W), dtype=torch.float32, device="cuda")
    for name, mesh in (("depth_hull", (v.cpu().numpy(), t.cpu().numpy())), ("depth_bust", (bv, bf))):
        r = DepthRenderer([mesh], "cuda:0")

        def draw():
            for i in range(len(recs)):
                r.render(recs[i], H, W, 0.0, out=planes[i])
        out[name + "_all_views"] = timed(draw, args.rounds)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
