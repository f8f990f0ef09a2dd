"""Time of the photograph renderer per view: the default hairstyle at 1920 x 1080, S = 4, device events
around the three launches of a view -- mh_photo_shade, mh_photo_front (its fill of the key plane included) and
mh_photo_resolve -- on projected vertices, the median over the views after a warm-up.

    python tools/bench_photo.py [--views 24] [--size 1080x1920] [--supersample 4] [--width 1] [--strands 2000]"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from monohair_amd import _lib, strandset, synth, synth_hair as sh          # noqa: E402
from monohair_amd.camera import camera_records, cameras_from_list          # noqa: E402
from monohair_amd.pmvo_utils import _ctx_for          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--size", type=sh._size, default=(1080, 1920))
    ap.add_argument("--supersample", type=int, default=sh.PHOTO_SUPERSAMPLE)
    ap.add_argument("--width", type=int, default=sh.PHOTO_WIDTH)
    ap.add_argument("--strands", type=int, default=2000)
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    (H, W), ss, V = args.size, args.supersample, args.views
    counts, points = sh.make_hairstyle(args.strands, 64, seed=0)
    recs = camera_records(cameras_from_list(synth.make_cameras(V, H, W)))
    light = sh.light_directions(recs)
    offs_h = strandset.offsets(counts)
    n, S = len(points), len(counts)
    L, ctx, st, p = _lib.lib(), _ctx_for(dev), _lib.stream_ptr(), _lib.ptr
    pts, offs = torch.from_numpy(points).to(dev), torch.from_numpy(offs_h).to(dev)
    alb = torch.from_numpy(sh.strand_albedo(S, 0)).to(dev)
    vert = torch.empty((n, 3), dtype=torch.float32, device=dev)
    valid, shade = (torch.empty(n, dtype=torch.uint8, device=dev) for _ in range(2))
    keys = torch.empty((ss * H, ss * W), dtype=torch.int64, device=dev)
    gray = torch.empty((H, W), dtype=torch.uint8, device=dev)
    cover = torch.empty((H, W), dtype=torch.int32, device=dev)
    dropped = torch.empty(1, dtype=torch.int32, device=dev)
    inner = torch.ones(n - 1, dtype=torch.bool, device=dev)
    inner[offs[1:-1] - 1] = False                       # (no segment from a strand's last point to the next strand's first)
    times, hair, fill, frags = [], [], [], []
    for i in range(args.warmup + V):
        v = i % V
        rec = recs[v].ctypes.data_as(ctypes.c_void_p)
        _lib.check(L.mh_capture_project(ctx, rec, p(pts), n, H, W, p(vert), p(valid), st))
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        _lib.check(L.mh_photo_shade(ctx, p(pts), p(valid), p(offs), S, n, p(alb), light[v].ctypes.data_as(ctypes.c_void_p),
                                    sh.PHOTO_AMBIENT, p(shade), st))
        ev[1].record()
        _lib.check(L.mh_photo_front(ctx, p(vert), p(valid), p(offs), S, n, p(shade), H, W, ss, args.width, None, p(keys),
                                    p(dropped), st))
        ev[2].record()
        _lib.check(L.mh_photo_resolve(ctx, p(keys), None, H, W, ss, sh.PHOTO_BUST_CODE, sh.PHOTO_BACKGROUND_CODE, p(gray),
                                      p(cover), st))
        ev[3].record()
        # the fill alone: the front pass of an empty strand set
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        if i >= args.warmup:
            hair.append(int(cover.sum().item()))
            # the fragments of the view, before clipping at the image border: samples x footprint
            d = (vert[1:, :2].double() - vert[:-1, :2].double()).abs().amax(1) * ss
            ok = inner & (valid[1:] != 0) & (valid[:-1] != 0)
            frags.append(int(d[ok].ceil().clamp(min=1).sum().item()) * (2 * args.width + 1) ** 2)
        a.record()
        _lib.check(L.mh_photo_front(ctx, None, None, None, 0, 0, None, H, W, ss, args.width, None, p(keys), p(dropped), st))
        b.record()
        torch.cuda.synchronize()
        if i >= args.warmup:
            fill.append(a.elapsed_time(b))
            times.append([ev[k].elapsed_time(ev[k + 1]) for k in range(3)] + [ev[0].elapsed_time(ev[3])])
    t = np.median(np.array(times), axis=0)
    print(json.dumps(dict(views=V, H=H, W=W, supersample=ss, width=args.width, segments=int(n - S),
                          key_plane_bytes=int(keys.numel() * 8), hair_sub_pixels_median=int(np.median(hair)),
                          fragments_median=int(np.median(frags)),
                          ms_shade=round(float(t[0]), 4), ms_front_with_fill=round(float(t[1]), 4),
                          ms_fill_alone=round(float(np.median(fill)), 4),
                          ms_resolve=round(float(t[2]), 4), ms_view=round(float(t[3]), 4))))


if __name__ == "__main__":
    main()
