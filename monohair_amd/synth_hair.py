"""A synthetic capture with known strands: a seeded strand model on the synthetic head of `synth.write_case`, and the GPU
renderer that turns any strand set -- generated here or read from a `.hair` file -- into the four per-view maps PMVO reads
(depth, orientation code, confidence code, hair mask), either as device-resident planes for `PMVO.from_u8` or as a complete
on-disk case in the reference's layout with the ground truth next to it:

    python -m monohair_amd.synth_hair --root data --case synthetic_hair [--hair GT.hair] [--views 24 --size 480x270
                                      --strands 2000 --seed 0 --radius 1 --tol 0.25]
                                      [--photo [--supersample 4 --width 1 --ambient 0.3]]
    python PMVO.py --yaml=configs/reconstruct/synthetic_hair
    python HairGrow.py --yaml=configs/reconstruct/synthetic_hair
    python -m monohair_amd.hairmetrics data/synthetic_hair/output/10-16/refine/connected_strands.hair \
                                       data/synthetic_hair/gt_strands.hair

The reference has no counterpart.  The capture rule is written out in include/mh_pmvo.h ("Hair capture") and restated in
numpy by tests/hair_capture_np.py; the kernels are csrc/haircapture.hip.  Hair is sub-pixel thin, so a pixel accumulates the
doubled-angle directions of all the strand samples near its front layer: where strands cross the confidence drops, as a Gabor
bank's would.  With --photo the capture is made of photographs instead (photo_planes: the "Hair photograph" rule of the same
header, restated by tests/hair_photo_np.py): capture_images/ holds shaded, anti-aliased gray pictures of the strands, and
best_ori/ and conf/ are what the Gabor stage makes of them.  There is no CPU path for the renderer; the strand model is host
code (numpy, libm: the same arrays for the same seed on one host, not bit for bit between hosts)."""
import argparse
import json
import math
import os
import sys

import numpy as np
import torch

from . import _lib, synth
from ._lib import host_ptr
from .camera import cameras_from_list
from .pmvo_utils import load_strand, read_obj, write_strand
from .strandset import Occluder, StrandSet, load, records

HEAD_R = 0.10          # the scalp sphere of synth.write_case (scalp_tsfm.obj)
BUST_R = 0.09          # its bust sphere (bust_long_tsfm.obj)
CAP_Y_MIN = 0.03       # the scalp cap: the part of the sphere with y >= this
CLEARANCE = 0.0005     # every point after the root stays at least this far outside the head
MAX_COLMAP_POINTS = 200000
# the photograph's defaults (what was tried): a strand 3 of 4 sub-pixels wide, a head light
PHOTO_SUPERSAMPLE = 4
PHOTO_WIDTH = 1
PHOTO_AMBIENT = 0.3
PHOTO_ALBEDO = (0.35, 1.0)
PHOTO_BUST_CODE = 64
PHOTO_BACKGROUND_CODE = 32


def code_table():
    """float32 [180,2]: (cos 2 theta_k, sin 2 theta_k), theta_k = k degrees -- the table mh_capture_resolve picks the
    orientation code from (host libm; handed to the kernel, so the host decides its last bits, not the device)."""
    th = np.arange(180, dtype=np.float64) * (math.pi / 180.0)
    return np.stack([np.cos(2.0 * th), np.sin(2.0 * th)], -1).astype(np.float32)


def make_hairstyle(n_strands=2000, n_points=64, seed=0, length=(0.10, 0.22), gravity=30.0, wave=(0.0, 0.6),
                   wave_length=(0.02, 0.05)):
    """A seeded hairstyle on the synthetic head -> (counts int64 [n_strands], points float32 [n_strands * n_points, 3]).

    Roots are uniform on the scalp cap (radius HEAD_R, y >= CAP_Y_MIN).  A strand leaves along the normal, its direction bends
    towards -y at `gravity` radians per metre, a per-strand helical wave (amplitude drawn from `wave`, in radians of direction;
    wave length from `wave_length`, metres) turns it about its own axis, and a point that would enter the head is pushed out to
    HEAD_R + CLEARANCE: long strands wrap around the head and hang below it, so the scene is non-convex and occludes itself."""
    n_strands, n_points = int(n_strands), int(n_points)
    if n_strands < 0 or not 2 <= n_points < 65536:
        raise ValueError("n_strands >= 0 and 2 <= n_points < 65536 (a .hair file counts points in 16 bits)")
    rng = np.random.default_rng(seed)
    y = rng.uniform(CAP_Y_MIN, HEAD_R, n_strands)                # uniform in height = uniform in area on a sphere
    az = rng.uniform(0.0, 2.0 * math.pi, n_strands)
    rho = np.sqrt(np.maximum(HEAD_R * HEAD_R - y * y, 0.0))
    normal = np.stack([rho * np.cos(az), y, rho * np.sin(az)], 1) / HEAD_R
    total = rng.uniform(length[0], length[1], n_strands)
    amp = rng.uniform(wave[0], wave[1], n_strands)
    omega = 2.0 * math.pi / rng.uniform(wave_length[0], wave_length[1], n_strands)
    phase = rng.uniform(0.0, 2.0 * math.pi, n_strands)
    ds = total / (n_points - 1)
    down = np.array([0.0, -1.0, 0.0])

    def unit(v):
        return v / np.maximum(np.linalg.norm(v, axis=1, keepdims=True), 1e-12)

    pts = np.empty((n_strands, n_points, 3), np.float64)
    p = normal * HEAD_R
    d = normal.copy()
    pts[:, 0] = p
    for i in range(1, n_points):
        s = ds * (i - 1)
        d = unit(d + down * (gravity * ds)[:, None])
        # a frame across the smooth direction for the wave
        e1 = unit(np.cross(d, normal + 1e-3))
        e2 = np.cross(d, e1)
        w = (amp * np.cos(omega * s + phase))[:, None] * e1 + (amp * np.sin(omega * s + phase))[:, None] * e2
        p = p + unit(d + w) * ds[:, None]
        r = np.linalg.norm(p, axis=1)
        inside = r < HEAD_R + CLEARANCE
        p = np.where(inside[:, None], p * ((HEAD_R + CLEARANCE) / np.maximum(r, 1e-12))[:, None], p)
        # a strand that was pushed out goes on along the surface, not into it
        n_here = p / np.maximum(np.linalg.norm(p, axis=1, keepdims=True), 1e-12)
        inward = np.minimum((d * n_here).sum(1), 0.0)
        d = np.where(inside[:, None], unit(d - inward[:, None] * n_here), d)
        pts[:, i] = p
    return np.full(n_strands, n_points, np.int64), pts.reshape(-1, 3).astype(np.float32)


def _empty(device, **specs):
    """name=(shape, dtype) -> dict of fresh device tensors: the pieces of a view that return_details hands back"""
    return {k: torch.empty(shape, dtype=dtype, device=device) for k, (shape, dtype) in specs.items()}


def _capture_stages(L, ctx, st, s, rec, H, W, radius, tol, n_full, d0, table, out):
    """One view by the stage calls mh_capture_view makes, on fresh tensors -> the details dict of capture_planes"""
    p, n = _lib.ptr, s.n
    b = _empty(s.points.device, vert=((max(n, 1), 3), torch.float32), valid=(max(n, 1), torch.uint8),
               zmin=((H, W), torch.float32), cnt=((H, W), torch.int32), c2=((H, W), torch.int64), s2=((H, W), torch.int64),
               dropped=(1, torch.int32))
    strands = (p(b["vert"]), p(b["valid"]), p(s.offsets), s.S, n, H, W, radius)
    _lib.check(L.mh_capture_project(ctx, host_ptr(rec), p(s.points), n, H, W, p(b["vert"]), p(b["valid"]), st),
               "mh_capture_project")
    _lib.check(L.mh_capture_zmin(ctx, *strands, p(d0), p(b["zmin"]), p(b["dropped"]), st), "mh_capture_zmin")
    _lib.check(L.mh_capture_accumulate(ctx, *strands, float(tol), p(d0), p(b["zmin"]), p(b["cnt"]), p(b["c2"]), p(b["s2"]), st),
               "mh_capture_accumulate")
    _lib.check(L.mh_capture_resolve(ctx, p(b["zmin"]), p(b["cnt"]), p(b["c2"]), p(b["s2"]), p(d0), host_ptr(table), n_full, H,
                                    W, *out, st), "mh_capture_resolve")
    return dict(b, vert=b["vert"][:n], valid=b["valid"][:n], dropped=int(b["dropped"].item()), depth0=d0)


def capture_planes(strands, camera, H, W, radius=1, tol=0.25, bust=None, device="cuda:0", return_details=False,
                   n_full=None, pixel_center=0.0):
    """strands = (counts, points); camera: dict view -> Camera (or [V,48] camera records) -> device tensors (depth float32
    [V,H,W], ori_u8, conf_u8, mask_u8 uint8 [V,H,W]): what PMVO.from_u8 takes.  bust = (vertices, faces): the occluder, drawn
    by render.DepthRenderer at the integer pixel positions PMVO rounds to (pixel_center 0).  With return_details a fifth value:
    per view a dict of the accumulators (vert, valid, zmin, cnt, c2, s2 tensors, dropped int, depth0 or None)."""
    if not torch.cuda.is_available():
        raise _lib.MhError("monohair_amd.synth_hair needs a ROCm GPU: the renderer has no CPU fallback")
    device = torch.device(device)
    H, W, radius = int(H), int(W), int(radius)
    n_full = 2 * radius + 1 if n_full is None else int(n_full)
    s = StrandSet(strands, device)
    recs = records(camera)
    V = recs.shape[0]
    table = code_table()
    L, ctx = _lib.lib(), _lib.bare_ctx(device)
    with torch.cuda.device(device):
        st = _lib.stream_ptr()
        depth = torch.empty((V, H, W), dtype=torch.float32, device=device)
        ori, conf, mask = (torch.empty((V, H, W), dtype=torch.uint8, device=device) for _ in range(3))
        occluder = Occluder(bust, device)
        details = []
        scratch = None if return_details else torch.empty(int(L.mh_capture_scratch_bytes(s.n, H, W)), dtype=torch.uint8,
                                                          device=device)
        for v in range(V):
            d0 = occluder.plane(recs[v], H, W, pixel_center)
            out = (_lib.ptr(depth[v]), _lib.ptr(ori[v]), _lib.ptr(conf[v]), _lib.ptr(mask[v]))
            if return_details:
                details.append(_capture_stages(L, ctx, st, s, recs[v], H, W, radius, tol, n_full, d0, table, out))
                continue
            _lib.check(L.mh_capture_view(ctx, host_ptr(recs[v]), _lib.ptr(s.points), _lib.ptr(s.offsets), s.S, s.n, H, W, radius,
                                         float(tol), n_full, _lib.ptr(d0), host_ptr(table), _lib.ptr(scratch), scratch.numel(),
                                         *out, st), "mh_capture_view")
        torch.cuda.current_stream().synchronize()      # (the occluder plane and the scratch are read asynchronously)
    if return_details:
        return depth, ori, conf, mask, details
    return depth, ori, conf, mask


def strand_albedo(n_strands, seed=0, lo=PHOTO_ALBEDO[0], hi=PHOTO_ALBEDO[1]):
    """float32 [n_strands], uniform in [lo, hi]: the per-strand albedo table mh_photo_shade is handed (host numpy in float64,
    rounded once; a stream of its own, so a strand's albedo says nothing about where make_hairstyle(seed=seed) rooted it)."""
    if not 0.0 <= float(lo) <= float(hi) <= 1.0:
        raise ValueError("0 <= lo <= hi <= 1")
    return np.random.default_rng([int(seed), 1]).uniform(float(lo), float(hi), int(n_strands)).astype(np.float32)


def light_directions(camera):
    """float64 [V,3], unit length: per view the world direction towards the camera -- the third row of the rotation of its
    world-to-camera pose (the camera looks down -z), normalised -- a head light."""
    r = records(camera)[:, 8:11].astype(np.float64)
    return r / np.sqrt((r * r).sum(1))[:, None]


def _photo_stages(L, ctx, st, s, rec, shading, H, W, ss, width, d0, bust_code, background_code, gray):
    """One view by the stage calls mh_photo_view makes, on fresh tensors -> the details dict of photo_planes"""
    p, n = _lib.ptr, s.n
    b = _empty(s.points.device, vert=((max(n, 1), 3), torch.float32), valid=(max(n, 1), torch.uint8),
               shade=(max(n, 1), torch.uint8), keys=((ss * H, ss * W), torch.int64), cover=((H, W), torch.int32),
               dropped=(1, torch.int32))
    _lib.check(L.mh_capture_project(ctx, host_ptr(rec), p(s.points), n, H, W, p(b["vert"]), p(b["valid"]), st),
               "mh_capture_project")
    _lib.check(L.mh_photo_shade(ctx, p(s.points), p(b["valid"]), p(s.offsets), s.S, n, *shading, p(b["shade"]), st),
               "mh_photo_shade")
    _lib.check(L.mh_photo_front(ctx, p(b["vert"]), p(b["valid"]), p(s.offsets), s.S, n, p(b["shade"]), H, W, ss, width, p(d0),
                                p(b["keys"]), p(b["dropped"]), st), "mh_photo_front")
    _lib.check(L.mh_photo_resolve(ctx, p(b["keys"]), p(d0), H, W, ss, bust_code, background_code, gray, p(b["cover"]), st),
               "mh_photo_resolve")
    return dict(b, vert=b["vert"][:n], valid=b["valid"][:n], shade=b["shade"][:n], dropped=int(b["dropped"].item()), depth0=d0)


def photo_planes(strands, camera, H, W, supersample=PHOTO_SUPERSAMPLE, width=PHOTO_WIDTH, ambient=PHOTO_AMBIENT, albedo=None,
                 seed=0, bust=None, bust_code=PHOTO_BUST_CODE, background_code=PHOTO_BACKGROUND_CODE, light=None,
                 device="cuda:0", return_details=False, pixel_center=0.0):
    """strands = (counts, points); camera as for capture_planes -> uint8 [V,H,W] device tensor: the gray photographs of the
    strand set by the photograph rule of include/mh_pmvo.h.  albedo: float32 [n_strands] (default strand_albedo(n_strands,
    seed)); light: float64 [V,3] unit vectors (default light_directions(camera)); bust = (vertices, faces): the occluder, drawn
    as capture_planes draws it and shown as bust_code.  With return_details a second value: per view a dict of vert, valid,
    shade (uint8 [n_points]: entry i is segment (i, i+1)), keys (int64 tensor holding the unsigned 64-bit key plane
    [S H, S W]), cover (int32 [H,W]), dropped (int), depth0 (or None)."""
    if not torch.cuda.is_available():
        raise _lib.MhError("monohair_amd.synth_hair needs a ROCm GPU: the renderer has no CPU fallback")
    device = torch.device(device)
    H, W, ss, width = int(H), int(W), int(supersample), int(width)
    s = StrandSet(strands, device)
    S, n = s.S, s.n
    recs = records(camera)
    V = recs.shape[0]
    albedo_h = strand_albedo(S, seed) if albedo is None else np.ascontiguousarray(albedo, dtype=np.float32).reshape(-1)
    if albedo_h.shape[0] != S or not (np.isfinite(albedo_h).all() and (albedo_h >= 0).all()):
        raise ValueError("albedo: one finite value >= 0 per strand")
    light_h = np.ascontiguousarray(light_directions(recs) if light is None else light, dtype=np.float64).reshape(-1, 3)
    if light_h.shape[0] != V:
        raise ValueError("light: one direction per view")
    L, ctx = _lib.lib(), _lib.bare_ctx(device)
    need = int(L.mh_photo_scratch_bytes(n, H, W, ss))
    if need == 0:
        raise ValueError("photo_planes: supersample in {1, 2, 4, 8} and supersample^2 * H * W < 2^31")
    with torch.cuda.device(device):
        st = _lib.stream_ptr()
        alb = torch.from_numpy(albedo_h if S else np.zeros(1, np.float32)).to(device)
        gray = torch.empty((V, H, W), dtype=torch.uint8, device=device)
        occluder = Occluder(bust, device)
        details = []
        scratch = None if return_details else torch.empty(need, dtype=torch.uint8, device=device)
        for v in range(V):
            d0 = occluder.plane(recs[v], H, W, pixel_center)
            shading = (_lib.ptr(alb), host_ptr(light_h[v]), float(ambient))
            if return_details:
                details.append(_photo_stages(L, ctx, st, s, recs[v], shading, H, W, ss, width, d0, int(bust_code),
                                             int(background_code), _lib.ptr(gray[v])))
                continue
            _lib.check(L.mh_photo_view(ctx, host_ptr(recs[v]), _lib.ptr(s.points), _lib.ptr(s.offsets), S, n, *shading, H, W,
                                       ss, width, _lib.ptr(d0), int(bust_code), int(background_code), _lib.ptr(scratch),
                                       scratch.numel(), _lib.ptr(gray[v]), None, st), "mh_photo_view")
        torch.cuda.current_stream().synchronize()      # (the occluder plane and the scratch are read asynchronously)
    if return_details:
        return gray, details
    return gray


def write_geometry(base, strands, cams, seed=0):
    """The files of a case that need no GPU, under the case directory `base`: ours/cam_params.json, the bust and scalp
    spheres of synth.write_case (the scalp with `vn` records), ours/colmap_points.obj -- a vertices-only OBJ of the strand
    points (a seeded subsample beyond MAX_COLMAP_POINTS), which the candidate sampling of PMVO.py reads -- and
    gt_strands.hair, the ground truth.  -> (counts, points) as written"""
    counts, points = load(strands)
    if counts.size and counts.max() >= 65536:
        raise ValueError("a strand of %d points: a .hair file counts them in 16 bits" % int(counts.max()))
    os.makedirs(os.path.join(base, "ours"), exist_ok=True)
    with open(os.path.join(base, "ours", "cam_params.json"), "w") as f:
        json.dump({"cam_list": cams}, f)
    synth.sphere_obj(os.path.join(base, "ours", "bust_long_tsfm.obj"), BUST_R, 24, 48)
    synth.sphere_obj(os.path.join(base, "ours", "scalp_tsfm.obj"), HEAD_R, 24, 48, y_min=CAP_Y_MIN, normals=True)
    sub = points
    if len(sub) > MAX_COLMAP_POINTS:
        sub = sub[np.sort(np.random.default_rng(seed).choice(len(sub), MAX_COLMAP_POINTS, replace=False))]
    with open(os.path.join(base, "ours", "colmap_points.obj"), "w") as f:
        f.write("".join("v %.9f %.9f %.9f\n" % (float(p[0]), float(p[1]), float(p[2])) for p in sub))
    write_strand(points, os.path.join(base, "gt_strands.hair"), [int(c) for c in counts])
    return counts, points


def write_case(root, case="synthetic_hair", V=24, H=480, W=270, seed=0, n_strands=2000, n_points=64, strands=None, radius=1,
               tol=0.25, scale=1.7, rings=1, device="cuda:0", photo=False, supersample=PHOTO_SUPERSAMPLE, width=PHOTO_WIDTH,
               ambient=PHOTO_AMBIENT):
    """Write a complete on-disk capture of a strand set in the layout of synth.write_case, so that
    `python PMVO.py --yaml=configs/reconstruct/<case>` and `python HairGrow.py ...` run on it through the real loaders:
      the files of write_geometry, capture_images/<view>.png, render_depth/<view>.npy [H,W,3] f32, best_ori/<view>.png (u8
      degrees), conf/<view>.png (u8), hair_mask/<view>.png.
    strands = (counts, points) renders that set instead of make_hairstyle(n_strands, n_points, seed).
    photo: capture_images/<view>.png are photographs (photo_planes; mode L), best_ori/, conf/ and Ori/ are what the Gabor
    stage makes of them through its file path (gabor.batch_generate), and the geometric codes go to gt_best_ori/ and
    gt_conf/; depth and hair mask stay geometric.  -> the case directory"""
    from PIL import Image

    base = os.path.join(root, case)
    for d in ("ours", "capture_images", "render_depth", "best_ori", "conf", "hair_mask"):
        os.makedirs(os.path.join(base, d), exist_ok=True)
    if strands is None:
        strands = make_hairstyle(n_strands, n_points, seed)
    cams = synth.make_cameras(V, H, W, scale=scale, rings=rings)
    counts, points = write_geometry(base, strands, cams, seed)
    bust = read_obj(os.path.join(base, "ours", "bust_long_tsfm.obj"))
    depth, ori, conf, mask = capture_planes((counts, points), cameras_from_list(cams), H, W, radius=radius, tol=tol,
                                            bust=bust, device=device)
    depth, ori, conf, mask = (t.cpu().numpy() for t in (depth, ori, conf, mask))
    ori_dir, conf_dir, image = "best_ori", "conf", conf
    if photo:
        ori_dir, conf_dir = "gt_best_ori", "gt_conf"
        for d in (ori_dir, conf_dir):
            os.makedirs(os.path.join(base, d), exist_ok=True)
        image = photo_planes((counts, points), cameras_from_list(cams), H, W, supersample=supersample, width=width,
                             ambient=ambient, seed=seed, bust=bust, device=device).cpu().numpy()
    for i, cam in enumerate(cams):
        name = cam["file"]
        np.save(os.path.join(base, "render_depth", name + ".npy"), np.repeat(depth[i][..., None], 3, axis=2))
        Image.fromarray(ori[i]).save(os.path.join(base, ori_dir, name + ".png"))
        Image.fromarray(conf[i]).save(os.path.join(base, conf_dir, name + ".png"))
        Image.fromarray(np.repeat(mask[i][..., None], 3, axis=2)).save(os.path.join(base, "hair_mask", name + ".png"))
        Image.fromarray(image[i]).save(os.path.join(base, "capture_images", name + ".png"))
    if photo:
        from . import gabor

        with torch.cuda.device(torch.device(device)):
            gabor.batch_generate(base, "capture_images")       # the shipped stage through its file path
    return base


def _size(text):
    h, sep, w = text.lower().partition("x")
    if not sep:
        raise argparse.ArgumentTypeError("size %r is not HxW" % text)
    return int(h), int(w)


def main(argv=None):
    ap = argparse.ArgumentParser(prog="python -m monohair_amd.synth_hair",
                                 description="write a synthetic capture whose ground-truth strands are known")
    ap.add_argument("--root", default="data")
    ap.add_argument("--case", default="synthetic_hair")
    ap.add_argument("--hair", default=None, help="render this .hair file instead of a generated hairstyle")
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--size", type=_size, default=(480, 270), help="HxW in pixels (default 480x270)")
    ap.add_argument("--strands", type=int, default=2000)
    ap.add_argument("--points", type=int, default=64, help="points per generated strand")
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--radius", type=int, default=1)
    ap.add_argument("--tol", type=float, default=0.25)
    ap.add_argument("--photo", action="store_true",
                    help="capture_images/ are rendered photographs and best_ori/, conf/ come from the Gabor stage run on them "
                         "(the geometric codes go to gt_best_ori/, gt_conf/)")
    ap.add_argument("--supersample", type=int, default=PHOTO_SUPERSAMPLE, choices=(1, 2, 4, 8))
    ap.add_argument("--width", type=int, default=PHOTO_WIDTH, help="half-width of a strand in sub-pixels")
    ap.add_argument("--ambient", type=float, default=PHOTO_AMBIENT)
    ap.add_argument("--device", default="cuda:0")
    args = ap.parse_args(argv)
    strands = None
    if args.hair:
        segments, points = load_strand(args.hair)
        strands = (np.asarray(segments, np.int64), points.astype(np.float32))
    base = write_case(args.root, args.case, V=args.views, H=args.size[0], W=args.size[1], seed=args.seed,
                      n_strands=args.strands, n_points=args.points, strands=strands, radius=args.radius, tol=args.tol,
                      device=args.device, photo=args.photo, supersample=args.supersample, width=args.width,
                      ambient=args.ambient)
    print("wrote %s (ground truth: %s)" % (base, os.path.join(base, "gt_strands.hair")))
    return 0


if __name__ == "__main__":
    sys.exit(main())
