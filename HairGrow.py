#!/usr/bin/env python
"""HairGrow.py -- the last command of the pipeline, same command line, YAML keys and files as the reference's HairGrow.py
(config_parser :837-873, __main__ :876-976):

    python HairGrow.py --yaml=configs/reconstruct/<case> [--PMVO.infer_inner] [--HairGenerate.generate_segments=]
                       [--HairGenerate.connect_segments=] [--HairGenerate.connect_scalp=] [--scalp_diffusion]
                       [--HairGenerate.diffuse_scalp] [--a.b=v]

in : data/<case>/output/<name>/{refine|full}/{Occ3D,Ori3D}.mat (PMVO.py), data/<case>/ours/scalp_tsfm.obj
out: in the same directory scalp_samples.npz, scalp_segment.hair, scalp_segment_smooth.hair, num_root.npy, strands.hair,
     connected_strands.hair

Stages, each behind its HairGenerate flag: generate_segments (scalp roots and voxel seeds traced on the volume,
csrc/hairgrow.hip), connect_segments (csrc/hairconnect.hip), connect_scalp (csrc/hairscalp.hip).  The scalp roots are
HairGenerate.num_scalp_samples points with interpolated normals sampled from the scalp mesh (csrc/meshsample.hip).  The
reference samples them with an unseeded generator; here the draw follows `seed`, the samples are saved to
scalp_samples.npz (`points`, `normals`: float32, voxel units, as tracing receives them), and
--HairGenerate.scalp_samples=<file.npz> feeds such a file back in place of sampling.  One HairGrowing serves all stages.
With --scalp_diffusion the stages read Occ3D_diffusion.mat / Ori3D_diffusion.mat, as in the reference, which has no
command that writes them: here a stage in front (csrc/hairdiffuse.hip, the reference's library function diffusion_scalp
on the scalp samples of the run) writes the two files when one is missing, or always with --HairGenerate.diffuse_scalp.
All arithmetic runs in the HIP library; this file is host orchestration.
"""
import json
import os
import sys
import time

import numpy as np

from monohair_amd import options

# the reference's defaults of the section (its configs/reconstruct/base.yaml:80-89) and the two keys added here
HAIRGENERATE_DEFAULTS = dict(connect_threshold=0.005, grow_threshold=0.8, connect_dot_threshold=0.7, generate_segments=True,
                             connect_segments=True, connect_scalp=True, out_ratio=0.5, num_scalp_samples=60000,
                             scalp_samples=None)
# a key no case file carries, consulted only when `scalp_diffusion` is set: write the _diffusion.mat files even if they exist
HAIRGENERATE_SWITCHES = dict(diffuse_scalp=False)


def config_parser(argv=None):
    print("Process ID: {}".format(os.getpid()))
    opt_cmd = options.parse_arguments(sys.argv[1:] if argv is None else argv)
    args = options.set(opt_cmd=opt_cmd)
    hg = args.setdefault("HairGenerate", options.Opt())
    for key, value in list(HAIRGENERATE_DEFAULTS.items()) + list(HAIRGENERATE_SWITCHES.items()):
        hg.setdefault(key, value)
    args.output_path = os.path.join(args.data.root, args.data.case, args.output_root, args.name)
    os.makedirs(args.output_path, exist_ok=True)
    options.save_options_file(args)
    args.data.root = os.path.join(args.data.root, args.data.case)
    args.bbox_min = np.array(args.bbox_min)
    args.bust_to_origin = np.array(args.bust_to_origin)
    for key in ("strands_path", "bust_path", "scalp_path"):
        args.data[key] = os.path.join(args.data.root, args.data[key])
    args.image_camera_path = os.path.join(args.data.root, args.image_camera_path)
    suffix = "_diffusion" if args.get("scalp_diffusion") else ""
    args.save_path = os.path.join(args.output_path, "full" if args.PMVO.infer_inner else "refine")
    args.data.Occ3D_path = os.path.join(args.save_path, "Occ3D{}.mat".format(suffix))
    args.data.Ori3D_path = os.path.join(args.save_path, "Ori3D{}.mat".format(suffix))
    return args


def scalp_samples(args):
    """The scalp roots of the run, (points, normals) float32 [n,3] tensors in voxel units: read from
    HairGenerate.scalp_samples when that names a file, otherwise sampled from the mesh at data.scalp_path with seed
    args.seed and saved to <save_path>/scalp_samples.npz."""
    import torch

    from monohair_amd.hairgrow import sample_scalp

    given = args.HairGenerate.scalp_samples
    if given:
        z = np.load(given)
        pts, nrm = np.asarray(z["points"], np.float32), np.asarray(z["normals"], np.float32)
        if pts.ndim != 2 or pts.shape[1] != 3 or nrm.shape != pts.shape:
            raise SystemExit("HairGrow: %s: `points` and `normals` must both be [n,3]" % given)
        return torch.from_numpy(pts), torch.from_numpy(nrm)
    pts, nrm = sample_scalp(args.data.scalp_path, args.bust_to_origin, int(args.HairGenerate.num_scalp_samples),
                            seed=args.get("seed"), device=args.device)
    np.savez(os.path.join(args.save_path, "scalp_samples.npz"), points=pts.cpu().numpy(), normals=nrm.cpu().numpy())
    return pts, nrm


def run(args, scalp_points=None, scalp_normals=None):
    """The stages of HairGrow.py's __main__ on a configured `args` (config_parser).  scalp_points / scalp_normals: the
    scalp roots in voxel units (float32 [n,3] tensors) in place of scalp_samples(args); they are needed by
    generate_segments only, so nothing is sampled or read when that stage is off.  Returns the wall seconds per stage, each
    read after the device has finished."""
    import torch

    from monohair_amd.hairgrow import HairGrowing, connect_scalp, connect_segments, diffuse_scalp, generate_segments

    hg, dev = args.HairGenerate, args.device
    T = {}

    def timed(name, fn):
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        T[name] = round(time.perf_counter() - t0, 4)
        return out

    t_all = time.perf_counter()
    os.makedirs(args.save_path, exist_ok=True)
    if args.get("scalp_diffusion") and (hg.diffuse_scalp or not (os.path.exists(args.data.Occ3D_path) and
                                                                 os.path.exists(args.data.Ori3D_path))):
        # the reference has the switch but no command that writes the two files it then reads
        if scalp_points is None or scalp_normals is None:
            scalp_points, scalp_normals = timed("scalp_samples_s", lambda: scalp_samples(args))
        timed("diffuse_scalp_s", lambda: diffuse_scalp(args.save_path, scalp_points, scalp_normals, device=dev))
    solver = timed("load_volume_s", lambda: HairGrowing(args.data.Occ3D_path, args.data.Ori3D_path, device=dev,
                                                        image_size=args.data.image_size))
    if hg.generate_segments:
        if scalp_points is None or scalp_normals is None:
            scalp_points, scalp_normals = timed("scalp_samples_s", lambda: scalp_samples(args))
        _, num_root = timed("generate_segments_s", lambda: generate_segments(
            None, None, scalp_points, scalp_normals, args.save_path, args.bust_to_origin, hg.grow_threshold, device=dev,
            write_smooth=True, solver=solver))
    else:
        num_root = int(np.load(os.path.join(args.save_path, "num_root.npy")))
    print("num_root:", num_root)
    if hg.connect_segments:
        timed("connect_segments_s", lambda: connect_segments(args.save_path, args.bust_to_origin, hg.connect_threshold,
                                                             hg.connect_dot_threshold, device=dev, solver=solver))
    if hg.connect_scalp:
        timed("connect_scalp_s", lambda: connect_scalp(args.save_path, args.bust_to_origin, hg.out_ratio, device=dev,
                                                       infer_inner=bool(args.PMVO.infer_inner), solver=solver))
    T["total_s"] = round(time.perf_counter() - t_all, 4)
    return T


def main(argv=None):
    print("Run HairGrow...")
    T = run(config_parser(argv))
    print(json.dumps(T))
    return T


if __name__ == "__main__":
    main()
