#!/usr/bin/env python
"""Time the HairGrow.py command, stage by stage, on the volume of the synthetic headline workload: the exterior pass of
tools/full_pass.py (60 views of 1920 x 1080, 256^3 candidates) writes refine/{Occ3D,Ori3D}.mat, a scalp cap of the 10 cm
sphere is written as an OBJ with `vn` records, and HairGrow.main runs on them with 60 000 scalp samples.
   python tools/hairgrow_pass.py [--views 60 --height 1920 --width 1080 --volume 256 --patch 7 --samples 60000]
Prints one JSON line: the pass's stage seconds, the command's per-stage seconds (HairGrow.run's dict) and the strand counts."""
import argparse
import json
import math
import os
import sys
import tempfile
import time
import types

import numpy as np
import torch
from scipy.spatial import KDTree

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import HairGrow  # noqa: E402
from monohair_amd import synth  # noqa: E402
from monohair_amd.camera import camera_records, cameras_from_list  # noqa: E402
from monohair_amd.pmvo import PMVO, filter_negative_points, optimize, refine  # noqa: E402
from monohair_amd.pmvo_utils import load_strand  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--views", type=int, default=60)
ap.add_argument("--height", type=int, default=1920)
ap.add_argument("--width", type=int, default=1080)
ap.add_argument("--volume", type=int, default=256)
ap.add_argument("--patch", type=int, default=7)
ap.add_argument("--samples", type=int, default=60000)
a = ap.parse_args()
dev = torch.device("cuda", 0)


def scalp_cap_obj(path, radius=0.10, n_lat=24, n_lon=48, y_min=0.03):
    """the part above y_min of a latitude / longitude sphere, with its outward normals as `vn` records"""
    vs, fs = [], []
    for i in range(n_lat + 1):
        th = math.pi * i / n_lat
        for j in range(n_lon):
            ph = 2 * math.pi * j / n_lon
            vs.append((math.sin(th) * math.cos(ph), math.cos(th), math.sin(th) * math.sin(ph)))
    for i in range(n_lat):
        for j in range(n_lon):
            p00, p01 = i * n_lon + j, i * n_lon + (j + 1) % n_lon
            fs += [(p00, p00 + n_lon, p01 + n_lon), (p00, p01 + n_lon, p01)]
    keep = [k for k, v in enumerate(vs) if v[1] * radius >= y_min]
    new = {k: m + 1 for m, k in enumerate(keep)}
    with open(path, "w") as f:
        for k in keep:
            f.write("v %.9f %.9f %.9f\n" % tuple(radius * c for c in vs[k]))
        for k in keep:
            f.write("vn %.9f %.9f %.9f\n" % vs[k])
        for t in fs:
            if all(k in new for k in t):
                f.write("f %d//%d %d//%d %d//%d\n" % tuple(new[k] for k in t for _ in range(2)))


T = {}
tmp = tempfile.mkdtemp()
case = os.path.join(tmp, "synthetic_sphere")
out = os.path.join(case, "output", "headline")
os.makedirs(os.path.join(case, "ours"))
os.makedirs(os.path.join(out, "refine"))
t0 = time.perf_counter()
scene = synth.make_scene(a.views, a.height, a.width, device=dev)
cams = cameras_from_list(scene["cams"])
pm = PMVO.from_planes(camera_records(cams), scene["depth"], scene["ori"], scene["conf"], scene["mask"], device=dev,
                      patch_size=a.patch, visible_threshold=1, conf_threshold=0.15, camera=cams)
rng = np.random.default_rng(1)
b = rng.normal(size=(2000, 3))
b = b / np.linalg.norm(b, axis=1, keepdims=True) * 0.09
scalp = b[b[:, 1] > 0.03] * (0.1 / 0.09)
pm.set_head(KDTree(b), KDTree(scalp), scalp.max(0))
cand = synth.candidate_points(res=a.volume, seed=0)
args = types.SimpleNamespace(device=str(dev), output_path=out, save_root=out + "/optimize", save_path=out + "/refine",
                             PMVO=types.SimpleNamespace(visible_threshold=1), data=types.SimpleNamespace(root=case))
s_idx, s_pts, f_idx = filter_negative_points(cand, pm, args)
sp, so, ml, hc = optimize(s_pts, pm, args)
refine(sp.copy(), so.copy(), ml.copy(), pm, cand[:len(f_idx)][f_idx].astype(np.float32), args, infer_inner=False,
       threshold=0.025, return_dense=False)
torch.cuda.synchronize()
T["exterior_pass_s"] = round(time.perf_counter() - t0, 3)
del pm, scene
torch.cuda.empty_cache()
scalp_cap_obj(os.path.join(case, "ours", "scalp_tsfm.obj"))
cwd = os.getcwd()
os.chdir(ROOT)
try:
    stages = HairGrow.main(["--yaml=configs/reconstruct/synthetic_sphere", "--data.root=%s" % tmp, "--name=headline",
                            "--data.image_size=[%d,%d]" % (a.height, a.width),
                            "--HairGenerate.num_scalp_samples=%d" % a.samples])
finally:
    os.chdir(cwd)
save = os.path.join(out, "refine")
counts = {"num_root": int(np.load(os.path.join(save, "num_root.npy")))}
for name in ("scalp_segment", "strands", "connected_strands"):
    segs, pts = load_strand(os.path.join(save, name + ".hair"))
    counts[name] = [len(segs), int(pts.shape[0])]
print(json.dumps({"views": a.views, "image": [a.height, a.width], "volume": a.volume, "scalp_samples": a.samples,
                  "candidates": len(cand), **T, "hairgrow": stages, **counts}))
