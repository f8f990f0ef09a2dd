#!/usr/bin/env python
"""Time the segment connection stage (find_connect_info + smoothing) on the GPU.

    python tools/bench_connect.py                         # the fixture's traced segments (tests/golden/hair_connect.npz)
    python tools/bench_connect.py --occ Occ3D.mat --ori Ori3D.mat    # full size: the segments generate_segments traces
                                                          # from a fitted volume (e.g. the one tools/full_pass.py writes)
Prints one JSON line: segment count, points in / out, stage and per-step wall times (ms, median of --reps)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from monohair_amd.hairgrow import HairGrowing  # noqa: E402
from monohair_amd.strand_smooth import smooth_strands  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--occ")
ap.add_argument("--ori")
ap.add_argument("--reps", type=int, default=5)
a = ap.parse_args()
dev = "cuda:0"

if a.occ:
    hg = HairGrowing(a.occ, a.ori, device=dev)
    torch.manual_seed(0)
    segs = hg.randomlyGenerateSegments(0.8)
    segs = hg.VoxelToWorld(segs)
    segs = [s.astype(np.float64) for s in segs]
    label = "full"
else:
    z = np.load(os.path.join(ROOT, "tests", "golden", "hair_connect.npz"))
    G = tuple(int(g) for g in z["vol_shape"])
    occ = np.zeros(G, np.float32)
    occ[tuple(z["occ_nz"].T.astype(np.int64))] = 1
    ori = np.zeros(G + (3,), np.float32)
    ori[tuple(z["ori_nz"].T.astype(np.int64))] = z["ori_nz_val"]
    hg = HairGrowing(None, None, device=dev, occ=occ.transpose(2, 1, 0)[..., None], ori=ori.transpose(2, 1, 0, 3))
    b = z["seg_hair"].tobytes()
    n = int(np.frombuffer(b[:4], "<u4")[0])
    lens = np.frombuffer(b[8:8 + 2 * n], "<u2").astype(int)
    pts = np.frombuffer(b[8 + 2 * n:], "<f4").astype(np.float64).reshape(-1, 3)
    segs = [s + z["bust"] for s in np.split(pts, np.cumsum(lens)[:-1])[int(z["num_root"]):]]
    label = "fixture"

times = {"connect": [], "smooth": []}
for r in range(a.reps + 1):
    np.random.seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = hg.find_connect_info([s.copy() for s in segs])
    t1 = time.perf_counter()
    sm = smooth_strands(list(out), 4.0, 2.0, device=dev)
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    if r:                       # the first round loads the code objects
        times["connect"].append((t1 - t0) * 1e3)
        times["smooth"].append((t2 - t1) * 1e3)
med = {k: float(np.median(v)) for k, v in times.items()}
print(json.dumps(dict(case=label, segments=len(segs), points_in=int(sum(s.shape[0] for s in segs)),
                      points_out=int(sum(s.shape[0] for s in out)), fail=hg.connect_fail,
                      connect_ms=round(med["connect"], 2), smooth_ms=round(med["smooth"], 2),
                      stage_ms=round(med["connect"] + med["smooth"], 2),
                      us_per_segment=round((med["connect"] + med["smooth"]) * 1e3 / max(len(segs), 1), 2))))
