"""Golden vectors of the segment connection stage (tests/golden/hair_connect.npz), run by the imported reference.

    python tools/gen_golden_connect.py

Case "shell": the reference's HairGrowing traces a synthetic 256x256x192 volume (a noisy spherical shell) from the CPU,
then the generate_segments / connect_segments stages of HairGrow.py's __main__ (:897-952) run on the result:
scalp_segment.hair, scalp_segment_smooth.hair, the connection table, the connected float64 strands, the fail count,
np.random's next value and strands.hair are recorded.  Case "edge": find_connect_info on hand-made segments (more than 50
ends within the radius, an end at exactly the bound, cycles, strands leaving the box, negative voxel indices, isolated
segments) plus some traced ones.

points_to_voxel is wrapped to clone its input: on a CPU device torch.from_numpy(ss).to(occ.device) aliases `ss`, and the
reference's in-place points_to_voxel would negate the strand itself (on the CUDA device the reference targets, .to()
copies).
"""
import contextlib
import io
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)

from ref_import import import_reference  # noqa: E402
from gen_golden_more import hair_volume  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
G = (256, 256, 192)      # X, Y, Z: the box the reference's occupancy test hard-codes
VMIN = np.array([-0.32, -0.32, -0.24], np.float32).astype(np.float64)
BUST = np.array([0.006, -0.0125, 0.031])
THR, DOT = 0.005, 0.7


def vox_to_world(v):
    return (v * 0.0025 + VMIN) * np.array([1.0, -1.0, -1.0])


def end_lists(strands, thr):
    """The reference's four end queries (KDTree.query(k=50, distance_upper_bound)) and a brute force ordered by
    (distance, index); asserts that scipy orders every list like the brute force (no tie resolved otherwise)."""
    from scipy.spatial import KDTree

    roots = np.stack([s[0] for s in strands])
    tips = np.stack([s[-1] for s in strands])
    out = {}
    for name, q, d in (("rr", roots, roots), ("rt", roots, tips), ("tr", tips, roots), ("tt", tips, tips)):
        tree = KDTree(d)
        idx = np.full((len(q), 50), -1, np.int32)
        dist = np.zeros((len(q), 50))
        for i, p in enumerate(q):
            nd, ni = tree.query(p, k=50, distance_upper_bound=thr)
            keep = nd < 9999
            nd, ni = nd[keep], ni[keep]
            self_ = ni == i
            nd, ni = nd[~self_], ni[~self_]
            df = p - d
            dd = (df[:, 0] * df[:, 0] + df[:, 1] * df[:, 1]) + df[:, 2] * df[:, 2]
            cand = np.flatnonzero(dd < thr * thr)
            cand = cand[np.lexsort((cand, dd[cand]))][:50]
            cand = cand[cand != i]
            assert np.array_equal(cand, ni), (name, i, cand, ni)
            assert np.array_equal(np.sqrt(dd[cand]), nd), (name, i)
            idx[i, :len(ni)] = ni
            dist[i, :len(ni)] = nd
        out[name + "_idx"] = idx.astype(np.int16)     # the distances follow from the indices (checked above)
    return out


def table_array(info):
    t = np.full((len(info), 2, 2), -1, np.int32)
    for i, ci in enumerate(info):
        for k, e in enumerate(("root", "tip")):
            if ci[e] is not None:
                t[i, k] = (int(ci[e][0]), 0 if ci[e][1] == "root" else 1)
    return t


def run_connect(HairGrow, solver, strands):
    """find_connect_info with the table captured, the draws per strand counted and the fail count parsed."""
    rec = {"table": None, "draws": []}
    orig_cs = HairGrow.HairGrowing.connect_segments
    orig_rand = np.random.random

    def cs(self, info, ss, i):
        if rec["table"] is None:
            rec["table"] = table_array(info)
        rec["draws"].append(0)
        return orig_cs(self, info, ss, i)

    def rnd(*a, **k):
        if rec["draws"]:
            rec["draws"][-1] += 1
        return orig_rand(*a, **k)

    HairGrow.HairGrowing.connect_segments = cs
    np.random.random = rnd
    buf = io.StringIO()
    try:
        with contextlib.redirect_stdout(buf):
            out = solver.find_connect_info(strands, THR, DOT, solver.occ)
    finally:
        HairGrow.HairGrowing.connect_segments = orig_cs
        np.random.random = orig_rand
    fail = int([ln for ln in buf.getvalue().splitlines() if ln.startswith("fail:")][0].split()[1])
    return out, rec["table"], np.array(rec["draws"], np.int32), fail


def pack(prefix, strands, out):
    out[prefix + "_len"] = np.array([s.shape[0] for s in strands], np.int32)
    out[prefix + "_pts"] = np.concatenate(strands, 0)


def edge_segments(rng):
    segs = []
    c = np.array([128.0, 150.0, 96.0])
    for k in range(60):                        # > 50 roots within the radius of each other
        d = rng.normal(size=3)
        d /= np.linalg.norm(d)
        p0 = c + rng.normal(scale=0.3, size=3)
        segs.append(vox_to_world(p0 + np.outer(np.arange(6), d) * 0.8))
    for k in range(8):                         # a ring: the tip of each segment meets the root of the next
        a0, a1 = 2 * np.pi * k / 8, 2 * np.pi * (k + 1) / 8
        t = np.linspace(a0, a1, 7)
        segs.append(vox_to_world(np.stack([128 + 14 * np.cos(t), 128 + 14 * np.sin(t), 96 + 0 * t], 1)))
    t = np.arange(8)[:, None]
    segs.append(vox_to_world(np.array([250.0, 128, 96]) + t * np.array([1.0, 0, 0])))      # leaves the box (x >= 256)
    segs.append(vox_to_world(np.array([3.0, 128, 96]) - t * np.array([1.0, 0, 0])))        # negative x indices
    segs.append(vox_to_world(np.array([128.0, 20, 20]) + t * np.array([0, 1.0, 0])))       # isolated
    # an end at exactly the bound: x = 0 and x = THR give a float64 squared distance of exactly THR*THR
    p = np.array([0.0, -0.1, -0.05])
    q = np.array([THR, -0.1, -0.05])
    assert (p[0] - q[0]) * (p[0] - q[0]) == THR * THR
    segs.append(p + np.outer(np.arange(-7, 1), [0, 0, 0.0025]))
    segs.append(q + np.outer(np.arange(8), [0, 0, -0.0025]))
    return segs


def main():
    R = import_reference()
    os.chdir("/tmp")
    import scipy.io

    import HairGrow
    import Utils.Utils as U

    orig_ptv = HairGrow.points_to_voxel
    HairGrow.points_to_voxel = lambda p: orig_ptv(p.clone())      # see the module docstring
    occ, ori = hair_volume(G, R=10.0, seed=4)
    tmp = tempfile.mkdtemp(prefix="mh_hc_")
    o = ori.transpose((0, 1, 3, 2)).reshape(G[0], G[1], G[2] * 3).transpose((1, 0, 2))
    scipy.io.savemat(os.path.join(tmp, "Ori3D.mat"), {"Ori": o})
    scipy.io.savemat(os.path.join(tmp, "Occ3D.mat"), {"Occ": occ.transpose((1, 0, 2))})
    rng = np.random.default_rng(11)
    nrm = rng.normal(size=(300, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    centre = np.array([G[0] / 2, G[1] / 2, G[2] / 2])
    pts = (centre + nrm * 6.0 + rng.normal(0, 0.3, size=(300, 3))).astype(np.float32)
    nrm = nrm.astype(np.float32)
    nz = np.argwhere(occ != 0)
    out = dict(vol_shape=np.array(G), occ_nz=nz.astype(np.int16),
               ori_nz=np.argwhere(np.any(ori != 0, -1)).astype(np.int16), scalp_points=pts, scalp_normals=nrm,
               bust=BUST, thr=np.float64(THR), dot=np.float64(DOT))
    out["ori_nz_val"] = ori[tuple(out["ori_nz"].T.astype(np.int64))].astype(np.float32)

    solver = HairGrow.HairGrowing(os.path.join(tmp, "Occ3D.mat"), os.path.join(tmp, "Ori3D.mat"), device="cpu")
    torch.manual_seed(77)
    with contextlib.redirect_stdout(io.StringIO()):
        strands, num_root = solver.GenerateGuideStrandFromScalp(torch.from_numpy(pts.copy()), torch.from_numpy(nrm.copy()),
                                                                None, 0.8)
    world = solver.VoxelToWorld(strands, BUST)
    U.save_hair_strands(os.path.join(tmp, "scalp_segment.hair"), world)
    with contextlib.redirect_stderr(io.StringIO()):
        smooth = U.smooth_strands(list(world), 4.0, 2.0)
    U.save_hair_strands(os.path.join(tmp, "scalp_segment_smooth.hair"), smooth)
    out["num_root"] = np.int32(num_root)
    out["seg_hair"] = np.frombuffer(open(os.path.join(tmp, "scalp_segment.hair"), "rb").read(), np.uint8)
    out["seg_smooth_hair"] = np.frombuffer(open(os.path.join(tmp, "scalp_segment_smooth.hair"), "rb").read(), np.uint8)
    print("segments:", len(world), "roots:", num_root)

    # the connect_segments stage of __main__ (:925-952)
    segment, points = U.load_strand(os.path.join(tmp, "scalp_segment.hair"), return_strands=False)
    seg_strands = []
    beg = 0
    for i, seg in enumerate(segment):
        strand = points[beg:beg + seg]
        if i >= num_root:
            strand += BUST
        seg_strands.append(strand)
        beg += seg
    segs = seg_strands[num_root:]
    out.update({"shell_" + k: v for k, v in end_lists(segs, THR).items()})
    np.random.seed(1234)
    connected, table, draws, fail = run_connect(HairGrow, solver, segs)
    out["shell_next_random"] = np.float64(np.random.random())
    new_strands = seg_strands[:num_root] + [c - BUST for c in connected]
    with contextlib.redirect_stderr(io.StringIO()):
        new_strands = U.smooth_strands(new_strands, 4.0, 2.0)
    U.save_hair_strands(os.path.join(tmp, "strands.hair"), new_strands)
    out["shell_table"], out["shell_draws"], out["shell_fail"] = table, draws, np.int32(fail)
    pack("shell_out", connected, out)
    out["strands_hair"] = np.frombuffer(open(os.path.join(tmp, "strands.hair"), "rb").read(), np.uint8)
    print("shell: %d segments -> %d points, fail %d, retried %d, exhausted %d" %
          (len(segs), out["shell_out_pts"].shape[0], fail, int((draws > 0).sum()), int((draws == 50).sum())))

    # edge cases
    edge = edge_segments(np.random.default_rng(5)) + [s.copy() for s in segs[:200]]
    out.update({"edge_" + k: v for k, v in end_lists(edge, THR).items()})
    assert (out["edge_rr_idx"] >= 0).sum(1).max() == 50 or (out["edge_rr_idx"] >= 0).sum(1).max() == 49
    pack("edge_in", edge, out)
    np.random.seed(99)
    connected, table, draws, fail = run_connect(HairGrow, solver, edge)
    out["edge_next_random"] = np.float64(np.random.random())
    out["edge_table"], out["edge_draws"], out["edge_fail"] = table, draws, np.int32(fail)
    pack("edge_out", connected, out)
    print("edge: %d segments -> %d points, fail %d, retried %d, exhausted %d, cycles %d" %
          (len(edge), out["edge_out_pts"].shape[0], fail, int((draws > 0).sum()), int((draws == 50).sum()),
           int(sum(table[i, 1, 0] >= 0 for i in range(60, 68)))))
    shutil.rmtree(tmp)
    np.savez_compressed(os.path.join(OUT, "hair_connect.npz"), **out)
    print("hair_connect written: %.1f kB" % (os.path.getsize(os.path.join(OUT, "hair_connect.npz")) / 1024))


if __name__ == "__main__":
    main()
