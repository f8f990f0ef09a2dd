"""Golden vectors of the scalp attachment stage (tests/golden/hair_scalp.npz), run by the imported reference.

    python tools/gen_golden_scalp.py

Case "shell": the connect_scalp stage of HairGrow.py's __main__ (:954-976) on the strands.hair that case "shell" of
hair_connect.npz records (299 rooted and 848 floating strands on the same synthetic 256x256x192 volume, which is read from
that file and not stored again): WorldToVoxel, connect_to_scalp, back to world units, smoothing, connected_strands.hair.
Case "edge": connect_to_scalp on hand-made strands that land on every branch (edge_strands below).

Recorded per case: per pass the thresholds and the rooted / out counts after it; the final flags, out_ratio, flip parity,
the neighbour strand and point index of the last join per strand, random_move_strands' orientation score per join, the
returned strands; for "shell" the bytes of connected_strands.hair.  The numpy restatement of tests/test_hair_scalp_host.py
is run alongside: it must reproduce the reference's run, report no exact tie in a nearest-point distance or between two
losses (scipy's answer at such a tie follows its tree layout), no decision within rounding of its threshold, and -- for
"edge" -- every family of edge_strands.  If an assertion fails, change the seed or the hand-made coordinates.

points_to_voxel is wrapped to clone its input (tools/gen_golden_connect.py explains why).
"""
import contextlib
import io
import os
import shutil
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

from ref_import import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
RATIO = {"shell": 0.2, "edge": 0.0}       # HairGenerate.out_ratio differs per case in the reference's configs (0 .. 0.5)


def line(p0, d, n, step=1.0):
    d = np.asarray(d, np.float64)
    return np.asarray(p0, np.float64) + np.outer(np.arange(n) * step, d / np.linalg.norm(d))


def edge_strands(rng):
    """(strands, num_root).  Rooted strands are straight lines with unit steps; a floating strand starts beside point k of
    one and runs on with steps of 3 and more, so that the mean nearest distance of its first points is >= 1."""
    roots, floats = [], []
    j = lambda a: a + rng.normal(scale=1e-3, size=a.shape)          # noqa: E731  (no exact ties)

    def beside(root, k, off, d=(3.0, 1.0, 0.0), n=6):
        return j(line(root[k] + np.array([0.0, off, 0.0]), d, n, np.linalg.norm(d)))

    # nearest indices 0, 1, 2 (and a plain join at 5)
    for k, y in ((0, 20.0), (1, 30.0), (2, 40.0), (5, 50.0)):
        r = j(line([30.0, y, 30.0], [1, 0, 0], 12))
        roots.append(r)
        floats.append(beside(r, k, 0.3))
    # floating strands of 2 and 4 points
    for n, y in ((2, 60.0), (4, 70.0)):
        r = j(line([30.0, y, 30.0], [1, 0, 0], 12))
        roots.append(r)
        floats.append(beside(r, 5, 0.3, (4.0, 2.0, 0.0), n))
    # balls with exactly 30 and with 34 distinct strands, each more than one wave's worth of points at the wider radii
    for cnt, y in ((30, 90.0), (34, 110.0)):
        for t in range(cnt):
            a = 2 * np.pi * t / cnt
            roots.append(j(line([30.0, y + 0.35 * np.cos(a), 30.0 + 0.35 * np.sin(a)], [1, 0, 0], 12)))
        floats.append(j(line([35.0, y, 30.0], [3.0, 1.0, 0.3], 6, 3.2)))
    # an empty ball
    floats.append(j(line([200.0, 200.0, 150.0], [1, 0, 0], 8)))
    # a core point at exactly thr_dist = 0.5 (no jitter): joins only once the radius has grown
    roots.append(line([50.5, 135.0, 40.0], [0, 1, 0], 12))
    floats.append(line([50.0, 140.0, 40.0], [1.0, 3.0, 0.0], 6, 3.2))
    # len > 60 and len + idx > 150
    r = j(line([20.0, 150.0, 60.0], [1, 0, 0], 130))
    roots.append(r)
    floats.append(beside(r, 100, 0.3, (3.0, 1.0, 0.0), 62))
    # must flip: runs against its neighbour, its start further along it than its end; one that can join afterwards
    r = j(line([30.0, 170.0, 30.0], [1, 0, 0], 14))
    roots.append(r)
    floats.append(j(np.array([[38.0, 170.3, 30], [35.0, 171.3, 30], [32.0, 172.3, 30], [29.0, 173.3, 30]])))
    r = j(line([30.0, 180.0, 30.0], [1, 0, 0], 14))
    roots.append(r)
    floats.append(j(np.array([[38.0, 180.3, 30], [36.0, 182.2, 30], [34.0, 182.2, 30], [32.0, 180.3, 30]])))
    # the joined part leaves the 256 x 256 x 192 box
    r = j(line([262.0, 100.0, 50.0], [-1, 0, 0], 20))
    roots.append(r)
    floats.append(beside(r, 10, 0.3, (-3.0, 1.0, 0.0)))
    # runs alongside its neighbour: mean nearest distance of its first points < 1
    r = j(line([30.0, 210.0, 30.0], [1, 0, 0], 12))
    roots.append(r)
    floats.append(beside(r, 5, 0.3, (1.0, 0.0, 0.0)))
    # beside the 34 lines at too wide an angle to join: at the widest radius its ball holds more than 64 points (more
    # than one wave's worth)
    floats.append(j(line([38.0, 111.0, 30.0], [3.0, 5.0, 0.0], 6, 5.8)))
    # connects only at (2.0, 0.6)
    r = j(line([30.0, 200.0, 30.0], [1, 0, 0], 12))
    roots.append(r)
    floats.append(beside(r, 5, 1.9, (3.0, 3.8, 0.0)))
    return [s.astype(np.float32) for s in roots + floats], len(roots)


def run_reference(HairGrow, solver, strands, num_root, ratio):
    """connect_to_scalp with every join traced: -> dict of the recorded quantities"""
    n = len(strands)
    original = [s.copy() for s in strands]
    HairGrow.args.HairGenerate.out_ratio = ratio
    cur = {"i": -1}
    root, out = np.zeros(n, bool), np.zeros(n, bool)
    root[:num_root] = True
    out_ratio = np.zeros(n)
    choice = np.full((n, 2), -1, np.int32)
    sims = np.zeros(n, np.float32)

    def tq(it):
        for i in it:
            cur["i"] = i
            yield i

    orig_rms, orig_tqdm = HairGrow.random_move_strands, HairGrow.tqdm

    def rms(strand, occ, ori, threshold=0.4, index=-1):
        res = orig_rms(strand, occ, ori, threshold, index=index)
        i, m = cur["i"], index - 1
        s0 = strands[i][0]         # the reference has already stored the flipped strand
        hit = [k for k in np.flatnonzero(root) if len(strands[k]) > m and
               np.array_equal(s0 * 0.95 + strands[k][m] * 0.05, strand[m]) and
               np.array_equal(strand[m] + (strands[k][m - 1] - strands[k][m]), strand[m - 1])]
        assert len(hit) == 1, (i, hit)
        choice[i] = (hit[0], m)
        # the score the reference compares with 0.3, by the same torch calls on the same tensors
        ss = torch.from_numpy(strand.copy()[:index])
        so = torch.cat([ss[1:] - ss[:-1], ss[-1:] - ss[-2:-1]], 0)
        idx = torch.round(ss).type(torch.long)
        if not (idx[:, 2].max() >= 192 or (idx[:, 1] >= 256).any() or (idx[:, 0] >= 256).any()):
            o = ori[:, idx[:, 2], idx[:, 1], idx[:, 0]].permute(1, 0)
            s1 = torch.maximum(torch.cosine_similarity(-o, so, dim=-1), torch.cosine_similarity(o, so, dim=-1))
            sims[i] = float(torch.sum(s1) / torch.sum(occ[0, idx[:, 2], idx[:, 1], idx[:, 0]]))
        out_ratio[i] = float(res[2])
        pending.append((i, bool(res[1])))
        return res

    pending = []
    HairGrow.random_move_strands, HairGrow.tqdm = rms, tq
    buf = io.StringIO()
    passes = []
    try:
        # the flags of a pass take effect when it ends: apply `pending` whenever the reference prints a new pass header
        class Tap(io.StringIO):
            def write(self, s):
                if s.startswith("iter:") or s.startswith("done"):
                    for i, ok in pending:
                        (root if ok else out)[i] = True
                    del pending[:]
                return buf.write(s)

        with contextlib.redirect_stdout(Tap()):
            ret = solver.connect_to_scalp(strands, num_root)
    finally:
        HairGrow.random_move_strands, HairGrow.tqdm = orig_rms, orig_tqdm
    lines = buf.getvalue().splitlines()
    good = [int(float(l.split(":")[1])) for l in lines if l.startswith("num of good strands:")][1:]
    outs = [int(float(l.split(":")[1])) for l in lines if l.startswith("num of out strands:")]
    td = [float(l.split(":")[1]) for l in lines if l.startswith("current thr_dist:")]
    tdot = [float(l.split(":")[1]) for l in lines if l.startswith("current thr_dot:")]
    for k in range(len(td)):       # counts AFTER pass k = the header of pass k+1, or the final flags
        passes.append((td[k], tdot[k], good[k + 1] if k + 1 < len(td) else int(root.sum()),
                       outs[k + 1] if k + 1 < len(td) else int(out.sum())))
    flipped = np.array([0 if np.array_equal(strands[i][-len(original[i]):], original[i]) else 1 for i in range(n)], np.int32)
    for i in range(n):
        assert np.array_equal(strands[i][-len(original[i]):], original[i][::-1] if flipped[i] else original[i])
    assert len(ret) == int((root | out).sum())
    return dict(passes=np.array(passes, np.float64), root=root, out=out, out_ratio=out_ratio, flipped=flipped,
                choice=choice, similar=sims, returned=ret)


def record(out, tag, rec, num_root, ratio):
    for k in ("passes", "root", "out", "out_ratio", "flipped", "choice", "similar"):
        out["%s_%s" % (tag, k)] = rec[k]
    out[tag + "_ret_len"] = np.array([s.shape[0] for s in rec["returned"]], np.int32)
    out[tag + "_ret_pts"] = np.concatenate(rec["returned"], 0).astype(np.float32)
    out[tag + "_num_root"], out[tag + "_ratio_thr"] = np.int32(num_root), np.float64(ratio)


def main():
    import_reference()
    os.chdir("/tmp")
    import scipy
    import scipy.io

    import HairGrow
    import Utils.Utils as U
    from test_hair_scalp_host import check_recorded, load_volume, rs_connect, similar_close

    orig_ptv = HairGrow.points_to_voxel
    HairGrow.points_to_voxel = lambda p: orig_ptv(p.clone())
    HairGrow.args = types.SimpleNamespace(PMVO=types.SimpleNamespace(infer_inner=False), device="cpu",
                                          HairGenerate=types.SimpleNamespace(out_ratio=0.0))
    zc = np.load(os.path.join(OUT, "hair_connect.npz"))
    occ, ori, vox = load_volume(zc)
    tmp = tempfile.mkdtemp(prefix="mh_hs_")
    G = tuple(int(g) for g in zc["vol_shape"])
    o = ori.transpose(2, 1, 0, 3).transpose((0, 1, 3, 2)).reshape(G[0], G[1], G[2] * 3).transpose((1, 0, 2))
    scipy.io.savemat(os.path.join(tmp, "Ori3D.mat"), {"Ori": o})
    scipy.io.savemat(os.path.join(tmp, "Occ3D.mat"), {"Occ": occ[..., 0].transpose(2, 1, 0).transpose((1, 0, 2))})
    solver = HairGrow.HairGrowing(os.path.join(tmp, "Occ3D.mat"), os.path.join(tmp, "Ori3D.mat"), device="cpu")
    assert np.array_equal(solver.occ[0].numpy(), vox[..., 3]) and np.array_equal(solver.ori.permute(1, 2, 3, 0).numpy(), vox[..., :3])
    out = dict(meta=np.array("numpy %s, scipy %s, torch %s" % (np.__version__, scipy.__version__, torch.__version__)))
    bust = zc["bust"]

    # ---- shell: the connect_scalp stage of __main__ (:954-976)
    with open(os.path.join(tmp, "strands.hair"), "wb") as f:
        f.write(zc["strands_hair"].tobytes())
    num_root = int(zc["num_root"])
    _, _, strands, _ = U.load_strand(os.path.join(tmp, "strands.hair"), return_strands=True)
    strands = solver.WorldToVoxel(strands, bust)
    shell_in = [s.copy() for s in strands]
    rec = run_reference(HairGrow, solver, strands, num_root, RATIO["shell"])
    world = []
    for ss in rec["returned"]:
        w = HairGrow.voxel_to_points(torch.from_numpy(ss.copy())).cpu().numpy()
        w -= bust
        world.append(w)
    with contextlib.redirect_stderr(io.StringIO()):
        world = U.smooth_strands(world, 4.0, 2.0)
    U.save_hair_strands(os.path.join(tmp, "connected_strands.hair"), world)
    record(out, "shell", rec, num_root, RATIO["shell"])
    out["connected_strands_hair"] = np.frombuffer(open(os.path.join(tmp, "connected_strands.hair"), "rb").read(), np.uint8)

    # ---- edge
    edge, edge_root = edge_strands(np.random.default_rng(7))
    out["edge_in_len"] = np.array([s.shape[0] for s in edge], np.int32)
    out["edge_in_pts"] = np.concatenate(edge, 0)
    rec_e = run_reference(HairGrow, solver, [s.copy() for s in edge], edge_root, RATIO["edge"])
    record(out, "edge", rec_e, edge_root, RATIO["edge"])
    shutil.rmtree(tmp)

    # ---- the restatement reproduces both runs and reports no tie and no decision at its threshold
    for tag, inp, nr in (("shell", shell_in, num_root), ("edge", edge, edge_root)):
        res = rs_connect(inp, nr, vox, RATIO[tag])
        check_recorded(out, tag, res)
        st = res["stats"]
        print(tag, "passes", len(res["passes"]), "rooted", int(res["root"].sum()), "out", int(res["out"].sum()), dict(st))
        for k in ("nearest_ties", "loss_ties", "similar_near_0.3", "mean_near_5", "dist_near_thr"):
            assert st[k] == 0, (tag, k, st[k])
        joined = out[tag + "_choice"][:, 0] >= 0
        d = np.abs(res["similar"][joined] - out[tag + "_similar"][joined])
        print(tag, "similar: largest finite difference", np.nanmax(np.where(np.isfinite(d), d, 0)))
        assert similar_close(res["similar"][joined], out[tag + "_similar"][joined])
        if tag == "edge":
            for k in ("ball_distinct_0", "ball_distinct_1", "ball_distinct_30", "ball_distinct_>30", "on_radius",
                      "len_2_joined", "len_4_joined", "refused_long", "nearest_index_0", "nearest_index_1",
                      "nearest_index_2", "flipped", "left_box", "stopped_at_30", "refused_mean", "ball_gt64"):
                assert st[k] > 0, k
            assert res["passes"][-1][:2] == (2.0, 0.6) and (len(edge) - edge_root) // 500 == 0
            last = len(edge) - 1       # the strand that joins only at the widest thresholds
            assert res["choice"][last, 0] >= 0 and len(res["passes"]) >= 7
        else:
            assert (len(inp) - nr) // 500 == 1
    np.savez_compressed(os.path.join(OUT, "hair_scalp.npz"), **out)
    print("hair_scalp written: %.1f kB" % (os.path.getsize(os.path.join(OUT, "hair_scalp.npz")) / 1024))


if __name__ == "__main__":
    main()
