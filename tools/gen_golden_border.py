"""Generate tests/golden/pmvo_border.npz by RUNNING THE REFERENCE ITSELF (imported read-only, CPU torch) on the case of
tests/border_cases.py: centres on the image edges, in the corners, one pixel either side of them, exact rounding ties and
degenerate projections, over maps that are random per pixel.  Recorded: project_points per view; Compute_Visible_and_Ori for
patch sizes 1, 3, 4, 7, 11 (the [V,N] results in full, the patch tensors on the pairs of border_cases.golden_pairs -- never an
interior pair is kept in place of a border one); the three filter index sets, for the batch and for the batch tiled to the size
of the lane-per-point vote kernel; forward (patch 7 and 11) in the original, the reversed and the doubled batch; the refine loss
of a fixed direction per point; and what this CPU's float -> long conversion makes of non-finite and out-of-range values, which
the reference's out_index and clamp lean on.  The file holds seeds, the code table, the reference's camera tensors, the points
and the results.

As tools/gen_golden_cascade.py: the work runs in a child process with ATEN_CPU_CAPABILITY=avx2; forward, the votes and the
refine loss run at 1 and at 8 threads and must agree.  Sensitivity: the numpy restatement of tests/border_cases.py must equal
the reference's full results, and each of its wrong rules must change a recorded result at every patch size it can affect.

    python tools/gen_golden_border.py
"""
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
CHILD = "MH_GEN_BORDER_CHILD"


def parent():
    env = dict(os.environ, ATEN_CPU_CAPABILITY="avx2")
    env[CHILD] = "1"
    raise SystemExit(subprocess.call([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))


if __name__ == "__main__" and not os.environ.get(CHILD):
    parent()

import numpy as np  # noqa: E402
import torch  # noqa: E402

sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

import border_cases as bc  # noqa: E402
import cascade_cases as cc  # noqa: E402
from ref_import import import_reference  # noqa: E402
from monohair_amd import synth  # noqa: E402
from monohair_amd.pmvo_utils import map_code_lut  # noqa: E402

THREADS = (1, 8)
FWD_PATCHES = (7, 11)
VOTE_PATCH = 7


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def at_threads(fn):
    res = []
    for t in THREADS:
        torch.set_num_threads(t)
        res.append(fn())
    for r in res[1:]:
        assert all(eq(x, y) for x, y in zip(res[0], r)), "the result depends on ATen's thread count"
    return res[-1]


def main():
    assert torch.backends.cpu.get_cpu_capability() == "AVX2", torch.backends.cpu.get_cpu_capability()
    os.makedirs(OUT, exist_ok=True)
    os.chdir("/tmp")
    torch.manual_seed(0)
    R = import_reference(gabor=False)
    from scipy.spatial import KDTree

    lut = map_code_lut()
    cams_list = bc.cameras()
    k8, c8, m8, depth = bc.code_maps()
    maps = bc.decode(lut, k8, c8, m8, depth)
    pts, target, tags = bc.build_points(cams_list, depth)
    N = len(pts)
    Cam = R["Camera_utils"].Camera
    ref_cams = [Cam(c["ndc_prj"], np.linalg.inv(np.array(c["pose"])), c["file"]) for c in cams_list]
    out = dict(seed=np.int64(bc.SEED), lut=lut, points=pts, target=target, tags=tags.astype("U1"), map_sums=bc.map_checksums(maps),
               cam_pose=np.stack([c.pose.numpy() for c in ref_cams]), cam_proj=np.stack([c.proj.numpy() for c in ref_cams]),
               cam_rinv=np.stack([torch.linalg.inv(c.pose[:3, :3]).numpy() for c in ref_cams]))
    rec = np.zeros((bc.V, 48), np.float32)
    rec[:, 0:16], rec[:, 16:32], rec[:, 32:41] = (out[k].reshape(bc.V, -1) for k in ("cam_pose", "cam_proj", "cam_rinv"))
    classes = bc.classify(rec, pts)
    counts = {k: int(v.sum()) for k, v in classes.items()}
    empty = [k for k, n in counts.items() if n == 0]
    assert not empty, "empty classes: %s" % empty
    tie = tags == "c"
    _, o_zp, o_oob, pixf = bc.project(rec, pts)
    assert np.array_equal(pixf[bc.HAND][tie].astype(np.float64), target[tie, 1:3]), "the ties are not exact"
    pairs = bc.golden_pairs(classes, target, tags)
    out["pairs"] = pairs

    def make_pmvo(patch):
        scene = dict(cams=[dict(file=c["file"]) for c in cams_list], **{k: torch.from_numpy(v) for k, v in maps.items()})
        depths, Ori, Conf, masks = synth.scene_to_reference_dicts(scene)
        return R["PMVO"].PMVO({c.id: c for c in ref_cams}, depths, Ori, Conf, masks, device="cpu", image_size=[bc.H, bc.W],
                              patch_size=patch, visible_threshold=bc.VIS_THR, conf_threshold=bc.THR)

    tp = torch.from_numpy(pts).type(torch.float)
    # ---- what this CPU's float -> long conversion does (PMVO.py:383), alone and inside a long tensor (vector and scalar loops)
    probe = np.array([np.nan, np.inf, -np.inf, 1e30, -1e30, 2.0 ** 63, -2.0 ** 63, np.float32(2.0 ** 63) * (1 - 2.0 ** -24),
                      2.0 ** 31, -2.0 ** 31 - 256, 3e9, -0.0, 0.5, 1.5, 2.5, -0.5, -1.5], np.float32)
    cast = torch.round(torch.from_numpy(probe)).type(torch.long).numpy()
    long_in = np.concatenate([np.zeros(61, np.float32), probe, np.zeros(67, np.float32)])
    assert np.array_equal(torch.round(torch.from_numpy(long_in)).type(torch.long).numpy()[61:61 + len(probe)], cast)
    for a, b in zip(probe, cast):
        print("round(%r).long() = %d" % (float(a), int(b)))
    out["cast_in"], out["cast_out"] = probe, cast

    # ---- project_points per view
    pm = make_pmvo(1)
    uv, zp, oob = [], [], []
    for cam in ref_cams:
        a, b, c = pm.project_points(tp, cam, [bc.H, bc.W])
        uv.append(a.numpy().astype(np.int32)), zp.append(b.numpy().copy()), oob.append(c.numpy().copy())
    out["uv"], out["zp"], out["out_index"] = np.stack(uv), np.stack(zp), np.stack(oob)
    assert eq(out["zp"], o_zp), "the oracle's z' is not the reference's: the sensitivity check would start from other inputs"

    # ---- Compute_Visible_and_Ori per patch size
    want = {}
    for patch in bc.PATCHES:
        pm = make_pmvo(patch)
        pm.Compute_Visible_and_Ori(tp)
        want[patch] = {k: getattr(pm, k).numpy().copy() for k in bc.RESULT_KEYS}
        for k in ("visible", "Ori", "Conf", "mask"):
            assert eq(want[patch][k], want[bc.PATCHES[0]][k])
        for k in ("Ori_patch", "Conf_patch"):
            out["p%d_%s" % (patch, k)] = want[patch][k][pairs[:, 0], pairs[:, 1]]
    for k in ("visible", "Ori", "Conf", "mask"):
        out[k] = want[bc.PATCHES[0]][k]
    report = bc.sensitivity(pixf, o_zp, maps, want)
    for rule, ch in report.items():
        print("wrong rule %-18s changes %s" % (rule, {p: ",".join(v) for p, v in ch.items()}))

    # ---- votes, refine loss (patch 7), forward (patch 7 and 11)
    bust, scalp = cc.toy_head()
    R["PMVO"].bust_tree, R["PMVO"].scalp_tree = KDTree(data=bust), KDTree(data=scalp)
    R["PMVO"].scalp_max = np.max(scalp, axis=0)
    pm = make_pmvo(VOTE_PATCH)
    tiled = torch.from_numpy(np.tile(pts, (bc.TILE, 1))).type(torch.float)
    rows = np.flatnonzero(np.isfinite(pts).all(1)).astype(np.int32)      # (scipy's tree refuses non-finite queries)
    dirs = cc.directions(N, bc.SEED)
    tr, td = torch.from_numpy(pts[rows]).type(torch.float), torch.from_numpy(dirs[rows])

    def votes():
        res = []
        for t in (tp, tiled):
            sidx, _, fidx = pm.filter_points(t)
            res += [sidx.numpy().copy(), fidx.numpy().copy(), pm.compute_unvisible_points(t).numpy().copy()]
        return tuple(res) + (pm.refine(tr, td).numpy().copy(),)

    v = at_threads(votes)
    for k, a in zip(("surface_index", "filter_index", "unvisible_index", "tiled_surface_index", "tiled_filter_index",
                     "tiled_unvisible_index", "refine_loss"), v):
        out[k] = a
    out["refine_rows"], out["dirs"] = rows, dirs
    for patch in FWD_PATCHES:
        pm = make_pmvo(patch)

        def fwd(p=pts):
            _, so, ml, hc = pm.forward(p)
            bidx, bval = pm.Find_max_conf_from_visible_view()
            return so.numpy().copy(), ml.numpy().copy(), hc.numpy().copy(), bidx.numpy().astype(np.int32), bval.numpy().copy()

        f = at_threads(fwd)
        rev = tuple(a[::-1].copy() for a in fwd(pts[::-1].copy())[:3])
        dup = fwd(np.concatenate([pts, pts], 0))
        assert all(eq(a[:N], a[N:]) for a in dup[:3])
        pre = "f%d_" % patch
        for k, a in zip(("fwd_ori", "fwd_loss", "fwd_hc", "base_idx", "base_val"), f):
            out[pre + k] = a
        for tag, res in (("rev", rev), ("dup", tuple(a[:N] for a in dup[:3]))):
            for k, a in zip(("ori", "loss", "hc"), res):
                out[pre + "%s_%s" % (tag, k)] = a
        print("forward patch %d: %d finite losses, %d rows differ reversed, %d doubled" % (
            patch, int(np.isfinite(f[1]).sum()), int((~((rev[1] == f[1]) | (np.isnan(rev[1]) & np.isnan(f[1])))).sum()),
            int((~((dup[1][:N] == f[1]) | (np.isnan(dup[1][:N]) & np.isnan(f[1])))).sum())))
    meta = dict(H=bc.H, W=bc.W, V=bc.V, N=N, seed=bc.SEED, thr=bc.THR, vis_thr=bc.VIS_THR, patches=list(bc.PATCHES),
                fwd_patches=list(FWD_PATCHES), vote_patch=VOTE_PATCH, tile=bc.TILE, torch=torch.__version__,
                capability=torch.backends.cpu.get_cpu_capability(), threads=list(THREADS), class_counts=counts,
                stored_pairs=int(len(pairs)),
                wrong_rules={r: {p: list(v) for p, v in ch.items()} for r, ch in report.items()},
                cast_rule="round(x).long() of NaN, +-inf and |x| >= 2^63 is INT64_MIN on this CPU (x86 conversion): negative, "
                          "so the pair is out of bounds and its centre clamps to row / column 0")
    print("class counts", counts)
    print("stored pairs", len(pairs), "finite refine rows", len(rows))
    path = os.path.join(OUT, "pmvo_border.npz")
    np.savez_compressed(path, meta=np.array(repr(meta)), **out)
    print("pmvo_border.npz: %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
