"""Generate tests/golden/pmvo_softmask.npz by RUNNING THE REFERENCE ITSELF (imported read-only, CPU torch) on the cases of
tests/softmask_cases.py: soft hair masks (codes 0 / 49 / 50 / 51 / 52 / 255, and a float palette around 0.2f), confidences on the
threshold codes, depth gaps that equal 0.1f / 0.9f / 1.0 exactly and one ulp either side, at 24 and at 272 views.  Recorded per
view count and palette: the three filter sets and compute_unvisible_points at conf_threshold 0.4 and 0.2 and patch 3 and 5, for
the batch, the batch tiled to the size of the lane-per-point vote kernel and batches of one point; filter_head_points at
visible_threshold 1.0 and 0.1; PMVO.refine's loss; Compute_Visible_and_Ori's visible / Conf / mask (the last 24 views at 272);
and forward (patch 3 and 5) for the batch and the batches of one, for the tiled batch at TILED_FORWARD.  The file holds seeds, the code table, the reference's
camera tensors, the points and the results.

As tools/gen_golden_border.py: the work runs in a child process with ATEN_CPU_CAPABILITY=avx2; the votes and the refine loss run
at 1 and at 8 threads and must agree.  Conditions asserted on the case: every tie family occurs, the numpy restatement of the
votes equals the reference on every row, and the rows whose decision changes under another summation order or the opposite
operator of each rule are counted (tests/softmask_cases.py: sensitivity); what the case cannot tell apart is printed and
stored under meta["indistinguishable"].

    python tools/gen_golden_softmask.py
    python tools/gen_golden_softmask.py --search 29 30 31 32 33 34     # how softmask_cases.SEED was chosen
"""
import os
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
CHILD = "MH_GEN_SOFTMASK_CHILD"


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
import softmask_cases as sc  # noqa: E402
from ref_import import import_reference  # noqa: E402
from monohair_amd import synth  # noqa: E402
from monohair_amd.pmvo_utils import map_code_lut  # noqa: E402

THREADS = (1, 8)
TILED_FORWARD = (24, 0.4, 3)      # forward of the tiled batch (4368 points): this view count, threshold and patch only
HEAD_VIS = (1.0, 0.1)
KEPT_VIEWS = 24          # Compute_Visible_and_Ori's [V,N] results are stored for the last 24 views


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
    base_cams = bc.cameras()
    Cam = R["Camera_utils"].Camera
    ref24 = [Cam(c["ndc_prj"], np.linalg.inv(np.array(c["pose"])), c["file"]) for c in base_cams]
    out = dict(seed=np.int64(sc.SEED), lut=lut, cam_pose=np.stack([c.pose.numpy() for c in ref24]),
               cam_proj=np.stack([c.proj.numpy() for c in ref24]),
               cam_rinv=np.stack([torch.linalg.inv(c.pose[:3, :3]).numpy() for c in ref24]))
    rec24 = sc.records24(out)
    bust, scalp = cc.toy_head()
    R["PMVO"].bust_tree, R["PMVO"].scalp_tree = KDTree(data=bust), KDTree(data=scalp)
    R["PMVO"].scalp_max = np.max(scalp, axis=0)
    meta = dict(H=sc.H, W=sc.W, seed=sc.SEED, thrs=list(sc.THRS), vis_thr=sc.VIS_THR, patches=list(sc.PATCHES), tiled_forward=list(TILED_FORWARD),
                tile=sc.TILE, head_vis=list(HEAD_VIS), kept_views=KEPT_VIEWS, torch=torch.__version__,
                capability=torch.backends.cpu.get_cpu_capability(), threads=list(THREADS), cases={})
    for V in sc.VIEW_COUNTS:
        case = sc.build(rec24, V)
        pts, N = case["points"], len(case["points"])
        assert N * sc.TILE >= 4096 and N % 32 and (N * sc.TILE) % 32
        rec = sc.view_records(rec24, V)
        cams_list = sc.camera_list(V)
        ref_cams = [Cam(c["ndc_prj"], np.linalg.inv(np.array(c["pose"])), c["file"]) for c in cams_list]
        hands = np.flatnonzero(np.arange(V) % sc.NCAM == sc.HAND)
        pre = "v%d_" % V
        out[pre + "points"], out[pre + "tags"], out[pre + "info"] = pts, case["tags"].astype("U1"), case["info"]
        dirs = cc.directions(N, sc.SEED)
        out[pre + "dirs"] = dirs
        comps = sc.compositions(case)
        info = dict(N=N, palettes={})
        for pal in sc.PALETTES:
            maps = sc.decode(lut, case, pal)
            out[pre + pal + "_map_sums"] = sc.map_checksums(maps)
            pp = pre + pal + "_"

            def make_pmvo(patch, thr, vis_thr=sc.VIS_THR):
                scene = dict(cams=[dict(file=c["file"]) for c in cams_list], **{k: torch.from_numpy(v) for k, v in maps.items()})
                depths, Ori, Conf, masks = synth.scene_to_reference_dicts(scene)
                return R["PMVO"].PMVO({c.id: c for c in ref_cams}, depths, Ori, Conf, masks, device="cpu", image_size=[sc.H, sc.W],
                                      patch_size=patch, visible_threshold=vis_thr, conf_threshold=thr)

            tp = torch.from_numpy(pts).type(torch.float)
            pm = make_pmvo(sc.PATCHES[0], sc.THRS[0])
            pm.Compute_Visible_and_Ori(tp)
            cvo = {k: getattr(pm, k).numpy().copy() for k in ("visible", "Conf", "mask")}
            for k, a in cvo.items():
                out[pp + k] = a[-KEPT_VIEWS:]
            # the case's own arithmetic against the reference's: projection, gap, mask
            t3 = sc.pair_terms(rec, pts, case, maps, 3)
            for v in (0, int(hands[0]), V - 1):
                uv, z, oob = pm.project_points(tp, ref_cams[v], [sc.H, sc.W])
                assert eq(oob.numpy(), t3["oob"][v]) and eq((z * 255 - pm.get_depth(uv, pm.camera_key[v])).numpy(), t3["gap"][v])
                assert eq(pm.get_mask(uv, pm.camera_key[v]).numpy(), t3["m"][v])
            gaps = sc.gap_families(t3, case["tags"], case["info"], hands)
            assert min(gaps.values()) > 0, gaps
            pinfo = dict(gap_families=gaps, combos={})
            for vt in HEAD_VIS:
                ph = make_pmvo(sc.PATCHES[0], sc.THRS[0], vt)
                for name, p in comps.items():
                    got = at_threads(lambda: (ph.filter_head_points(torch.from_numpy(p).type(torch.float), vt).numpy().copy(),))[0]
                    out[pp + "head%g_%s" % (vt, name)] = got
                    want = sc.votes(sc.vote_terms(sc.pair_terms(rec, p, case, maps, 3), sc.THRS[0], vt))[3] & ~cc.head_top(p, scalp)
                    assert eq(got, want), "the restated head vote differs from the reference"
            for thr in sc.THRS:
                for patch in sc.PATCHES:
                    pm = make_pmvo(patch, thr)
                    key = pp + "t%dp%d_" % (sc.thr_code(thr), patch)
                    for name, p in comps.items():
                        t = torch.from_numpy(p).type(torch.float)

                        def run():
                            sidx, _, fidx = pm.filter_points(t)
                            return sidx.numpy().copy(), fidx.numpy().copy(), pm.compute_unvisible_points(t).numpy().copy()

                        got = at_threads(run)
                        for k, a in zip(("surface", "filter", "unvisible"), got):
                            out[key + k + "_" + name] = a
                        want = sc.votes(sc.vote_terms(sc.pair_terms(rec, p, case, maps, patch), thr))
                        assert all(eq(a, b) for a, b in zip(got, want[:3])), "the restated votes differ from the reference"
                        if name != "tiled":
                            dr = dirs if name == "batch" else dirs[case["singles"][int(name[3:])]][None]
                            out[key + "refine_" + name] = at_threads(lambda: (pm.refine(t, torch.from_numpy(dr)).numpy().copy(),))[0]
                    tpatch = sc.pair_terms(rec, pts, case, maps, patch)
                    fam = sc.families(tpatch, cvo["visible"], thr)
                    assert min(fam.values()) > 0 or patch != 3, fam     # (the painted windows are 3 x 3)
                    rep = sc.sensitivity(tpatch, thr, N)
                    pinfo["combos"]["t%dp%d" % (sc.thr_code(thr), patch)] = dict(families=fam, sensitivity=rep)
                    print(V, pal, thr, patch, fam, rep)
                torch.set_num_threads(THREADS[-1])
                for patch in sc.PATCHES:
                    pm = make_pmvo(patch, thr)
                    key = pp + "t%dp%d_" % (sc.thr_code(thr), patch)
                    for name, p in comps.items():
                        if name == "tiled" and (V, thr, patch) != TILED_FORWARD:
                            continue
                        t0 = time.time()
                        _, so, ml, hc = pm.forward(p)
                        bidx, bval = pm.Find_max_conf_from_visible_view()
                        for k, a in zip(("fwd_ori", "fwd_loss", "fwd_hc", "base_idx", "base_val"),
                                        (so.numpy(), ml.numpy(), hc.numpy(), bidx.numpy().astype(np.int32), bval.numpy())):
                            out[key + k + "_" + name] = a.copy()
                        if name in ("batch", "tiled"):
                            print(V, pal, thr, patch, name, "forward: %.1f s, %d finite losses, %d high-confidence rows" % (
                                time.time() - t0, int(np.isfinite(ml.numpy()).sum()), int(hc.numpy().sum())), flush=True)
                if pal == sc.PALETTES[0]:        # (the search reads no mask: once per view count and threshold)
                    pm = make_pmvo(sc.PATCHES[0], thr)
                    pm.Compute_Visible_and_Ori(tp)
                    bidx, _ = pm.Find_max_conf_from_visible_view()
                    samp, surf = pm.sample_next_3d_pos(tp, bidx[0])
                    D = pm.compute_reproject_ori(surf, samp)
                    _, index, hc = pm.compute_prj_loss(D, pm.Ori, pm.compute_weight(pm.visible, pm.Conf, pm.mask))
                    srep = sc.search_sensitivity(D.numpy(), pm.Ori_patch.numpy(), pm.Conf_patch.numpy(), pm.visible.numpy(), thr,
                                                 index.numpy(), hc.numpy())
                    info.setdefault("search", {})["t%d" % sc.thr_code(thr)] = srep
                    print(V, thr, "search, first base view:", srep, flush=True)
            info["palettes"][pal] = pinfo
        meta["cases"][V] = info
    # what the fixture can and cannot tell apart, over every case
    found, miss = {}, []
    for V, info in meta["cases"].items():
        for pal, pinfo in info["palettes"].items():
            for combo in pinfo["combos"].values():
                for k, n in combo["sensitivity"].items():
                    found[k] = found.get(k, 0) + (sum(n.values()) if isinstance(n, dict) else n)
        for srep in info["search"].values():
            for k, n in srep.items():
                if k.startswith("op_search_") or k in ("weight_on_thr", "positive_4", "positive_5"):
                    found[k] = found.get(k, 0) + n
            # (numpy rounds the cosine otherwise than ATen: a near-tie of two samples can pick another index.  Such rows are
            # left out of the proof; they must stay few)
            assert srep["agree"] >= 0.95 * srep["rows"], "the restated search loss differs from the reference's (index, flag)"
    for k, n in sorted(found.items()):
        print("%-24s rows whose recorded decision changes: %d" % (k, n))
        if n == 0 and "unvisible" not in k:          # (the unvisible vote sums 0 / 1 only: no order can change it)
            miss.append(k)
    meta["sensitive_rows"], meta["indistinguishable"] = found, miss
    for need in ("order_main_surface", "order_main_filter", "order_main_head", "order_tail_surface", "order_tail_filter",
                 "order_tail_head", "op_gap01", "op_gap_vis", "op_gap09", "op_cmax", "op_mask", "op_gap_head", "op_search_cmax",
                 "op_search_tap", "op_search_weight", "weight_on_thr"):
        assert found[need] > 0, need
    print("indistinguishable with this family of cases:", miss)
    path = os.path.join(OUT, "pmvo_softmask.npz")
    np.savez_compressed(path, meta=np.array(repr(meta)), **out)
    print("pmvo_softmask.npz: %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


def search(seeds):
    """the family of cases over seeds (placements of the fractional views, points, maps): rows whose decision changes per order
    and vote rule, summed over view counts and palettes at conf_threshold 0.4, patch 3.  No reference needed."""
    from monohair_amd.camera import camera_records, cameras_from_list

    rec24, lut = camera_records(cameras_from_list(bc.cameras())), map_code_lut()
    for seed in seeds:
        tot = {}
        for V in sc.VIEW_COUNTS:
            case = sc.build(rec24, V, seed)
            for pal in sc.PALETTES:
                t = sc.pair_terms(sc.view_records(rec24, V), case["points"], case, sc.decode(lut, case, pal), 3)
                for k, n in sc.sensitivity(t, sc.THRS[0], len(case["points"])).items():
                    tot["%d:%s" % (V, k)] = tot.get("%d:%s" % (V, k), 0) + (sum(n.values()) if isinstance(n, dict) else n)
        print(seed, tot, flush=True)


if __name__ == "__main__":
    if "--search" in sys.argv:
        search([int(a) for a in sys.argv[sys.argv.index("--search") + 1:]])
    else:
        main()
