"""Generate tests/golden/cascade_views.npz and tests/golden/consensus_levels.npz by RUNNING THE REFERENCE ITSELF (imported
read-only, CPU torch) at the sizes where ATen's cascade sums take up another level: sums over 255 .. 4095 views, means over
groups of 127 .. 9728 members.  The inputs are regenerated from seeds by tests/cascade_cases.py; the files hold the seeds,
the 24 base views, the reference's camera tensors and the reference's results.

The project pins ATen's AVX2 summation order (8 floats per vector), so the work runs in a child process with
ATEN_CPU_CAPABILITY=avx2, which asserts that capability.  Every case runs at 1 and at 8 threads and must agree (the point
counts in tests/cascade_cases.py are chosen so that ATen's split over threads does not move a column into another order).
Sensitivity: every sum is evaluated again with cascade levels left out (torch.sum / torch.mean swapped for the numpy
transcriptions of tests/cascade_cases.py inside the reference's own code); the generator asserts that the full
transcription IS ATen's result and that the shortened one changes recorded results at every size that reaches the level,
re-seeding until it does.

    python tools/gen_golden_cascade.py [--only views|consensus]
"""
import argparse
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
CHILD = "MH_GEN_CASCADE_CHILD"


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

import cascade_cases as cc  # noqa: E402
from ref_import import import_reference  # noqa: E402
from monohair_amd import synth  # noqa: E402

THREADS = (1, 8)


class swapped:
    """inside the block, torch.sum(float32, dim=0) / torch.mean(float32, dim=-1) are the numpy transcriptions with the
    given number of cascade levels (tail_levels: the row_sum form of the trailing columns)"""

    def __init__(self, levels, tail_levels=None):
        self.levels, self.tail = levels, tail_levels

    def __enter__(self):
        self.sum, self.mean = torch.sum, torch.mean
        real_sum, real_mean, lv, tl = self.sum, self.mean, self.levels, self.tail

        def my_sum(x, *a, **k):
            dim = k.get("dim", a[0] if a else None)
            if x.dtype == torch.float32 and dim == 0 and x.dim() >= 2:
                return torch.from_numpy(cc.outer_sum(x.contiguous().numpy(), lv, tl))
            return real_sum(x, *a, **k)

        def my_mean(x, *a, **k):
            dim = k.get("dim", a[0] if a else None)
            if x.dtype == torch.float32 and dim == -1 and x.dim() == 3:
                K = x.shape[-1]
                s = cc.inner_sum(x.contiguous().numpy().reshape(-1, K), lv)
                return (torch.from_numpy(s) / K).reshape(x.shape[:-1])
            return real_mean(x, *a, **k)

        torch.sum, torch.mean = my_sum, my_mean
        return self

    def __exit__(self, *exc):
        torch.sum, torch.mean = self.sum, self.mean


def eq(a, b):
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def at_threads(fn):
    """fn() at every thread count: the results must not depend on it"""
    res = []
    for t in THREADS:
        torch.set_num_threads(t)
        res.append(fn())
    torch.set_num_threads(THREADS[-1])
    for r in res[1:]:
        assert all(eq(x, y) for x, y in zip(res[0], r)), "the result depends on ATen's thread count"
    return res[-1]


def bare_pmvo(R, V):
    pm = R["PMVO"].PMVO({}, {}, {}, {}, {}, device="cpu", image_size=[cc.BASE["H"], cc.BASE["W"]], patch_size=cc.PATCH,
                        visible_threshold=cc.VIS_THR, conf_threshold=cc.THR)
    return pm


def loss_case(R, V, seed):
    D, op, cp, vis = cc.loss_inputs(V, seed)
    pm = bare_pmvo(R, V)
    pm.Ori_patch, pm.Conf_patch = torch.from_numpy(op), torch.from_numpy(cp)
    pm.visible, pm.mask = torch.from_numpy(vis), torch.ones(vis.shape)

    def run():
        return tuple(t.numpy().copy() for t in pm.compute_prj_loss(torch.from_numpy(D), None, None))

    ref = at_threads(run)
    with swapped(4):
        assert all(eq(a, b) for a, b in zip(run(), ref)), "the transcription is not ATen's order"
    with swapped(2):
        short = run()
    return ref, ~((short[0] == ref[0]) | (np.isnan(short[0]) & np.isnan(ref[0])))


def scene_case(R, base, base_cams, cand, V, seed):
    from scipy.spatial import KDTree

    maps = cc.view_maps(base, V, seed)
    names = ["view_%04d" % v for v in range(V)]
    cams = {n: base_cams[v % len(base_cams)] for v, n in enumerate(names)}
    scene = dict(cams=[dict(file=n) for n in names], **{k: torch.from_numpy(v) for k, v in maps.items()})
    depths, Ori, Conf, masks = synth.scene_to_reference_dicts(scene)
    pm = R["PMVO"].PMVO(cams, depths, Ori, Conf, masks, device="cpu", image_size=[cc.BASE["H"], cc.BASE["W"]],
                        patch_size=cc.PATCH, visible_threshold=cc.VIS_THR, conf_threshold=cc.THR)
    pts_s = cc.pick(cand, cc.N_SEARCH, seed)
    pts_v = cc.pick(cand, cc.N_VOTES, seed + 1) * np.where(np.arange(cc.N_VOTES) % 3 == 0, 1.04, 1.0)[:, None]
    dirs = cc.directions(cc.N_VOTES, seed)
    bust, scalp = cc.toy_head()
    R["PMVO"].bust_tree, R["PMVO"].scalp_tree = KDTree(data=bust), KDTree(data=scalp)
    R["PMVO"].scalp_max = np.max(scalp, axis=0)
    tv = torch.from_numpy(pts_v).type(torch.float)

    def fwd():
        _, so, ml, hc = pm.forward(pts_s)
        bidx, bval = pm.Find_max_conf_from_visible_view()
        return so.numpy().copy(), ml.numpy().copy(), hc.numpy().copy(), bidx.numpy().astype(np.int32), bval.numpy().copy()

    def votes():
        sidx, _, fidx = pm.filter_points(tv)
        unv = pm.compute_unvisible_points(tv)
        return pm.refine(tv, torch.from_numpy(dirs)).numpy().copy(), sidx.numpy().copy(), fidx.numpy().copy(), unv.numpy().copy()

    f, r = at_threads(fwd), at_threads(votes)
    with swapped(4):
        assert eq(votes()[0], r[0]) and eq(fwd()[1], f[1]), "the transcription is not ATen's order"
    ne = lambda a, b: ~((a == b) | (np.isnan(a) & np.isnan(b)))          # noqa: E731
    with swapped(2):
        d_fwd, d_ref = ne(fwd()[1], f[1]), ne(votes()[0], r[0])
    out = dict(points=pts_s, vote_points=pts_v, dirs=dirs, fwd_ori=f[0], fwd_loss=f[1], fwd_hc=f[2], base_idx=f[3],
               base_val=f[4], refine_loss=r[0], surface_index=r[1], filter_index=r[2], unvisible_index=r[3],
               map_sums=cc.map_checksums(maps))
    return out, d_fwd, d_ref


def gen_views(R):
    base = synth.make_scene(cc.BASE["V"], cc.BASE["H"], cc.BASE["W"], seed=cc.BASE["seed"], scale=cc.BASE["scale"],
                            rings=cc.BASE["rings"])
    Cam = R["Camera_utils"].Camera
    base_cams = [Cam(c["ndc_prj"], np.linalg.inv(np.array(c["pose"])), c["file"]) for c in base["cams"]]
    out = dict(base_pose=np.stack([c.pose.numpy() for c in base_cams]), base_proj=np.stack([c.proj.numpy() for c in base_cams]),
               base_rinv=np.stack([torch.linalg.inv(c.pose[:3, :3]).numpy() for c in base_cams]))
    bnp = {k: base[k].numpy() for k in ("depth", "ori", "conf", "mask")}
    for k, v in bnp.items():
        out["base_" + k] = v
    cand = synth.candidate_points(res=32, seed=7)
    meta = dict(base=cc.BASE, patch=cc.PATCH, thr=cc.THR, vis_thr=cc.VIS_THR, S=cc.S, torch=torch.__version__,
                capability=torch.backends.cpu.get_cpu_capability(), threads=list(THREADS),
                column_rule="whole blocks of 32 columns: cascade; trailing C mod 32 columns: row_sum (sum_block 32); "
                            "identical at 1 and 8 threads", cases={})
    for V in cc.VIEW_COUNTS:
        tail0 = cc.N_VOTES - cc.N_VOTES % 32
        for seed in range(100, 140):
            (loss, idx, hc), d_loss = loss_case(R, V, seed)
            if V >= cc.V_FEELS_LEVEL2 and not d_loss.any():
                continue
            break
        else:
            raise SystemExit("V=%d: no seed makes compute_prj_loss feel level 2" % V)
        for sseed in range(200, 240):
            sc, d_fwd, d_ref = scene_case(R, bnp, base_cams, cand, V, sseed)
            if V >= cc.V_FEELS_LEVEL2 and not (d_ref[:tail0].any() and d_fwd.any()):
                continue
            if V >= 4 * cc.V_FEELS_LEVEL2 and not d_ref[tail0:].any():
                continue
            break
        else:
            raise SystemExit("V=%d: no seed makes the scene's losses feel level 2" % V)
        if V < cc.V_FEELS_LEVEL2:
            assert not (d_loss.any() or d_fwd.any() or d_ref.any())
        if V < 4 * cc.V_FEELS_LEVEL2:
            assert not d_ref[tail0:].any()            # row_sum's partials see V / 4 rows each
        pre = "v%d_" % V
        out.update({pre + "loss": loss, pre + "idx": idx.astype(np.int32), pre + "hc": hc})
        out.update({pre + k: v for k, v in sc.items()})
        meta["cases"][V] = dict(loss_seed=seed, scene_seed=sseed,
                                share_differing_without_level2=dict(
                                    prj_loss=float(d_loss.mean()), forward=float(d_fwd.mean()),
                                    refine_cascade_rows=float(d_ref[:tail0].mean()), refine_row_sum_rows=float(d_ref[tail0:].mean())),
                                finite=dict(prj_loss=int(np.isfinite(loss).sum()), forward=int(np.isfinite(sc["fwd_loss"]).sum()),
                                            refine=int(np.isfinite(sc["refine_loss"]).sum())))
        print("views", V, meta["cases"][V], flush=True)
    np.savez_compressed(os.path.join(OUT, "cascade_views.npz"), meta=np.array(repr(meta)), **out)


def gen_consensus(R):
    sim = R["PMVO_utils"].compute_points_similarity
    meta = dict(torch=torch.__version__, capability=torch.backends.cpu.get_cpu_capability(), threads=list(THREADS), cases={})
    out = {}
    for K in cc.GROUP_SIZES:
        for seed in range(300, 340):
            g = cc.group(K, seed)
            t = torch.from_numpy(g)[None]

            def index_of(res):
                hit = np.flatnonzero((g == res.numpy()[0]).all(axis=1))
                assert len(hit) == 1
                return int(hit[0])

            def run():
                return (sim(t).numpy().copy(),)

            ref = at_threads(run)[0] if K <= 4097 else run()[0]      # (the 1-thread run of the largest groups takes minutes)
            i_ref = index_of(torch.from_numpy(ref))
            with swapped(4):
                assert index_of(sim(t)) == i_ref, "the transcription is not ATen's order"
            with swapped(2):
                i2 = index_of(sim(t))
            with swapped(1):
                i1 = index_of(sim(t))
            if (K >= cc.K_FEELS_LEVEL2 and i2 == i_ref) or (K >= cc.K_FEELS_LEVEL1 and i1 == i_ref):
                continue
            break
        else:
            raise SystemExit("K=%d: no seed separates the orders" % K)
        if K < cc.K_FEELS_LEVEL2:
            assert i2 == i_ref
        if K < cc.K_FEELS_LEVEL1:
            assert i1 == i_ref
        out["k%d_out" % K], out["k%d_index" % K] = ref, np.int32(i_ref)
        meta["cases"][K] = dict(seed=seed, index=i_ref, index_levels01=i2, index_one_level=i1)
        print("consensus", K, meta["cases"][K], flush=True)
    np.savez_compressed(os.path.join(OUT, "consensus_levels.npz"), meta=np.array(repr(meta)), **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default=None, choices=("views", "consensus"))
    a = ap.parse_args()
    assert torch.backends.cpu.get_cpu_capability() == "AVX2", torch.backends.cpu.get_cpu_capability()
    os.makedirs(OUT, exist_ok=True)
    os.chdir("/tmp")
    torch.manual_seed(0)
    R = import_reference(gabor=False)
    if a.only in (None, "consensus"):
        gen_consensus(R)
    if a.only in (None, "views"):
        gen_views(R)


if __name__ == "__main__":
    main()
