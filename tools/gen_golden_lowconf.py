"""Generate tests/golden/pmvo_lowconf.npz by RUNNING THE REFERENCE ITSELF (imported read-only, CPU torch) on the cases of
tests/lowconf_cases.py: hand-edited patches that leave a point exactly 0, 1, 4, 5, 6 and 90 positive samples on rank 0 (4 and 5
also counted from the far end of the sweep, with patch 7, and at 4 and 5 samples in all), on both sides of the low-confidence rule
`lt(sum(positive_index), 5)` (PMVO.py:199).  The batch is the case points only.  Recorded: forward() per (patch, S) of
lowconf_cases.RUNS (the default of sample_next_3d_pos set to S, as tools/gen_golden_samples.py does) with the ranking it used;
the reference's own compute_prj_loss on rank 0 -- loss, index, flag, and the count of positive samples it compares with 5 (the
first argument of that torch.lt, taken while the method runs); forward() with the base-view rankings of
lowconf_cases.rankings() returned from Find_max_conf_from_visible_view (rank 0 repeated at rank 2; a later rank with base_val 0
and with a tiny positive one).  The file holds the seed, the reference's camera tensors, the edits, checksums of the maps, the
points and the results.

As tools/gen_golden_softmask.py: the work runs in a child process with ATEN_CPU_CAPABILITY=avx2, every call at 1 and at 8
threads, which must agree.  Asserted and printed: the reference's count equals the wanted count of every case; the numpy
restatement (tests/softmask_cases.py: prj_loss_np) gives the reference's (index, flag, count) on every row; the same restatement
with `< 4` and with `< 6` changes recorded (index, flag) rows; the rank taken by `tiny` and not by `zero` has the smaller loss.

8-bit code maps: orientation codes are 1 degree apart and a sweep turns about 0.8 degrees per sample, so a 4 / 5 pair needs two
codes whose bisector (on the half-degree grid) falls between samples 3 | 4 and 4 | 5: lowconf_cases.build_codes tries every usable
pair of the quantised scene (synth.make_scene_codes) and every pair of codes.  What it finds is recorded under c8_* (the
reference on the decoded planes, batch of the two points); if it finds none, that is printed and meta["codes"] is None.

    python tools/gen_golden_lowconf.py
"""
import io
import os
import subprocess
import sys
import zipfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
OUT = os.path.join(ROOT, "tests", "golden")
CHILD = "MH_GEN_LOWCONF_CHILD"


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

import lowconf_cases as lc  # noqa: E402
import softmask_cases as sc  # noqa: E402
from ref_import import import_reference  # noqa: E402
from monohair_amd import synth  # noqa: E402

THREADS = (1, 8)


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


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp per member: a second run reproduces the file byte for byte"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


class CountSeen:
    """while active, torch.lt(x, 5) of an integer tensor x -- the one comparison of compute_prj_loss (PMVO.py:199) -- leaves x"""

    def __enter__(self):
        self.seen, self._lt = [], torch.lt

        def lt(a, b, *args, **kw):
            if isinstance(b, int) and b == 5 and torch.is_tensor(a) and not a.is_floating_point():
                self.seen.append(a.numpy().copy())
            return self._lt(a, b, *args, **kw)

        torch.lt = lt
        return self

    def __exit__(self, *exc):
        torch.lt = self._lt


def main():
    assert torch.backends.cpu.get_cpu_capability() == "AVX2", torch.backends.cpu.get_cpu_capability()
    os.makedirs(OUT, exist_ok=True)
    os.chdir("/tmp")
    torch.manual_seed(0)
    R = import_reference(gabor=False)
    cls = R["PMVO"].PMVO
    cam_list = lc.scene()[0]
    Cam = R["Camera_utils"].Camera
    ref_cams = [Cam(c["ndc_prj"], np.linalg.inv(np.array(c["pose"])), c["file"]) for c in cam_list]
    out = dict(seed=np.int64(lc.SEED), cam_pose=np.stack([c.pose.numpy() for c in ref_cams]),
               cam_proj=np.stack([c.proj.numpy() for c in ref_cams]),
               cam_rinv=np.stack([torch.linalg.inv(c.pose[:3, :3]).numpy() for c in ref_cams]))
    rec = lc.records(out)
    case = lc.build(rec)
    ranks = lc.rankings(rec, case)
    pts, maps = case["points"], case["maps"]
    N = len(pts)
    out.update(points=pts, rows=case["rows"], view=case["view"], base=case["base"], edits=case["edits"],
               edit_conf=case["edit_conf"], map_sums=lc.map_checksums(maps))
    tp = torch.from_numpy(pts).type(torch.float)

    def make_pmvo(patch):
        scene = dict(cams=[dict(file=c["file"]) for c in cam_list], **{k: torch.from_numpy(v) for k, v in maps.items()})
        depths, Ori, Conf, masks = synth.scene_to_reference_dicts(scene)
        return cls({c.id: c for c in ref_cams}, depths, Ori, Conf, masks, device="cpu", image_size=[lc.H, lc.W],
                   patch_size=patch, visible_threshold=1, conf_threshold=lc.THR)

    def forward(pm):
        _, so, ml, hc = pm.forward(pts)
        return so.numpy().copy(), ml.numpy().copy(), hc.numpy().copy()

    default = cls.sample_next_3d_pos.__defaults__
    changed = {4: 0, 6: 0}
    meta = dict(V=lc.V, H=lc.H, W=lc.W, seed=lc.SEED, thr=lc.THR, cases=[list(c) for c in lc.CASES], runs=[list(r) for r in lc.RUNS],
                torch=torch.__version__, capability=torch.backends.cpu.get_cpu_capability(), threads=list(THREADS), npos={})
    try:
        for patch, S in lc.RUNS:
            cls.sample_next_3d_pos.__defaults__ = (S,)
            pm = make_pmvo(patch)
            key = "p%ds%d_" % (patch, S)
            fwd = at_threads(lambda: forward(pm))
            bidx, bval = pm.Find_max_conf_from_visible_view()
            assert eq(bidx[0].numpy(), case["base"])
            for k, a in zip(("fwd_ori", "fwd_loss", "fwd_hc", "base_idx", "base_val"), fwd + (bidx.numpy().astype(np.int32), bval.numpy())):
                out[key + k] = a.copy()

            def first_rank():
                pm.Compute_Visible_and_Ori(tp)
                b, _ = pm.Find_max_conf_from_visible_view()
                samp, surf = pm.sample_next_3d_pos(tp, b[0])
                D = pm.compute_reproject_ori(surf, samp)
                with CountSeen() as cs:
                    loss, index, hc = pm.compute_prj_loss(D, pm.Ori, pm.compute_weight(pm.visible, pm.Conf, pm.mask))
                assert len(cs.seen) == 1 and cs.seen[0].shape == (N,)
                return loss.numpy().copy(), index.numpy().copy(), hc.numpy().copy(), cs.seen[0].astype(np.int32), D.numpy().copy()

            loss, index, hc, npos, D = at_threads(first_rank)
            assert D.shape == (lc.V, N, S, 2)
            for k, a in zip(("r0_loss", "r0_idx", "r0_hc", "r0_npos"), (loss, index.astype(np.int32), hc, npos)):
                out[key + k] = a
            mine = lc.case_rows(patch, S)
            for ci in mine:
                assert npos[ci] == lc.CASES[ci][3], (lc.CASES[ci], int(npos[ci]))
            args = (D, pm.Ori_patch.numpy(), pm.Conf_patch.numpy(), pm.visible.numpy(), lc.THR)
            st = sc.prj_loss_np(*args)
            # (numpy rounds the cosine otherwise than ATen: on a row this run's patches were NOT tuned for, two samples whose
            # losses tie within 1e-6 can swap.  Count and flag must agree on every row, the index on every row of the run's own
            # cases and wherever there is no such tie)
            assert eq(st["hc"], hc) and eq(st["npos"], npos), "the restated rank-0 loss differs from the reference"
            for n in np.flatnonzero(st["idx"] != index):
                assert n not in mine and abs(st["all"][n, index[n]] - st["loss"][n]) < 1e-6, "the restated index differs from the reference"
                print("  row %s: restated index %d, the reference's %d: a tie within 1e-6" % (lc.NAMES[n], st["idx"][n], index[n]))
            index_r = st["idx"]
            for bound in (4, 6):
                alt = sc.prj_loss_np(*args, low_below=bound)
                rows = np.flatnonzero((alt["idx"] != index_r) | (alt["hc"] != hc))
                assert set(rows) <= set(np.flatnonzero(npos == min(bound, 5))), rows
                changed[bound] += len(rows)
                print("  patch %d S %2d: `< %d` changes (index, flag) of rows %s" % (patch, S, bound, [lc.NAMES[r] for r in rows]))
            meta["npos"]["p%ds%d" % (patch, S)] = [int(x) for x in npos]
            print("patch %d S %2d: positive samples %s; cases of this run: %s" % (
                patch, S, npos.tolist(), ", ".join("%s=%d idx %d flag %d" % (lc.NAMES[i], npos[i], index[i], hc[i]) for i in mine)), flush=True)
            print("  forward: loss %s\n  flag %s" % (np.array2string(fwd[1], precision=5), fwd[2].astype(int).tolist()))
        # the rankings: patch 3, S = 90, handed over where forward() asks for its ranking
        cls.sample_next_3d_pos.__defaults__ = (90,)
        pm = make_pmvo(3)
        got = {}
        for name in lc.RANKINGS:
            idx, val = ranks[name]
            pm.Find_max_conf_from_visible_view = lambda idx=idx, val=val: (torch.from_numpy(idx).type(torch.long), torch.from_numpy(val))
            got[name] = at_threads(lambda: forward(pm))
            out["rk_%s_idx" % name], out["rk_%s_val" % name] = idx, val
            for k, a in zip(("fwd_ori", "fwd_loss", "fwd_hc"), got[name]):
                out["rk_%s_%s" % (name, k)] = a
        a, b = lc.NAMES.index("k4"), lc.NAMES.index("k5")
        zero, tiny = got["zero"], got["tiny"]
        flags = 0
        for n in (a, b):
            assert tiny[1][n] < zero[1][n], "the later rank does not have the smaller loss"
            flags += int(tiny[2][n] != zero[2][n])
            print("ranking %s: rank 0 alone (base_val 0 after it): loss %.6g flag %d; rank 2 with base_val %g: loss %.6g flag %d" % (
                lc.NAMES[n], zero[1][n], zero[2][n], lc.TINY, tiny[1][n], tiny[2][n]))
        assert flags > 0, "no flag changes between the `zero` and the `tiny` ranking"
        others = np.setdiff1d(np.arange(N), (a, b))
        assert all(eq(x[others], y[others]) for x, y in zip(zero, tiny))
        print("ranking rep: %d of %d rows equal to the batch's own ranking" % (
            int(sum(all(eq(x[n], y[n]) for x, y in zip(got["rep"], [out["p3s90_" + k] for k in ("fwd_ori", "fwd_loss", "fwd_hc")])) for n in range(N))), N))
        # the 4 / 5 pair on 8-bit code maps
        cc = lc.build_codes(rec)
        meta["codes"] = None
        if cc is None:
            print("8-bit code maps: no usable pair of the quantised scene leaves 4 and 5 positive samples")
        else:
            maps, pts = lc.decode(cc["codes"]), cc["points"]
            tp, N = torch.from_numpy(pts).type(torch.float), len(pts)
            pm = make_pmvo(3)
            fwd = at_threads(lambda: forward(pm))
            bidx, bval = pm.Find_max_conf_from_visible_view()
            loss, index, hc, npos, D = at_threads(first_rank)
            assert npos.tolist() == [k for _, k in lc.CODE_CASES], npos
            st = sc.prj_loss_np(D, pm.Ori_patch.numpy(), pm.Conf_patch.numpy(), pm.visible.numpy(), lc.THR)
            assert eq(st["idx"], index) and eq(st["hc"], hc) and eq(st["npos"], npos)
            moved = {}
            for bound in (4, 6):
                alt = sc.prj_loss_np(D, pm.Ori_patch.numpy(), pm.Conf_patch.numpy(), pm.visible.numpy(), lc.THR, low_below=bound)
                moved[bound] = int(((alt["idx"] != index) | (alt["hc"] != hc)).sum())
            assert moved == {4: 1, 6: 1}, moved
            out.update(c8_points=pts, c8_rows=cc["rows"], c8_view=cc["view"], c8_base=cc["base"], c8_edits=cc["edits"],
                       c8_map_sums=np.array([cc["codes"][k].astype(np.float64).sum() for k in ("depth", "k8", "c8", "m8")]),
                       c8_fwd_ori=fwd[0], c8_fwd_loss=fwd[1], c8_fwd_hc=fwd[2], c8_base_idx=bidx.numpy().astype(np.int32),
                       c8_base_val=bval.numpy().copy(), c8_r0_loss=loss, c8_r0_idx=index.astype(np.int32), c8_r0_hc=hc, c8_r0_npos=npos)
            meta["codes"] = dict(points=[int(x) for x in cc["rows"]], views=[int(x) for x in cc["view"]],
                                 ori_codes=[[int(e[4]), int(e[5])] for e in cc["edits"] if e[4] >= 0], changed_by_lt_4=1, changed_by_lt_6=1)
            print("8-bit code maps: %s; rank 0: positive samples %s index %s flag %s; forward loss %s flag %s; `< 4` and `< 6` change one row each" % (
                meta["codes"], npos.tolist(), index.tolist(), hc.astype(int).tolist(), fwd[1].tolist(), fwd[2].astype(int).tolist()))
    finally:
        cls.sample_next_3d_pos.__defaults__ = default
    assert changed[4] > 0 and changed[6] > 0, changed
    meta["rows_changed_by_lt_4"], meta["rows_changed_by_lt_6"] = changed[4], changed[6]
    print("rank-0 rows whose recorded (index, flag) change: %d under `< 4`, %d under `< 6`" % (changed[4], changed[6]))
    path = os.path.join(OUT, "pmvo_lowconf.npz")
    save_npz(path, dict(meta=np.array(repr(meta)), **out))
    print("pmvo_lowconf.npz: %d bytes" % os.path.getsize(path))
    assert os.path.getsize(path) < (1 << 20)


if __name__ == "__main__":
    main()
