"""tests/golden/refine_edges.npz -- refine()'s decisions (PMVO.py:81-107, :602-726; PMVO_utils.py:386-404) with the compared value
ON its bound and one float either side, recorded from the reference's own run on the CPU (cases `loop`, `fit`, `p2v` of
tests/refine_edge_cases.py, which also holds the numpy restatements used below).  Scene, cameras and options of
e2e_headfilter.npz.  The generator asserts what the fixture is for: every designed value is what was wanted, the restatement
with the reference's operator reproduces every recorded row, and each opposite form (`<= 0.95`, `<= 0.04`, `z <= L`,
`z < float32(L)`, `loss <= threshold`, `y >= 0`, floor(x + 1/2), clip before the cast, last maximum, shell rows first) changes at
least one recorded row and only rows whose value sits on the bound.  Deterministic: a second run writes the same bytes.

    python tools/gen_golden_refine_edges.py
"""
import ast
import os
import shutil
import sys
import tempfile
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

from ref_import import import_reference  # noqa: E402
from monohair_amd import synth  # noqa: E402
import refine_edge_cases as rc  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F = np.float32
FAR = np.array([[50.0, 50.0, 50.0]])           # a scalp of one far vertex: filter_head_points returns the votes alone
B = np.array([0.3, -0.8, 0.52], F)


class Ref:
    """the reference's PMVO object on the scene of e2e_headfilter.npz, and its module"""

    def __init__(self):
        R = import_reference()
        self.R, self.mod = R, R["PMVO"]
        z = np.load(os.path.join(OUT, "e2e_multichunk.npz"))
        self.z, self.case = z, ast.literal_eval(str(z["meta"]))
        c = self.case
        scene = synth.make_scene(c["V"], c["H"], c["W"], seed=c["seed"], scale=c["scale"], rings=c["rings"], quantize=c["quantize"])
        cams = {}
        for cam in scene["cams"]:
            cams[cam["file"]] = R["Camera_utils"].Camera(cam["ndc_prj"], np.linalg.inv(np.array(cam["pose"])), cam["file"])
        depths, Ori, Conf, masks = synth.scene_to_reference_dicts(scene)
        self.pm = self.mod.PMVO(cams, depths, Ori, Conf, masks, device="cpu", image_size=[c["H"], c["W"]], patch_size=c["patch"],
                                visible_threshold=c["vis_thr"], conf_threshold=c["thr"])
        assert np.array_equal(np.stack([k.pose.numpy() for k in self.pm.camera]), z["cam_pose"])
        self.mod.device = "cpu"
        self.set_scalp(FAR)

    def set_scalp(self, scalp):
        from scipy.spatial import KDTree

        self.mod.bust_tree = KDTree(data=self.z["toy_bust"])
        self.mod.scalp_tree = KDTree(data=scalp)
        self.mod.scalp_max = np.max(scalp, axis=0)

    def votes(self, pts):
        self.set_scalp(FAR)
        return self.pm.filter_head_points(torch.from_numpy(np.ascontiguousarray(pts, F)), self.case["vis_thr"]).numpy()

    def refine(self, pts, ori, loss, shell, threshold, only=False, files=None):
        """the reference's refine() in a fresh directory -> {file: array} of refine/*.npy (+ the voxels of the .mat files)"""
        import scipy.io

        tmp = tempfile.mkdtemp(prefix="mh_refine_edges_")
        args = types.SimpleNamespace(device="cpu", output_path=tmp, save_root=os.path.join(tmp, "optimize"),
                                     save_path=os.path.join(tmp, "refine"),
                                     PMVO=types.SimpleNamespace(visible_threshold=self.case["vis_thr"]),
                                     data=types.SimpleNamespace(root=tmp))
        os.makedirs(args.save_path, exist_ok=True)
        for k, v in (files or {}).items():
            np.save(os.path.join(args.save_path, k + ".npy"), v)
        self.mod.refine(pts.copy(), ori.copy(), loss.copy(), self.pm, shell.copy(), args, infer_inner=False, threshold=threshold,
                        genrate_ori_only=only)
        out = {k: np.load(os.path.join(args.save_path, k + ".npy")) for k in rc.FILES}
        Ori3 = scipy.io.loadmat(os.path.join(args.save_path, "Ori3D.mat"))["Ori"]
        Occ3 = scipy.io.loadmat(os.path.join(args.save_path, "Occ3D.mat"))["Occ"]
        nz = np.argwhere(Occ3 != 0)                                     # [Y, X, Z] on disk
        Z = Occ3.shape[2]
        vox = np.stack([nz[:, 1], nz[:, 0], nz[:, 2]], 1).astype(np.int64)
        vori = np.stack([Ori3[nz[:, 0], nz[:, 1], c * Z + nz[:, 2]] for c in range(3)], 1)
        o = np.lexsort((vox[:, 2], vox[:, 1], vox[:, 0]))
        out["voxels"], out["voxel_ori"] = vox[o], vori[o]
        shutil.rmtree(tmp)
        return out


# ---------------------------------------------------------------------------------------------------------------------------
def search_cos_rows(rng):
    """three rows each whose max-cosine with B is float32(0.95), its lower and its upper neighbour (torch's own value); the
    third of each kind has the opposite sign, so that the second cosine is the larger one"""
    t = rng.normal(size=(40000, 3))
    b = B.astype(np.float64) / np.linalg.norm(B.astype(np.float64))
    t -= (t @ b)[:, None] * b
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    ang = np.arccos(0.95) + rng.uniform(-1.5e-7, 1.5e-7, len(t))
    a = ((np.cos(ang)[:, None] * b + np.sin(ang)[:, None] * t) * rng.uniform(0.5, 2.0, (len(t), 1))).astype(F)
    a[2::3] *= F(-1)
    sim = rc.max_cos(np.broadcast_to(B, a.shape), a)
    direct = torch.cosine_similarity(torch.from_numpy(np.broadcast_to(B, a.shape).copy()), torch.from_numpy(a), dim=-1).numpy()
    rows, kinds = [], []
    for kind, want in (("eq", rc.COS), ("below", rc.COS_LO), ("above", rc.COS_HI)):
        pos, neg = np.flatnonzero((sim == want) & (direct > 0)), np.flatnonzero((sim == want) & (direct < 0))
        assert len(pos) >= 2 and len(neg) >= 1, (kind, len(pos), len(neg))
        rows += [a[pos[0]], a[pos[1]], a[neg[0]]]
        kinds += [kind] * 3
    return np.array(rows, F), kinds


def search_vertex(p, want):
    """the vertex p -+ (0.04 + k ulp) e_axis for which scipy's own query of the float32 point p returns exactly `want`, or None.
    (0.04 ends at 2^-57: the sum is a float64 only where it stays below 2^-4, so the step goes towards zero on an axis on which
    the point is less than 0.1 from it)"""
    from scipy.spatial import KDTree

    p64 = p.astype(np.float64)
    for axis in range(3):
        step = -0.04 if p64[axis] > 0 else 0.04
        if abs(p64[axis] + step) >= 2.0 ** -4:
            continue
        x = p64[axis] + step
        for _ in range(16):
            x = np.nextafter(x, -np.inf)
        for _ in range(32):
            v = p64.copy()
            v[axis] = x
            d, _ = KDTree(data=np.stack([v, FAR[0]])).query(p[None], k=1)
            if d[0] == want:
                return v
            x = np.nextafter(x, np.inf)
    return None


def build_loop(ref, rng):
    z = ref.z
    n_base = rc.N_SURFACE - rc.N_CLUSTER - 2
    pts = z["opt_select_p"][::33].copy()              # (every 33rd point: the whole head, not one side of it)
    ori = z["opt_select_o"][::33].copy()
    loss = z["opt_min_loss"][::33].copy()
    pts[::3] *= F(1.3)
    votes = ref.votes(pts)
    # the cluster's centre: a point the votes leave alone; every other base point 1 cm or more from it
    c0 = int(np.flatnonzero(~votes)[40])
    far = np.linalg.norm(pts.astype(np.float64) - pts[c0].astype(np.float64), axis=1) > 0.01
    keep = np.flatnonzero(far)[:n_base]
    centre = pts[c0].copy()
    pts, ori, loss, votes = pts[keep], ori[keep], loss[keep], votes[keep]
    # the height points: the filtered base point with the largest z, and two copies of it 1 mm and 2 mm along x
    filt = np.flatnonzero(votes)
    hq = int(filt[np.argmax(pts[filt, 2])])
    z0, zz = None, pts[hq, 2]
    for _ in range(200):          # a float32 z0 with float64(z0) + 0.01 - 0.01 == z0 (scalp "b") and z0 < L < z0 + ulp / 2 ("a")
        top_b = float(zz) + 0.01
        top_a = float(zz) + 0.01 + 1e-9
        La, Lb = top_a - 0.01, top_b - 0.01
        if Lb == float(zz) and F(La) == zz and float(zz) < La and float(F(La)) != La:
            z0 = zz
            break
        zz = np.nextafter(zz, F(-9))
    assert z0 is not None
    hrows = np.repeat(pts[hq][None], 3, 0)
    hrows[:, 0] += np.array([0, 0.001, 0.002], F)
    hrows[:, 2] = [z0, np.nextafter(z0, F(-9)), np.nextafter(z0, F(9))]
    pts[hq] = hrows[0]
    # the distance points: three filtered points well below the height bound, far from the height points
    dq, verts = [], []
    for want in (rc.DIST, rc.DIST_LO, rc.DIST_HI):
        for i in filt:
            v = search_vertex(pts[i], want)
            if (i not in dq and pts[i, 2] < z0 - F(0.02) and np.linalg.norm(pts[i] - pts[hq]) > 0.09 and v is not None
                    and all(np.linalg.norm(pts[i] - pts[j]) > 0.09 for j in dq)):
                dq.append(int(i)), verts.append(v)
                break
    assert len(dq) == 3
    verts.append(pts[hq].astype(np.float64) + np.array([0.001, 0.02, 0.0]))        # 2 cm from the three height points
    scalp = {k: np.array(verts + [[9.0, 9.0, top]]) for k, top in (("a", top_a), ("b", top_b))}
    # the cluster
    cl = (centre.astype(np.float64) + rng.uniform(-1, 1, (rc.N_CLUSTER, 3)) * 2e-4).astype(F)
    cl_ori = np.repeat(B[None], rc.N_CLUSTER, 0)
    a_rows, kinds = search_cos_rows(rng)
    a_at = np.arange(5, 5 + 9 * 7, 7)
    cl_ori[a_at] = a_rows
    n0 = len(pts)
    pts = np.concatenate([pts, hrows[1:], cl]).astype(F)
    ori = np.concatenate([ori, np.repeat(ori[hq][None], 2, 0), cl_ori]).astype(F)
    loss = np.concatenate([loss, np.repeat(loss[hq], 2), np.full(rc.N_CLUSTER, loss[c0], F)]).astype(F)
    assert pts.shape == (rc.N_SURFACE, 3)
    shell = z["candidates"][z["filter_index"]][:rc.N_SHELL].copy()
    rows = dict(height=np.array([hq, n0, n0 + 1]), dist=np.array(dq), cos=n0 + 2 + a_at, cluster=np.arange(n0 + 2, len(pts)))
    return dict(points=pts, ori=ori, loss=loss, shell=shell, scalp=scalp, rows=rows, kinds=kinds, L=dict(a=La, b=Lb), z0=z0)


def run_loop(ref, c, out):
    from scipy.spatial import KDTree

    pts, ori, loss, shell, rows = c["points"], c["ori"], c["loss"], c["shell"], c["rows"]
    votes = ref.votes(pts)
    assert votes[rows["height"]].all() and votes[rows["dist"]].all()
    # the medoids and the similarities the loop compares: the reference's own functions on its own neighbour table
    _, index = KDTree(data=pts).query(pts, 100)
    assert np.isin(index[rows["cluster"]], rows["cluster"]).all(), "a cluster point has a neighbour outside the cluster"
    center = ref.R["PMVO_utils"].compute_points_similarity(torch.from_numpy(ori[index])).numpy()
    assert (center[rows["cluster"]] == B).all(), "the medoid of a cluster point is not a B row"
    similar = rc.max_cos(center, ori)
    want = {"eq": rc.COS, "below": rc.COS_LO, "above": rc.COS_HI}
    assert [similar[r] for r in rows["cos"]] == [want[k] for k in c["kinds"]]
    direct = torch.cosine_similarity(torch.from_numpy(center), torch.from_numpy(ori), dim=-1).numpy()[rows["cos"]]
    assert (direct[2::3] < 0).all() and (direct[0::3] > 0).all() and (direct[1::3] > 0).all()
    out.update(loop_points=pts, loop_ori=ori, loop_loss=loss, loop_shell=shell, loop_votes=votes, loop_center=center,
               loop_similar=similar, loop_scalp_a=c["scalp"]["a"], loop_scalp_b=c["scalp"]["b"],
               loop_rows_height=rows["height"].astype(np.int32), loop_rows_dist=rows["dist"].astype(np.int32),
               loop_rows_cos=rows["cos"].astype(np.int32), loop_L=np.array([c["L"]["a"], c["L"]["b"]]))
    # run "a": L is no float32; three thresholds
    ref.set_scalp(c["scalp"]["a"])
    dist_a, _ = ref.mod.scalp_tree.query(pts, k=1)
    assert list(dist_a[rows["dist"]]) == [rc.DIST, rc.DIST_LO, rc.DIST_HI]
    assert (dist_a[rows["height"]] < 0.03).all() and float(ref.mod.scalp_max[2] - 0.01) == c["L"]["a"]
    out["loop_dist"] = dist_a
    first = ref.refine(pts, ori, loss, shell, 0.5)
    ml = first["min_loss"]
    fin = np.sort(ml[np.isfinite(ml) & (ml != 0.5)])
    l = fin[150]
    assert fin[149] < l < fin[151] and int((ml < l).sum()) == 150
    thresholds = [0.5, float(l), float(np.nextafter(l, F(9)))]
    runs = [first] + [ref.refine(pts, ori, loss, shell, t) for t in thresholds[1:]]
    out["loop_thresholds"] = np.array(thresholds)
    for k in ("select_p", "select_o", "min_loss"):
        assert all(rc.eq(r[k], first[k]) for r in runs)
        out["loop_ref_" + k] = first[k]
    for i, r in enumerate(runs):
        for k in ("filter_unvisible", "filter_unvisible_ori"):
            out["loop_t%d_%s" % (i, k)] = r[k]
        kept = rc.keep_rule(ml, thresholds[i])
        assert len(kept) >= 100
        print("loop: threshold %.9g keeps %d points, %d shell rows" % (thresholds[i], len(kept), len(r["filter_unvisible"])))
    assert not rc.eq(runs[1]["filter_unvisible_ori"], runs[2]["filter_unvisible_ori"]), "the row on the threshold decides nothing"
    assert (ml == 0.5).sum() > 50 and len(rc.keep_rule(ml, 0.5, "le")) == len(rc.keep_rule(ml, 0.5)) + (ml == 0.5).sum()
    # run "b": L is the float32 z0
    ref.set_scalp(c["scalp"]["b"])
    assert float(ref.mod.scalp_max[2] - 0.01) == c["L"]["b"] == float(c["z0"])
    dist_b, _ = ref.mod.scalp_tree.query(pts, k=1)
    assert np.array_equal(dist_a, dist_b)
    second = ref.refine(pts, ori, loss, shell, 0.5)
    assert rc.eq(second["select_o"], first["select_o"])
    out["loop_b_min_loss"] = second["min_loss"]
    for k in ("filter_unvisible", "filter_unvisible_ori"):
        out["loop_b_" + k] = second[k]

    # --- the restatements reproduce the record; the opposite forms change rows on the bound only ---
    z = pts[:, 2]
    on = dict(cos=similar == rc.COS, dist=dist_a == rc.DIST, z=z == c["z0"])
    assert rc.eq(rc.replace_rule(similar, center, ori), first["select_o"])
    d = np.flatnonzero((rc.replace_rule(similar, center, ori, "le") != first["select_o"]).any(1))
    assert len(d) >= 3 and on["cos"][d].all(), d
    print("`<= 0.95` changes rows", d, "of select_o.npy")

    def filtered(L, **kw):
        return votes & ~rc.head_top_rule(dist_a, z, L, **kw)

    for name, res, L in (("a", first, c["L"]["a"]), ("b", second, c["L"]["b"])):
        assert np.array_equal(filtered(L), res["min_loss"] == 0.5), name
    forms = dict(a=[("<= 0.04", dict(dist_op="le"), "dist"), ("z < float32(L)", dict(z_form="f32_lt"), "z")],
                 b=[("<= 0.04", dict(dist_op="le"), "dist"), ("z <= L", dict(z_form="f64_le"), "z")])
    for name, L in c["L"].items():
        for what, kw, bound in forms[name]:
            d = np.flatnonzero(filtered(L, **kw) != filtered(L))
            assert len(d) >= 1 and on[bound][d].all(), (name, what, d)
            print("scalp %s: `%s` changes rows %s of min_loss.npy" % (name, what, d))
    # the height test both ways, on scalp "a": exactly the z == float32(L) point tells them apart, and the run followed float64
    La = c["L"]["a"]
    f64, f32 = z.astype(np.float64) < La, z < F(La)
    assert np.array_equal(np.flatnonzero(f64 != f32), np.flatnonzero(on["z"])) and on["z"].sum() == 1
    hz = rows["height"]
    assert list(first["min_loss"][hz] != 0.5) == list(f64[hz]) == [True, True, False], "the reference's run did not follow float64"
    assert list(second["min_loss"][hz] != 0.5) == [False, True, False]
    assert (z.astype(np.float64) <= La)[hz].tolist() == f64[hz].tolist()      # (`z <= L` cannot differ where L is no float32)
    dr = rows["dist"]
    assert list(first["min_loss"][dr] != 0.5) == [False, True, False]
    return len(first["filter_unvisible"])


# ---------------------------------------------------------------------------------------------------------------------------
def at_voxel(ix, iy, iz, frac=0.2):
    """a float32 point `frac` of a voxel off the centre of voxel (ix, iy, iz) on every axis (|frac| < 1/2: inside it)"""
    v = rc.VOXEL_MIN + (np.array([ix, iy, iz], np.float64) + frac) * rc.VOXEL_SIZE
    return np.array([v[0], -v[1], -v[2]], F)


def build_fit(ref, loop):
    P, O, Ls, tags = [], [], [], []

    def add(p, o, l, tag):
        P.append(np.asarray(p, F)), O.append(np.asarray(o, F)), Ls.append(F(l)), tags.append(tag)

    plain, low = (0.6, -0.8, 0.0), F(0.01)
    thr = F(rc.FIT_THR)
    # where a shell point survives the head filter: the centre of the loop case's cluster
    c1 = loop["points"][loop["rows"]["cluster"][0]]
    a, b, c = (int(v) for v in rc.p2v_rule(c1[None], rc.VOXEL_MIN, rc.VOXEL_SIZE, rc.GRID)[0])
    rng = np.random.default_rng(11)
    for _ in range(110):                                            # the hundred neighbours of that shell point
        add(at_voxel(a + 2, b, c, rng.uniform(-0.3, 0.3)), (0, -1, 0), low, "T")
    add(at_voxel(a, b, c, 0.1), (1, 0, 0), low, "tie_shell")
    shell_special = at_voxel(a, b, c, -0.1).astype(np.float64)
    for i, l in enumerate([thr, np.nextafter(thr, F(0)), np.nextafter(thr, F(1)), np.nan, 0.0, -0.0, -1.0, 0.5]):
        add(at_voxel(10 + 2 * i, 20, 20), plain, l, "loss")
    for i, y in enumerate([0.0, -0.0, 1e-45, -1e-45, np.finfo(F).tiny]):
        add(at_voxel(10 + 2 * i, 22, 20), (0.5, y, 0.7), low, "flip")
    add(at_voxel(20, 22, 20), (0.0, 0.0, 0.0), low, "flip")
    for i, pair in enumerate((((1, 0, 0), (0, -1, 0)), ((0, -1, 0), (1, 0, 0)))):
        for o in pair:
            add(at_voxel(10 + 2 * i, 24, 20), o, low, "tie")
    inside = [30, 30, 30]
    for axis in range(3):
        g = int(rc.GRID[axis])
        for edge, outs in ((0, (-1, -40)), (g - 1, (g, g + 40))):
            for k, o in zip((edge,) + outs, (plain, (0.0, -0.6, 0.8), (0.05, -0.6, 0.8))):
                v = list(inside)
                v[axis] = k
                add(at_voxel(*v), o, low, "border")
        for s in (1.0, -1.0):
            p = at_voxel(31, 31, 31)
            p[axis] = F(s * 1e7)
            add(p, plain, low, "huge")
    shell = np.concatenate([shell_special[None], ref.z["candidates"][ref.z["filter_index"]][200:260]])
    return dict(points=np.array(P, F), ori=np.array(O, F), loss=np.array(Ls, F), shell=shell, tags=tags)


def run_fit(ref, c, loop, out):
    pts, ori, loss, shell, tags = c["points"], c["ori"], c["loss"], c["shell"], np.array(c["tags"])
    ref.set_scalp(loop["scalp"]["a"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")                # (the cast of 4e9 to int32 warns)
        conv = np.array([4e9, -4e9, 2147483648.0, np.nan]).astype(np.int32)
        print("this host's float64 -> int32 of (4e9, -4e9, 2^31, NaN):", conv)
        assert (conv == rc.INT_MIN).all()
        res = ref.refine(pts[:1], ori[:1], loss[:1], shell, rc.FIT_THR, only=True,
                         files=dict(select_p=pts, select_o=ori, min_loss=loss))
    out.update(fit_points=pts, fit_ori=ori, fit_loss=loss, fit_shell=shell, fit_int32_of_4e9=conv,
               fit_filter_unvisible=res["filter_unvisible"], fit_filter_unvisible_ori=res["filter_unvisible_ori"],
               fit_voxels=res["voxels"].astype(np.int32), fit_voxel_ori=res["voxel_ori"])
    sp, so = res["filter_unvisible"], res["filter_unvisible_ori"]
    assert sp[0].tobytes() == shell[0].astype(F).tobytes() and so[0].tolist() == [0, -1, 0], "the special shell point"

    def fit(loss_op="lt", **kw):
        kept = rc.keep_rule(loss, rc.FIT_THR, loss_op)
        v, m, s = rc.fit_rule(np.concatenate([pts[kept], sp]), np.concatenate([ori[kept], so]), len(kept), **kw)
        return v, m, s, kept

    vox, med, scores, kept = fit()
    assert len(kept) >= 100 and np.array_equal(vox, res["voxels"]) and rc.bits_equal(med, res["voxel_ori"])
    assert sorted(loss[kept[tags[kept] == "loss"]].tolist()) == sorted([float(np.nextafter(F(rc.FIT_THR), F(0))), 0.0, -0.0, -1.0])
    assert any(len(s) == 1 for s in scores) and sum(len(s) == 2 and s[0] == s[1] for s in scores) >= 3
    print("fit: %d kept points, %d shell rows, %d voxels" % (len(kept), len(sp), len(vox)))
    as_dict = lambda v, m: {tuple(r): x.astype(np.float64).tobytes() for r, x in zip(v.tolist(), m)}       # noqa: E731
    base = as_dict(vox, med)

    def changed(**kw):
        v, m, _, _ = fit(**kw)
        d = as_dict(v, m)
        return sorted(k for k in set(base) | set(d) if base.get(k) != d.get(k))

    vox_of = lambda rows: {tuple(r) for r in rc.p2v_rule(pts[rows], rc.VOXEL_MIN, rc.VOXEL_SIZE, rc.GRID).tolist()}    # noqa: E731
    clipped_last = lambda rows: {tuple(r) for r in rc.p2v_rule(pts[rows], rc.VOXEL_MIN, rc.VOXEL_SIZE, rc.GRID, clip_first=True).tolist()}   # noqa: E731
    on_thr = np.flatnonzero(loss == F(rc.FIT_THR))
    allp, allo = np.concatenate([pts[kept], sp]), np.concatenate([ori[kept], so])
    y0 = {tuple(r) for r in rc.p2v_rule(allp[allo[:, 1] == 0], rc.VOXEL_MIN, rc.VOXEL_SIZE, rc.GRID).tolist()}
    huge = np.flatnonzero(tags == "huge")
    ties = np.flatnonzero(np.isin(tags, ("tie", "tie_shell")))
    expect = {"loss <= threshold": (dict(loss_op="le"), vox_of(on_thr)),
              "y >= 0": (dict(flip="ge"), y0),
              "clip before the cast": (dict(clip_first=True), vox_of(huge) | clipped_last(huge)),
              "last maximum": (dict(tie="last"), vox_of(ties)),
              "shell rows first": (dict(shell_first=True), vox_of(np.flatnonzero(tags == "tie_shell")))}
    for what, (kw, allowed) in expect.items():
        d = changed(**kw)
        assert len(d) >= 1 and set(d) <= allowed, (what, d, allowed)
        print("fit: `%s` changes voxels %s" % (what, d))
    assert changed(rounding="floor") == []              # (no half is reachable on this grid: case p2v holds that rule)
    assert len(changed(tie="last")) == 3 and len(changed(shell_first=True)) == 1


def run_p2v(ref, out):
    p2v = ref.R["PMVO_utils"].p2v
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for name, dt in (("f32", F), ("f64", np.float64)):
            pts = rc.p2v_points(dt)
            x, y, z = p2v(pts.copy(), rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID)
            rec = np.stack([x, y, z], 1).astype(np.int32)
            out["p2v_%s_points" % name], out["p2v_%s_index" % name] = pts, rec
            assert np.array_equal(rc.p2v_rule(pts, rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID), rec)
            half, big = rc.on_a_half(pts, rc.BIN_MIN, rc.BIN_SIZE), rc.outside_int32(pts, rc.BIN_MIN, rc.BIN_SIZE)
            d = rc.p2v_rule(pts, rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID, rounding="floor") != rec
            assert d.any() and half[d].all(), name
            e = rc.p2v_rule(pts, rc.BIN_MIN, rc.BIN_SIZE, rc.BIN_GRID, clip_first=True) != rec
            assert e.any() and big[e].all(), name
            print("p2v %s: %d points; floor(x + 1/2) changes %d indices (%d on a half), clip before the cast %d (%d outside int32)"
                  % (name, len(pts), d.sum(), half.sum(), e.sum(), big.sum()))


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp on every member: the same arrays give the same bytes"""
    import zipfile

    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(arrays):
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with zf.open(info, "w") as f:
                np.lib.format.write_array(f, np.asanyarray(arrays[k]), allow_pickle=False)


def main():
    torch.manual_seed(0)
    ref = Ref()
    out = {}
    loop = build_loop(ref, np.random.default_rng(2024))
    n_shell = run_loop(ref, loop, out)
    run_fit(ref, build_fit(ref, loop), loop, out)
    run_p2v(ref, out)
    meta = dict(ref.case, numpy=np.__version__, torch=torch.__version__, height_rule="float64", fit_threshold=rc.FIT_THR,
                loop_shell_rows=n_shell)
    path = os.path.join(OUT, "refine_edges.npz")
    save_npz(path, dict(meta=np.array(repr(meta)), **out))
    print("refine_edges written: %d bytes" % os.path.getsize(path))


if __name__ == "__main__":
    main()
