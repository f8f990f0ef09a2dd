"""Golden vectors of the scalp diffusion (tests/golden/scalp_diffusion.npz), run by the imported reference function
diffusion_scalp (Utils/PMVO_utils.py:467-593) on float32 inputs, in a temporary working directory (it writes
total_normal.npy / total_sample.npy there, which are read back as the recorded rows).

    python tools/gen_golden_diffusion.py

Case "shell": a 48x64x64 (Z,Y,X) volume with a shell of hair around a sphere of 300 scalp samples; the orientations blend
the radial direction (either sign) with a random one, part of the shell is missing, part of it has no orientation and
some hair sits on the scalp, so that every way a walk can end occurs.  Case "edge": hand-made samples on a 16x24x40 volume (edge_case below);
case "one": the same volume with a single sample.

The reference exposes only the returned volumes and the two .npy files, so the run is traced from outside: the module's
`enumerate` names the current sample, torch.row_stack hands over point_set / normal_set of every accepted walk, the calls of
points_to_voxel and torch.cosine_similarity count loop turns and restarts (three cosines per restart), and the last
points_to_voxel result is the voxel of every row.  Recorded sparse: the occupied voxels with their orientations, and the
voxels the reference changed with their new values.  The numpy restatement (tests/scalp_diffusion_np.py) is run alongside
and must reproduce everything exactly, reach every family listed in `FAMILIES`, and stay clear of every decision boundary.
If an assertion fails, change the seed or the hand-made coordinates.
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
sys.path.insert(2, os.path.join(ROOT, "tests"))

from ref_import import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
F32 = np.float32
VMIN = np.array([-0.32, -0.32, -0.24], F32)
VS = F32(0.005 / 2)
FAMILIES = ("accept_pos_first", "accept_neg_first", "accept_pos_restarted", "accept_neg_restarted")


def to_world(v):
    """voxel coordinates (x, y, z) -> float32 world points (voxel_to_points)"""
    p = np.asarray(v, F32) * VS + VMIN
    p[..., 1:] *= -1
    return p.astype(F32)


def unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def shell_case(rng, n=300):
    Z, Y, X = 48, 64, 64
    c = np.array([32.0, 32.0, 24.0])
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    d = np.stack([xx, yy, zz], -1) + 0.5 - c
    r = np.linalg.norm(d, axis=-1)
    radial = d / r[..., None] * np.array([1.0, -1.0, -1.0])           # world frame: y and z negated
    hair = (r > 14) & (r < 19)
    hair &= ~((d[..., 0] > 6) & (np.abs(d[..., 1]) < 7))                # a hole: walks of ten steps
    hair |= (r > 8.5) & (r < 11.5) & (d[..., 2] > 7)                    # hair on the scalp: samples inside it
    blend = rng.random((Z, Y, X, 1))
    sign = np.where(rng.random((Z, Y, X, 1)) < 0.5, -1.0, 1.0)
    rnd = rng.normal(size=(Z, Y, X, 3))
    rnd /= np.linalg.norm(rnd, axis=-1, keepdims=True)
    o = unit(blend * sign * radial + (1 - blend) * rnd)
    o[d[..., 1] < -12] = 0                                              # hair without an orientation: nine restarts
    occ = hair.astype(F32)[None]
    ori = np.ascontiguousarray((o * hair[..., None]).transpose(3, 0, 1, 2)).astype(F32)
    dirs = rng.normal(size=(n, 3))
    dirs /= np.linalg.norm(dirs, axis=1, keepdims=True)
    pts = to_world(c + dirs * (9.7 + 0.6 * rng.random((n, 1))))
    nrm = unit(dirs * np.array([1.0, -1.0, -1.0]) + 0.15 * rng.normal(size=(n, 3)))
    return pts, nrm, ori, occ


def edge_case(rng):
    """(points, normals, ori, occ, expect): expect[name] = sample index of each hand-made situation"""
    Z, Y, X = 16, 24, 40
    occ = np.zeros((1, Z, Y, X), F32)
    ori = np.zeros((3, Z, Y, X), F32)
    ex = np.array([1, 0, 0], F32)
    pts, nrm, expect = [], [], {}

    def hair(x, y, z, o):
        occ[0, z, y, x] = 1
        ori[:, z, y, x] = np.asarray(o, F32)

    def sample(name, v, nv=ex):
        expect.setdefault(name, []).append(len(pts))
        pts.append(to_world(v))
        nrm.append(np.asarray(nv, F32))

    sample("step1", [10.5, 2.5, 2.5]); hair(11, 2, 2, ex)                                   # noqa: E702
    sample("step9", [10.5, 4.4, 2.6]); hair(19, 4, 2, ex)                                   # noqa: E702
    sample("ten_steps", [10.5, 6.5, 2.5])
    for k in range(3):                                                                      # three arcs into one voxel
        sample("three", [10.3 + 0.2 * k, 8.4 + 0.05 * k, 2.5])
    hair(13, 8, 2, ex)
    for k in range(70):                                                                     # more than a wave's worth
        sample("many", [10.2 + 0.008 * k, 10.3 + 0.004 * k, 2.3 + 0.005 * k])
    hair(14, 10, 2, ex)
    diag = unit([1, -1, -1])                                                                # (+,+,+) in voxel space
    sample("diagonal", [10.45, 12.4, 6.35], diag)
    for x in range(13, 16):
        for y in range(15, 18):
            for z in range(9, 12):
                hair(x, y, z, diag)
    sample("negative_coordinate", [-0.5, 14.5, 2.5]); hair(3, 14, 2, ex)                    # noqa: E702
    sample("zero_orientation", [10.5, 16.5, 2.5]); occ[0, 2, 16, 12] = 1                    # noqa: E702
    sample("inside", [20.5, 18.5, 2.5]); hair(20, 18, 2, ex)                                # noqa: E702
    sample("minus_grow_dir", [10.5, 20.5, 2.5]); hair(13, 20, 2, -ex)                       # noqa: E702
    g = unit([0.3, 0.95, 0.1])                                                              # 72 degrees off: restarts
    sample("bent", [10.5, 12.5, 13.5])
    for x in range(13, 24):
        for y in range(2, 22):
            for z in range(12, 16):
                hair(x, y, z, g)
    jit = rng.normal(scale=1e-4, size=(len(pts), 3)).astype(F32)                            # no exact boundary
    return (np.array(pts, F32) + jit).astype(F32), unit(np.array(nrm) + 1e-3 * rng.normal(size=(len(pts), 3))), ori, occ, expect


def run_reference(U, pts, nrm, ori, occ, tmp):
    """diffusion_scalp traced from outside -> dict of the recorded quantities"""
    n = pts.shape[0]
    cur = {"i": -1}
    turns, cosines = np.zeros(n + 1, np.int64), np.zeros(n + 1, np.int64)
    stacks, last = [], {}

    def enum(it, *a):
        for i, v in enumerate(it, *a):
            cur["i"] = i if i < n else n
            yield i, v
        cur["i"] = n

    orig_ptv, orig_cos, orig_stack = U.points_to_voxel, torch.cosine_similarity, torch.row_stack

    def ptv(p):
        turns[cur["i"]] += 1
        last["v"] = orig_ptv(p)
        return last["v"]

    def cos(*a, **k):
        cosines[cur["i"]] += 1
        return orig_cos(*a, **k)

    def stack(rows):
        stacks.append((cur["i"], orig_stack(rows).numpy().copy()))
        return orig_stack(rows)

    U.enumerate, U.points_to_voxel, torch.cosine_similarity, torch.row_stack = enum, ptv, cos, stack
    cwd = os.getcwd()
    os.chdir(tmp)
    try:
        with contextlib.redirect_stdout(io.StringIO()):
            cur["i"] = n
            o, c = U.diffusion_scalp(torch.from_numpy(pts.copy()), torch.from_numpy(nrm.copy()),
                                     torch.from_numpy(ori.copy()), torch.from_numpy(occ.copy()))
    finally:
        os.chdir(cwd)
        del U.enumerate
        U.points_to_voxel, torch.cosine_similarity, torch.row_stack = orig_ptv, orig_cos, orig_stack
    assert o.dtype == torch.float32 and c.dtype == torch.float32
    ts, tn = np.load(os.path.join(tmp, "total_sample.npy")), np.load(os.path.join(tmp, "total_normal.npy"))
    assert ts.dtype == np.float64 and tn.dtype == np.float64
    status, step, restarts = np.zeros(n, np.int32), np.zeros(n, np.int32), (cosines[:n] // 3).astype(np.int32)
    end, first, lastn = np.zeros((n, 3), F32), np.zeros((n, 3), F32), np.zeros((n, 3), F32)
    acc = set()
    for k in range(0, len(stacks), 2):
        (i, P), (j, N) = stacks[k], stacks[k + 1]
        assert i == j and P.shape == N.shape and np.array_equal(P[0], pts[i]) and P.dtype == F32 == N.dtype
        acc.add(i)
        step[i], end[i], first[i], lastn[i] = len(P) - 1, P[-1], N[0], N[-1]
    for i in range(n):
        if i not in acc:
            # not accepted: nine restarts, or the first turn ended it (inside hair), or ten steps without an end
            status[i] = 3 if restarts[i] == 9 else (1 if turns[i] == 1 else 2)
            step[i] = 10 if status[i] == 2 else 0
    o, c = o.numpy(), c.numpy()
    changed = np.argwhere((o != ori).any(0) | (c[0] != occ[0]))
    z, y, x = changed.T
    return dict(status=status, step=step, restarts=restarts, end_point=end, first_normal=first, last_normal=lastn,
                total_sample=ts, total_normal=tn, voxel=last["v"].type(torch.long).numpy(), changed=changed.astype(np.int32),
                changed_ori=o[:, z, y, x].T.copy(), changed_occ=c[0, z, y, x].copy())


def record(out, tag, pts, nrm, ori, occ, rec):
    nz = np.argwhere(occ[0] != 0)
    assert not (ori[:, occ[0] == 0] != 0).any()
    out[tag + "_shape"] = np.array(occ.shape[1:], np.int32)
    out[tag + "_occ_nz"] = nz.astype(np.int16)
    out[tag + "_ori_nz"] = ori[:, nz[:, 0], nz[:, 1], nz[:, 2]].T.copy()
    out[tag + "_points"], out[tag + "_normals"] = pts, nrm
    for k, v in rec.items():
        out["%s_%s" % (tag, k)] = v


def main():
    ref = import_reference()
    U = ref["PMVO_utils"]
    import scipy
    from test_scalp_diffusion_host import check_case, load_case

    out = dict(meta=np.array("numpy %s, scipy %s, torch %s" % (np.__version__, scipy.__version__, torch.__version__)))
    tmp = tempfile.mkdtemp(prefix="mh_df_")
    pts, nrm, ori, occ = shell_case(np.random.default_rng(11))
    record(out, "shell", pts, nrm, ori, occ, run_reference(U, pts, nrm, ori, occ, tmp))
    pe, ne, orie, occe, expect = edge_case(np.random.default_rng(5))
    record(out, "edge", pe, ne, orie, occe, run_reference(U, pe, ne, orie, occe, tmp))
    one = expect["step9"][0]
    record(out, "one", pe[one:one + 1], ne[one:one + 1], orie, occe, run_reference(U, pe[one:one + 1], ne[one:one + 1], orie, occe, tmp))
    shutil.rmtree(tmp)
    for k, v in expect.items():
        out["edge_expect_" + k] = np.array(v, np.int32)

    for tag in ("shell", "edge", "one"):
        case = load_case(out, tag)
        res, stats = check_case(out, tag, case)
        det = res[2]
        hist = np.bincount(det["status"], minlength=5)
        print(tag, "status", hist.tolist(), "rows", len(det["total_sample"]), "changed", len(out[tag + "_changed"]),
              "restarts of accepted", np.bincount(det["restarts"][det["status"] == 0]).tolist(), dict(stats))
        for k in ("cos_near", "boundary_near", "zero_tangent", "rows_outside"):
            assert stats[k] == 0, (tag, k, stats[k])
        assert hist[4] == 0
        if tag == "shell":
            for k in FAMILIES:
                assert stats[k] > 0, k
            assert hist[1] > 0 and hist[2] > 0 and hist[3] > 0
            r = det["restarts"][det["status"] == 0]
            assert r.min() == 0 and r.max() >= 2
        if tag == "edge":
            st, sp = det["status"], det["step"]
            e = {k: v for k, v in expect.items()}
            assert st[e["step1"][0]] == 0 and sp[e["step1"][0]] == 1 and st[e["step9"][0]] == 0 and sp[e["step9"][0]] == 9
            assert st[e["ten_steps"][0]] == 2 and sp[e["ten_steps"][0]] == 10
            assert (st[e["three"]] == 0).all() and (st[e["many"]] == 0).all() and st[e["diagonal"][0]] == 0
            assert st[e["negative_coordinate"][0]] == 0 and stats["trunc_negative"] > 0
            assert st[e["zero_orientation"][0]] == 3 and stats["zero_ori"] == 9 and st[e["inside"][0]] == 1
            assert st[e["minus_grow_dir"][0]] == 0 and stats["accept_neg_first"] > 0
            assert st[e["bent"][0]] == 0 and det["restarts"][e["bent"][0]] >= 1
            per = det["rows_per_voxel"]
            assert max(per.values()) > 64 and sum(1 for v in per.values() if v >= 3) >= 2
            off = np.concatenate([[0], np.cumsum(np.where(st == 0, sp + 1, 0))])
            d = e["diagonal"][0]
            vd = det["voxel"][off[d]:off[d + 1]]
            assert (np.abs(np.diff(vd, axis=0)).sum(1) == 0).any(), "two rows of one arc in one voxel"
            assert (det["voxel"][:, 0] == 0).any() and (det["total_sample"][:, 0] < float(VMIN[0])).any()
    np.savez_compressed(os.path.join(OUT, "scalp_diffusion.npz"), **out)
    print("scalp_diffusion written: %.1f kB" % (os.path.getsize(os.path.join(OUT, "scalp_diffusion.npz")) / 1024))


if __name__ == "__main__":
    main()
