"""Golden vectors of strand tracing and connection at production strand lengths and volume borders (tests/golden/strands_long.npz),
run by the imported reference on the CPU.

    python tools/gen_golden_strands_long.py

A 64 x 24 x 56 volume (W, H, Z pairwise different) holding: a slab at each of the six faces whose orientation points
outwards with a tilt, so that a walk leaves the volume and goes on over the clamped border voxels; two pillars along y
that leave through both y faces (both 256-step caps, 513 points), one of them stored with the opposite sign in its upper
part; a closed ring (hundreds of steps inside the volume); a block of occupied voxels without orientation.
HairGrowing.trace / traceFromScalp are called seed by seed with an empty flag volume, seeds outside the volume included,
then GenerateGuideStrandFromScalp and randomlyGenerateSegments run as a whole.

Connection, case "long": find_connect_info, smooth_strands and save_hair_strands on hand-laid segments of 2..513 points
(long_segments) in the 256 x 256 x 192 box the reference's occupancy test hard-codes, occupied in two boxes.

Every property the fixture exists for is asserted here, on the reference's output alone, before the file is written.
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
from gen_golden_connect import BUST, DOT, THR, VMIN, end_lists, pack, run_connect  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
GT = (64, 24, 56)            # X, Y, Z of the tracing volume
RING_C, RING_R, RING_T, PITCH, PULL = (32.0, 28.0), 12.0, 1.0, 0.004, 0.3
GROW = 0.8


# ---------------------------------------------------------------------------------------------- the tracing volume
SLABS = ((np.s_[0:2, 9:12, 25:28], (-1, 0.05, 0.012)), (np.s_[62:64, 9:12, 25:28], (1, -0.02, 0.012)),
         (np.s_[40:43, 0:2, 25:28], (0.02, -1, 0.012)), (np.s_[40:43, 22:24, 25:28], (0.012, 1, -0.03)),
         (np.s_[29:32, 9:12, 0:2], (0.02, 0.012, -1)), (np.s_[29:32, 9:12, 54:56], (-0.012, 0.04, 1)))
PILLAR_A, PILLAR_B, BLOCK = np.s_[3:5, :, 3:5], np.s_[56:58, :, 48:50], np.s_[30:33, :, 27:30]


def long_volume():
    """occ [X,Y,Z], ori [X,Y,Z,3] in the reference's array layout.  `e` below is the field the walk follows;
    HairGrowing.__init__ negates y and z of what is stored, so (e_x, -e_y, -e_z) is stored."""
    rng = np.random.default_rng(21)
    X, Y, Z = GT
    x, y, z = np.meshgrid(np.arange(X), np.arange(Y), np.arange(Z), indexing="ij")
    px, pz = x + 0.5 - RING_C[0], z + 0.5 - RING_C[1]
    r = np.sqrt(px * px + pz * pz)
    ux, uz = px / np.maximum(r, 1e-9), pz / np.maximum(r, 1e-9)
    e = np.stack([-uz - PULL * (r - RING_R) * ux, np.full(r.shape, PITCH), ux - PULL * (r - RING_R) * uz], -1)
    e = e / np.linalg.norm(e, axis=-1, keepdims=True)
    e = e + 0.02 * rng.normal(size=e.shape)
    e = e / np.linalg.norm(e, axis=-1, keepdims=True)
    ring = (np.abs(r - RING_R) <= RING_T) & (y >= 11) & (y < 13)      # a closed ring: hundreds of steps inside the volume
    occ = ring.astype(np.float64)
    e[~ring] = 0

    def fill(sl, d):
        d = np.asarray(d, float)
        occ[sl] = 1
        e[sl] = d / np.linalg.norm(d)
    for sl, d in SLABS:            # a slab at each face pointing outwards, tilted: the clamped walk drifts over border voxels
        fill(sl, d)
    fill(PILLAR_A, (0.001, 1, -0.001))          # leaves through both y faces: both caps
    fill(PILLAR_B, (-0.002, 1, 0.003))
    e[56:58, 16:, 48:50] *= -1                  # stored with the opposite sign: trace stops here, the scalp walk turns round
    occ[BLOCK] = 1                              # occupied, no orientation
    e[BLOCK] = 0
    ori = e * np.array([1.0, -1.0, -1.0])
    return occ, ori


def long_seeds(occ):
    """(trace seeds before the reference's in-place shift, scalp points, scalp normals), float32"""
    rng = np.random.default_rng(22)
    X, Y, Z = GT

    def pick(sl, k):
        m = np.zeros(GT, bool)
        m[sl] = True
        v = np.argwhere(m & (occ != 0)).astype(np.float32)
        return v[rng.choice(len(v), k, replace=False)]
    tr = [pick(np.s_[:, 11:13, :], 24), pick(PILLAR_A, 8), pick(PILLAR_B, 8), pick(BLOCK, 2)] + [pick(sl, 6) for sl, _ in SLABS]
    # seeds outside the volume: beyond each face, over an occupied border voxel (the reference clamps them)
    tr.append(np.array([[-5, 10, 26], [X + 3, 10, 26], [41, -4, 26], [41, Y + 2, 26], [30, 10, -6], [30, 10, Z + 4],
                        [3.2, -3, 3.2], [4, Y + 5, 4], [56.5, -40, 48.5], [-2, -2, -2]], np.float32))
    tr = np.concatenate(tr, 0).astype(np.float32)
    # scalp: roots around the structures, normals pointing at them, some roots outside the volume
    sp, sn = [], []
    for k in range(40):            # inside the ring, pointing outwards
        a, rad = rng.random() * 2 * np.pi, rng.random() * 8.0
        sp.append([RING_C[0] + rad * np.cos(a), 11.2 + rng.random() * 1.5, RING_C[1] + rad * np.sin(a)])
        sn.append([np.cos(a), rng.normal(scale=0.02) - 0.02, np.sin(a)])
    for k in range(12):            # beside the pillars, below the slab of the y+ face
        c = (4.5, 4.5) if k % 2 else (57.5, 49.5)
        a = rng.random() * 2 * np.pi
        sp.append([c[0] + 6 * np.cos(a), rng.random() * 30 - 4, c[1] + 6 * np.sin(a)])
        sn.append([-np.cos(a), rng.normal(scale=0.05), -np.sin(a)])
    for k in range(4):
        sp.append([40.5 + k, 10.0 + k, 25.5 + k])
        sn.append([0.0, 1.0, 0.0])
    # far from everything (25 steps through empty space), and through the block without orientation
    sp += [[20.0, 12.0, 40.0], [44.0, 30.0, 20.0], [30.5, 0.5, 28.5], [31.5, -2.5, 27.5]]
    sn += [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 1.0, 0.0]]
    sp, sn = np.array(sp), np.array(sn)
    sn /= np.linalg.norm(sn, axis=1, keepdims=True)
    return tr, sp.astype(np.float32), sn.astype(np.float32)


def trunc_clamp(p, dims):
    return np.clip(np.trunc(p).astype(np.int64), 0, np.array(dims) - 1)


def gen_tracing(HairGrow, out):
    import scipy.io

    X, Y, Z = GT
    occ, ori = long_volume()
    tmp = tempfile.mkdtemp(prefix="mh_sl_")
    o = ori.transpose((0, 1, 3, 2)).reshape(X, Y, Z * 3).transpose((1, 0, 2))
    scipy.io.savemat(os.path.join(tmp, "Ori3D.mat"), {"Ori": o})
    scipy.io.savemat(os.path.join(tmp, "Occ3D.mat"), {"Occ": occ.transpose((1, 0, 2))})
    solver = HairGrow.HairGrowing(os.path.join(tmp, "Occ3D.mat"), os.path.join(tmp, "Ori3D.mat"), device="cpu")
    assert tuple(solver.occ.shape[1:]) == (Z, Y, X)
    seeds, sp, sn = long_seeds(occ)
    out.update(trace_shape=np.array(GT), trace_occ_nz=np.argwhere(occ != 0).astype(np.int16),
               trace_ori_nz=np.argwhere(np.any(ori != 0, -1)).astype(np.int16), grow_thr=np.float32(GROW),
               scalp_points=sp, scalp_normals=sn)
    out["trace_ori_nz_val"] = ori[tuple(out["trace_ori_nz"].T.astype(np.int64))].astype(np.float32)
    occ_zyx = solver.occ[0].numpy()

    # ---- trace, seed by seed, empty flag volume
    flag = torch.zeros_like(solver.occ)[0]
    torch.manual_seed(31)
    shifted, first, lens, pts = [], [], [], []
    for s in seeds:
        t = torch.from_numpy(s.copy())
        st = solver.trace(t, flag, GROW, X, Y, Z)
        shifted.append(t.numpy().copy())
        if st is False:
            first.append(-1)
            lens.append(0)
            continue
        st = st.numpy()
        k = np.flatnonzero((st == shifted[-1]).all(1))
        assert len(k) >= 1
        k = int(k[0]) if len(k) == 1 else int(k[np.argmin(np.abs(k - (len(st) - 1) / 2))])
        first.append(256 - k)
        lens.append(len(st))
        pts.append(st)
    assert float(flag.max()) == 0
    first, lens = np.array(first, np.int32), np.array(lens, np.int32)
    out.update(trace_seeds_in=seeds, trace_seeds=np.stack(shifted), trace_first=first, trace_len=lens,
               trace_pts=np.concatenate(pts, 0))
    nb, nf = 256 - first, first + lens - 257                  # backward / forward steps
    ok = lens > 0
    assert (lens == 513).any(), "no strand with both caps"
    assert (ok & (nf == 256) & (nb < 256)).any(), "no strand at the forward cap only"
    for lo, hi in ((65, 128), (129, 192), (257, 512)):          # the last: more than 256 points without both caps
        assert ((lens >= lo) & (lens <= hi)).any(), (lo, hi)
    P = out["trace_pts"].astype(np.float64)
    dims = np.array(GT)
    for a in range(3):
        assert (P[:, a] < 0).any() and (P[:, a] >= dims[a]).any(), "no point beyond a face of axis %d" % a
    # a coordinate in (-1, 0) at which the walk goes on; >= 10 consecutive points outside the volume
    o_ = np.concatenate([[0], np.cumsum(lens)])
    frac_go, run_out = 0, 0
    for i in np.flatnonzero(ok):
        s = P[o_[i]:o_[i + 1]]
        outside = ((s < 0) | (s >= dims)).any(1)
        inner = ((s > -1) & (s < 0)).any(1)
        frac_go += int(inner[1:-1].sum())                       # interior points of a strand: the walk went on from them
        run = 0
        for f in outside:
            run = run + 1 if f else 0
            run_out = max(run_out, run)
    assert frac_go > 0 and run_out >= 10, (frac_go, run_out)
    sd = np.stack(shifted)
    assert (((sd < 0) | (sd >= dims)).any(1) & ok).any(), "no strand from a seed outside the volume"
    # .type(torch.long) truncates: every recorded point indexes an occupied voxel through trunc + clamp, except where a
    # walk stopped on an empty voxel (ends only)
    idx = trunc_clamp(P, GT)
    assert np.array_equal(idx, torch.from_numpy(out["trace_pts"]).type(torch.long).clamp(
        torch.zeros(3, dtype=torch.long), torch.tensor(GT) - 1).numpy())
    print("trace: %d seeds, %d strands, lengths %s, both caps %d, forward cap only %d, longest run outside %d" %
          (len(seeds), int(ok.sum()), np.percentile(lens[ok], [0, 25, 50, 75, 100]).astype(int).tolist(),
           int((lens == 513).sum()), int((ok & (nf == 256) & (nb < 256)).sum()), run_out))

    # ---- traceFromScalp, seed by seed, the branches of HairGrow.py:184-205 counted
    cnt = {"inner_keep": 0, "inner_lift": 0, "turn": 0, "stop": 0, "inner_turn": 0}
    slen, spts = [], []
    for p, nrm in zip(sp, sn):
        st = solver.traceFromScalp(torch.from_numpy(p.copy()), torch.from_numpy(nrm.copy()), GROW, X, Y, Z, None)
        if st is None:
            slen.append(0)
        else:
            slen.append(len(st))
            spts.append(st.numpy())
    slen = np.array(slen, np.int32)
    out.update(scalp_len=slen, scalp_pts=np.concatenate(spts, 0))
    assert np.array_equal(branch_counts(solver, sp, sn, cnt), slen)
    assert all(v > 0 for v in cnt.values()), cnt
    assert (slen == 257).any(), "no scalp strand at the cap"
    none = np.flatnonzero(slen == 0)
    # a None through 25 steps of empty space and one through 25 steps of occupied voxels without orientation
    kinds = set()
    for i in none:
        t = sn[i] + np.array([0, 1.0, 0]) * min(sn[i][1] + 1, 1)
        t /= np.linalg.norm(t)
        walk = sp[i].astype(np.float64) + np.outer(np.arange(26), t)         # straight while dot(Tan, n) >= 0.85 only
        if abs(t[1]) == 1.0:
            ii = trunc_clamp(walk, GT)
            kinds.add("block" if occ[ii[:, 0], ii[:, 1], ii[:, 2]].all() else
                      ("empty" if not occ[ii[:, 0], ii[:, 1], ii[:, 2]].any() else "mixed"))
    assert {"block", "empty"} <= kinds, kinds
    S = out["scalp_pts"].astype(np.float64)
    assert ((S < 0) | (S >= dims)).any()
    assert (((sp < 0) | (sp >= dims)).any(1) & (slen > 0)).any(), "no scalp strand from a root outside the volume"
    print("scalp: %d roots, %d None, lengths up to %d, at the cap %d, branches %s" %
          (len(sp), len(none), slen.max(), int((slen == 257).sum()), cnt))

    # ---- the two drivers
    for name in ("guide", "random"):
        solver = HairGrow.HairGrowing(os.path.join(tmp, "Occ3D.mat"), os.path.join(tmp, "Ori3D.mat"), device="cpu")
        torch.manual_seed(77)
        with contextlib.redirect_stdout(io.StringIO()), contextlib.redirect_stderr(io.StringIO()):
            if name == "guide":
                strands, num_root = solver.GenerateGuideStrandFromScalp(torch.from_numpy(sp.copy()),
                                                                        torch.from_numpy(sn.copy()), None, GROW)
                out["guide_num_root"] = np.int32(num_root)
            else:
                strands = solver.randomlyGenerateSegments(GROW)
        out[name + "_len"] = np.array([s.shape[0] for s in strands], np.int32)
        out[name + "_pts"] = torch.cat(strands, 0).numpy()
        assert out[name + "_len"].max() == 513 and len(strands) > 50
        print(name, "strands:", len(strands), "points:", out[name + "_pts"].shape[0], "longest", out[name + "_len"].max())
    assert int(out["guide_num_root"]) == int((slen > 0).sum())
    shutil.rmtree(tmp)
    return occ_zyx


def branch_counts(solver, sp, sn, cnt):
    """Which branches of traceFromScalp's step (HairGrow.py:184-205) the recorded roots take.  The step is replayed here
    with the reference's own torch ops on the solver's volume, and the replay is held to the recorded result of every
    root (same length, same None), so a count stands for a branch the reference took."""
    vol_ori, vol_occ = solver.ori.numpy(), solver.occ[0].numpy()
    X, Y, Z = GT
    f32 = np.float32
    lens = []
    for p, nrm in zip(sp, sn):
        d = np.array([0, 1, 0], f32)
        lift = min(float(torch.dot(torch.from_numpy(nrm), torch.from_numpy(d))) + 1, 1)
        t = torch.from_numpy(nrm) + torch.from_numpy(d) * lift
        t = (t / torch.linalg.norm(t, 2, -1)).numpy()
        pos = p.copy()
        inner, count = True, 0
        ii = trunc_clamp(pos, GT)
        while True:
            if vol_occ[ii[2], ii[1], ii[0]] == 0 and not inner:
                break
            nxt = (torch.from_numpy(pos) + torch.from_numpy(t)).numpy()
            ni = trunc_clamp(nxt, GT)
            nt = vol_ori[:, ni[2], ni[1], ni[0]].copy()
            tt, tn = torch.from_numpy(t), torch.from_numpy(nt)
            if float(torch.linalg.norm(tn, 2)) < 0.1 and inner:
                if float(torch.dot(tt, torch.from_numpy(nrm))) < 0.85:
                    cnt["inner_keep"] += 1
                    nt = t
                else:
                    cnt["inner_lift"] += 1
                    nt = tt + torch.from_numpy(d) * lift
                    nt = (nt / torch.linalg.norm(nt, 2, -1)).numpy()
            else:
                if float(torch.dot(tn, tt)) < GROW and not inner:
                    if float(torch.dot(-tn, tt)) < GROW:
                        cnt["stop"] += 1
                        break
                    cnt["turn"] += 1
                    nt = -nt
                if float(torch.dot(torch.from_numpy(nt), tt)) < 0 and inner:
                    cnt["inner_turn"] += 1
                    nt = -nt
                inner = False
            pos, t, ii = nxt, nt, ni
            count += 1
            if count >= 256 or (count >= 25 and inner):
                break
        lens.append(0 if inner else count + 1)
    return np.array(lens, np.int32)


# ---------------------------------------------------------------------------------------------- connection, case "long"
LONG_LENS = (2, 5, 6, 20, 21, 63, 64, 65, 127, 128, 129, 192, 193, 513)
# occupancy of the 256 x 256 x 192 box as filled boxes (x0, x1, y0, y1, z0, z1), voxel indices, upper bounds excluded
LONG_OCC_BOXES = np.array([[70, 190, 70, 190, 80, 112],          # holds the spiral: strands of > 1000 points accepted at once
                           [20, 60, 20, 40, 20, 40]], np.int16)   # its y/z faces are approached by the retry rows below


def _arc(c, R, a0, n, step, u, w):
    t = a0 + np.arange(n) * (step / R)
    return c + R * (np.outer(np.cos(t), u) + np.outer(np.sin(t), w))


def _frame(rng):
    u = rng.normal(size=3)
    u /= np.linalg.norm(u)
    w = np.cross(u, rng.normal(size=3))
    w /= np.linalg.norm(w)
    return u, w


def _partner(rng, arc, end, q, L, reverse=False):
    """a segment of L points starting q points back from the tip (end 1) or root (end 0) of `arc`, 0.0003 beside it,
    running on in the arc's direction and bending away; reversed, it ends there instead"""
    p = arc[-1 - q] if end else arc[q]
    d = (arc[-1] - arc[-2]) if end else (arc[0] - arc[1])
    d = d / np.linalg.norm(d)
    n = np.cross(d, rng.normal(size=3))
    n /= np.linalg.norm(n)
    k = np.arange(L)
    part = p + 0.0003 * n + np.outer(k, d) * 0.0025 + np.outer(k ** 2, n) * 2e-5
    return part[::-1].copy() if reverse else part


def long_segments():
    """Hand-laid segments in world units (float32 values, as a .hair file would give them).  Every length of LONG_LENS
    occurs.  What each group is for is asserted in gen_connect_long."""
    rng = np.random.default_rng(41)
    segs = []
    far = lambda k: np.array([-0.2 + 0.05 * (k % 8), 0.15 - 0.05 * (k // 8), 0.1])      # noqa: E731  empty space, apart
    # (a) a wide spiral inside the first occupied box, cut 513 | 2 | 513: a strand of 1028 points
    n = 513 + 2 + 513
    t = np.arange(n) * (0.0025 / 0.1) + 0.3
    sp = np.stack([0.1 * np.cos(t), 0.1 * np.sin(t), t * (0.012 / (2 * np.pi)) - 0.02], 1)
    segs += [sp[:513].copy(), sp[513:515].copy(), sp[515:].copy()]
    # (b) quarter arcs, points 0.00205 apart, a partner q points back from an end: 5 + q of the arc's points are close
    #     (arc, end, q, partner length, partner reversed): end 1 / not reversed = tip -> root, end 0 / reversed = root -> tip,
    #     end 0 / not reversed = root -> root, end 1 / reversed = tip -> tip
    k = 0
    for L, plan in ((65, [(1, 1, 6, False), (0, 1, 5, True)]), (127, [(0, 1, 20, False), (1, 1, 6, True)]),
                    (129, [(1, 1, 64, False), (0, 2, 5, True)]), (192, [(0, 1, 65, True), (1, 2, 6, False)]),
                    (193, [(0, 1, 63, False), (1, 1, 21, True)]), (128, [(1, 2, 5, False)]), (64, [(1, 1, 6, False)]),
                    (63, [(0, 1, 6, True)])):
        u, w = _frame(rng)
        arc = _arc(far(k), L * 0.00205 * 4.0 / (2 * np.pi), rng.random() * 6, L, 0.00205, u, w)
        segs.append(arc)
        for end, q, Lp, rev in plan:
            segs.append(_partner(rng, arc, end, q, Lp, rev))
        k += 1
    # (c) a nearly closed loop of 128 points 0.0045 apart (its ends 0.004 apart, so lim is small) with a 2-point segment
    #     leaving its tip past its root: few close points, refused by the end rule alone; the same loop opened to three
    #     quarters keeps its partner because dist[-1] >= lim
    for frac, Lp in ((1.0, 2), (0.75, 2)):
        u, w = _frame(rng)
        R = (127 * 0.0045 + 0.004) / (2 * np.pi) / frac
        arc = _arc(far(k), R, 0.0, 128, 0.0045, u, w)
        segs += [arc, _partner(rng, arc, 1, 0, Lp)]
        k += 1
    # (d) 5-point segments 0.002 apart with a partner q points back from the tip: 3 + q points closer than 0.005
    for q in (0, 1):
        u, w = _frame(rng)
        s5 = far(k) + np.outer(np.arange(5), u) * 0.002
        segs += [s5, _partner(rng, s5, 1, q, 6)]
        k += 1
    # (e) a 20-point segment whose tip has two admissible roots: the nearer one turned away (larger loss)
    u, w = _frame(rng)
    s20 = far(k) + np.outer(np.arange(20), u) * 0.0025
    d1 = 0.78 * u + np.sqrt(1 - 0.78 ** 2) * w
    segs += [s20, s20[-1] + 0.001 * w + np.outer(np.arange(5), d1) * 0.0025,
             s20[-1] + 0.003 * u + 0.0003 * w + np.outer(np.arange(6), u) * 0.0025]
    k += 1
    # (f) four segments end to end, the 2nd and 4th stored reversed: a chain of mixed orientations
    u, w = _frame(rng)
    line = far(k) + np.outer(np.arange(6 + 5 + 21 + 20), u) * 0.0025 + np.outer(np.arange(52) ** 2, w) * 1e-5
    segs += [line[:6].copy(), line[6:11][::-1].copy(), line[11:32].copy(), line[32:][::-1].copy()]
    k += 1
    # (g) a closed ring of four pieces: a cycle
    t = np.arange(80) * (2 * np.pi / 80)
    u, w = _frame(rng)
    ring = far(k) + 0.0025 * 80 / (2 * np.pi) * (np.outer(np.cos(t), u) + np.outer(np.sin(t), w))
    segs += [ring[20 * m:20 * m + 20].copy() for m in range(4)]
    k += 1
    # (h) rows just outside the y / z faces of the second occupied box: refused at first, accepted after a shift
    for m in range(3):
        x0 = np.array([25.0 + 10 * m, 40.2 + 0.3 * m, 40.2 + 0.2 * m])
        row = (x0 + np.outer(np.arange(6), [1.0, 0, 0]))
        segs.append((row * 0.0025 + VMIN) * np.array([1.0, -1.0, -1.0]))
    return [s.astype(np.float32).astype(np.float64) for s in segs]


def long_occ():
    occ = np.zeros((192, 256, 256), np.float32)           # [Z,Y,X]
    for x0, x1, y0, y1, z0, z1 in LONG_OCC_BOXES.astype(int):
        occ[z0:z1, y0:y1, x0:x1] = 1
    return occ


def gen_connect_long(HairGrow, U, out):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_hair_connect_gpu as T        # the plain numpy evaluation of the reference's rules (tests/test_hair_connect_host.py)

    segs = long_segments()
    assert {len(s) for s in segs} >= set(LONG_LENS)
    occ = long_occ()
    solver = HairGrow.HairGrowing.__new__(HairGrow.HairGrowing)      # find_connect_info needs no volume but `occ`
    solver.occ = torch.from_numpy(occ[None])
    orig_ptv = HairGrow.points_to_voxel
    HairGrow.points_to_voxel = lambda p: orig_ptv(p.clone())         # see gen_golden_connect's docstring
    out.update({"long_" + k: v for k, v in end_lists(segs, THR).items()})
    out["long_in_len"] = np.array([len(s) for s in segs], np.int32)
    out["long_in_pts"] = np.concatenate(segs, 0).astype(np.float32)
    assert np.array_equal(out["long_in_pts"].astype(np.float64), np.concatenate(segs, 0))
    out["long_occ_boxes"] = LONG_OCC_BOXES
    out.update(connect_thr=np.float64(THR), connect_dot=np.float64(DOT), bust=BUST)
    np.random.seed(4321)
    try:
        connected, table, draws, fail = run_connect(HairGrow, solver, [s.copy() for s in segs])
    finally:
        HairGrow.points_to_voxel = orig_ptv
    out["long_next_random"] = np.float64(np.random.random())
    out["long_table"], out["long_draws"], out["long_fail"] = table, draws, np.int32(fail)
    pack("long_out", connected, out)
    tmp = tempfile.mkdtemp(prefix="mh_sl_")
    with contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO()):
        smooth = U.smooth_strands([c - BUST for c in connected], 4.0, 2.0)
        U.save_hair_strands(os.path.join(tmp, "strands.hair"), smooth)
    out["long_strands_hair"] = np.frombuffer(open(os.path.join(tmp, "strands.hair"), "rb").read(), np.uint8)
    shutil.rmtree(tmp)

    # ---- what the case is for: the reference's table, and its rules evaluated in plain numpy
    st = T._stats()
    np.random.seed(4321)
    r_table, _, r_out, r_fail = T._rs_connect(segs, THR, DOT, occ, st)
    assert np.array_equal(r_table, table) and r_fail == fail, "the numpy evaluation disagrees with the reference"
    assert all(np.array_equal(a, b) for a, b in zip(r_out, connected))
    L = out["long_in_len"]
    for e in range(2):
        for ty in range(2):
            j = table[:, e, 0]
            m = (j >= 0) & (table[:, e, 1] == ty)
            assert (m & (L > 64) & (L <= 128)).any() and (m & (L > 128)).any(), ("no long join of pairing", e, ty)
    assert any(table[i, e, 0] >= 0 and L[i] > 64 and L[table[i, e, 0]] > 64 for i in range(len(L)) for e in range(2))
    need = ("count6_late", "count7_late", "short_count3", "short_count4", "end_rule_only_late", "kept_by_dlast", "fallback",
            "loss_order_differs", "chain_ge4", "cycle", "retried_ok", "exhausted")
    assert all(st[k] > 0 for k in need), {k: st[k] for k in need}
    olen = out["long_out_len"]
    assert (olen > 1000).any() and ((olen > 513) & (draws == 0)).any()
    assert ((draws > 0) & (draws < 50)).any() and (draws == 50).any()
    print("long: %d segments -> %d points, fail %d, retried %d, exhausted %d, longest %d; %s" %
          (len(segs), out["long_out_pts"].shape[0], fail, int((draws > 0).sum()), int((draws == 50).sum()), olen.max(),
           {k: st[k] for k in need}))


def main():
    import_reference()
    os.chdir(tempfile.gettempdir())
    import HairGrow
    import Utils.Utils as U

    out = {}
    gen_tracing(HairGrow, out)
    gen_connect_long(HairGrow, U, out)
    path = os.path.join(OUT, "strands_long.npz")
    np.savez_compressed(path, **out)
    print("strands_long written: %.1f kB" % (os.path.getsize(path) / 1024))


if __name__ == "__main__":
    main()
