"""Shared by tools/gen_golden_cascade.py and tests/test_cascade_levels_*.py: the seeded inputs behind
tests/golden/cascade_views.npz and tests/golden/consensus_levels.npz, regenerated bit for bit from what the files store
(numpy Generator streams and IEEE float32 arithmetic only, no libm), and plain numpy float32 transcriptions of ATen's CPU
summation orders (aten/src/ATen/native/cpu/SumKernel.cpp, AVX2 build: 8 floats per vector) with a switch that leaves
cascade levels out -- what the generator uses to prove that a fixture can tell a wrong order from the right one."""
import numpy as np

VIEW_COUNTS = (255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 4095)
GROUP_SIZES = (127, 128, 129, 511, 512, 513, 4095, 4096, 4097, 8191, 8192, 8193, 8704, 9728)
# Where leaving a level out can change a sum at all.  The first flush into a fresh level is exact (x + 0), and one more block
# only swaps the operands of one addition: a sum taken without level 2 is the SAME float until two more blocks of 16 rows
# follow the 256th row, i.e. from 289 rows on (4 * 289 views for row_sum, whose partials see every fourth row; 32 * 288 + 32
# members, whose rows hold 32 elements).  Likewise without level 1: from 16 + 2 rows on.  Below these sizes the generator
# asserts that the shortened sums are identical; 9728 members is the added size at which level 2 of the member sum can be felt.
V_FEELS_LEVEL2 = 256 + 32 + 1
K_FEELS_LEVEL1 = 32 * 18
K_FEELS_LEVEL2 = 32 * 288 + 32

BASE = dict(V=24, H=16, W=12, seed=3, scale=1.7, rings=3)       # the 24 rendered views every case cycles through
PATCH, THR, VIS_THR, S = 3, 0.15, 1.0, 90
N_SEARCH = 17      # 17 * 90 = 1530 columns = 47 blocks of 32 + 26 trailing columns
N_VOTES = 45       # [V, 45] sums: one block of 32 + 13 trailing columns (36..39 points change with ATen's thread count)
N_LOSS = 17        # the stand-alone compute_prj_loss case: [V, 17, 90]
F = np.float32


def _u(rng, shape):
    return rng.random(shape, dtype=np.float32)


def view_maps(base, V, seed):
    """[V,H,W] depth / conf / mask and [V,H,W,2] ori: view v shows base view v % 24 with seeded per-pixel changes (depth by
    +-0.04, inside the 0.1 ramp of the soft visibility; confidence scaled by 0.5..1; orientation moved off unit length)"""
    rng = np.random.default_rng([seed, V, 1])
    b = np.arange(V) % base["depth"].shape[0]
    H, W = base["depth"].shape[1:]
    r = _u(rng, (V, H, W, 4))
    depth = base["depth"][b] + (r[..., 0] - F(0.5)) * F(0.08)
    conf = base["conf"][b] * (F(0.5) + F(0.5) * r[..., 1])
    ori = base["ori"][b] + (r[..., 2:4] - F(0.5)) * F(0.4)
    return dict(depth=depth.astype(F), ori=ori.astype(F), conf=conf.astype(F), mask=base["mask"][b].astype(F))


def view_records(base_rec, V):
    """[V,48] camera records: view v has the camera of base view v % 24"""
    return np.ascontiguousarray(base_rec[np.arange(V) % base_rec.shape[0]])


def map_checksums(maps):
    return np.array([maps[k].astype(np.float64).sum() for k in ("depth", "ori", "conf", "mask")])


def pick(cand, n, seed):
    rng = np.random.default_rng([seed, 2])
    return cand[np.sort(rng.choice(len(cand), n, replace=False))]


def directions(n, seed):
    rng = np.random.default_rng([seed, 3])
    return (_u(rng, (n, 3)) * F(2) - F(1)).astype(F)


def loss_inputs(V, seed, N=N_LOSS, P=PATCH * PATCH):
    """seeded arguments of compute_prj_loss: D [V,N,S,2], Ori_patch [V,N,P,2], Conf_patch [V,N,P], visible [V,N] (a third of
    the views do not see a point, a third see it fully, the rest partly)"""
    rng = np.random.default_rng([seed, V, 4])
    D = _u(rng, (V, N, S, 2)) * F(2) - F(1)
    op = _u(rng, (V, N, P, 2)) * F(2) - F(1)
    cp = _u(rng, (V, N, P))
    u, w = _u(rng, (V, N)), _u(rng, (V, N))
    vis = np.where(u < F(0.33), F(-1), np.where(u < F(0.66), F(1), w)).astype(F)
    return D.astype(F), op.astype(F), cp.astype(F), vis


def toy_head():
    """the bust / scalp point sets PMVO.refine's head filter asks (as tools/gen_golden.py makes them)"""
    rngb = np.random.default_rng(123)
    bust = rngb.normal(size=(500, 3))
    bust = bust / np.linalg.norm(bust, axis=1, keepdims=True) * 0.09
    return bust, bust[bust[:, 1] > 0.03] * (0.1 / 0.09)


def group(K, seed):
    """[K,3] float32 directions in a tight cluster (sigma 1e-3 around one axis): |cos| of any two is within a few ulps of 1,
    so many candidates have nearly equal means and the winner follows the order of the sum.  No two rows are equal."""
    rng = np.random.default_rng([seed, K, 5])
    axis = _u(rng, (3,)) + F(0.25)
    g = (axis[None, :] + (_u(rng, (K, 3)) - F(0.5)) * F(2e-3)).astype(F)
    assert len(np.unique(g, axis=0)) == K
    return g


# ---------------------------------------------------------------------------------------------- ATen's orders in numpy
def _multi_row_sum(x, levels):
    """multi_row_sum over axis 0 of x [R, ...] (level_power 4): 16 rows into level 0; a full block goes into level 1, every
    16th block level 1 goes into level 2, every 256th level 2 into level 3.  levels = how many of the four exist: an absent
    level's flush stays in the level below (levels=1 is the plain running sum)."""
    R = x.shape[0]
    acc = [np.zeros(x.shape[1:], F) for _ in range(4)]
    i = 0
    while i + 16 <= R:
        for j in range(16):
            acc[0] = acc[0] + x[i + j]
        i += 16
        for lv in range(1, 4):
            if lv >= levels or (i & ((1 << (4 * lv)) - 1)) != 0:
                break
            acc[lv] = acc[lv] + acc[lv - 1]
            acc[lv - 1] = np.zeros_like(acc[0])
    for j in range(i, R):
        acc[0] = acc[0] + x[j]
    out = acc[0]
    for lv in range(1, 4):
        out = out + acc[lv]
    return out


def _row_sum(x, levels):
    """row_sum over axis 0: rows k, k + 4, ... into partial k (each a multi_row_sum), left-over rows into partial 0"""
    R = x.shape[0]
    L = R >> 2
    part = [_multi_row_sum(x[k:4 * L:4], levels) for k in range(4)]
    for i in range(4 * L, R):
        part[0] = part[0] + x[i]
    return ((part[0] + part[1]) + part[2]) + part[3]


def outer_sum(x, levels=4, tail_levels=None, block=32):
    """torch.sum(x, dim=0) of a contiguous float32 [V, ...]: the columns in whole blocks of 32 by multi_row_sum, the trailing
    C mod 32 columns by row_sum"""
    V = x.shape[0]
    x2 = np.ascontiguousarray(x, F).reshape(V, -1)
    C = x2.shape[1]
    t0 = C - C % block
    out = np.empty(C, F)
    out[:t0] = _multi_row_sum(x2[:, :t0], levels)
    out[t0:] = _row_sum(x2[:, t0:], levels if tail_levels is None else tail_levels)
    return out.reshape(x.shape[1:])


def inner_sum(x, levels=4):
    """torch.sum(x, dim=-1) of a contiguous float32 [M, K], K >= 8: element j < 32 (K // 32) to accumulator j mod 32 through
    multi_row_sum, left-over vectors of 8 into accumulator vector 0, the four vectors added, then the K mod 8 tail elements
    and the 8 lanes in order"""
    M, K = x.shape
    assert K >= 8
    vec, R = K >> 3, K >> 5
    a = _multi_row_sum(np.ascontiguousarray(x[:, :32 * R].reshape(M, R, 32).transpose(1, 0, 2)), levels)   # [M,32]
    for i in range(4 * R, vec):
        a[:, :8] = a[:, :8] + x[:, 8 * i:8 * i + 8]
    p = ((a[:, 0:8] + a[:, 8:16]) + a[:, 16:24]) + a[:, 24:32]
    fin = np.zeros(M, F)
    for j in range(8 * vec, K):
        fin = fin + x[:, j]
    for l in range(8):
        fin = fin + p[:, l]
    return fin


# ------------------------------------------------------------------------------------------------- reading the fixtures
def load(name):
    import ast
    import os

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", name + ".npz"), allow_pickle=False)
    return ast.literal_eval(str(z["meta"])), z


def views_case(meta, z, V):
    """(maps, [V,48] camera records from the reference's own tensors, the case's arrays by name) of one view count"""
    base = {k: z["base_" + k] for k in ("depth", "ori", "conf", "mask")}
    maps = view_maps(base, V, meta["cases"][V]["scene_seed"])
    assert np.array_equal(map_checksums(maps), z["v%d_map_sums" % V]), "the maps of V=%d do not regenerate" % V
    nb = base["depth"].shape[0]
    rec = np.zeros((nb, 48), F)
    rec[:, 0:16] = z["base_pose"].reshape(nb, 16)
    rec[:, 16:32] = z["base_proj"].reshape(nb, 16)
    rec[:, 32:41] = z["base_rinv"].reshape(nb, 9)
    pre = "v%d_" % V
    return maps, view_records(rec, V), {k[len(pre):]: z[k] for k in z.files if k.startswith(pre)}


def head_top(points32, scalp):
    """the host half of filter_head_points (PMVO.py:98-107)"""
    from scipy.spatial import KDTree

    d, _ = KDTree(data=scalp).query(points32, k=1)
    return np.logical_and(d < 0.04, points32[:, 2] < np.max(scalp, axis=0)[2] - 0.01)
