"""Shared by tools/gen_golden_refine_edges.py and tests/test_refine_edges_*.py: the cases behind tests/golden/refine_edges.npz.
The decisions of the second half of the pipeline, refine() (PMVO.py:81-107, :602-726, PMVO_utils.py:386-404), with the compared
value exactly ON its bound and one float either side -- what random inputs never produce:

  loop   the smoothing loop on the scene of e2e_headfilter.npz (24 views of 240 x 136, patch 3; 600 surface points, 200 shell
         points, one chunk): a tight cluster whose medoid is `B` everywhere and nine rows whose max(cos(B, A), cos(B, -A)) is
         float32(0.95) and its two neighbours; head-filtered points whose nearest vertex of a hand-made scalp is exactly 0.04 away
         (and the two float64 neighbours of 0.04); head-filtered points whose z is float32(L) and its two float32 neighbours for
         L = scalp_max[2] - 0.01, once with an L that is no float32 (scalp "a": the float64 and the float32 evaluation of
         `z < L` differ at z == float32(L)) and once with an L that is one (scalp "b": `<` and `<=` differ there); three loss
         thresholds: 0.5 (what every head-filtered point holds), a recorded output loss, its upper float32 neighbour.
  fit    genrate_ori_only=True on hand-written refine/*.npy: losses on the threshold, rows with y = +-0, +-1e-45, float32 tiny and
         an all-zero row alone in their voxels, points outside each of the six faces of the 256 x 256 x 192 grid that share the
         border voxel with an inside point, +-1e7 on each axis (rint(v) >= 2^31: the cast gives INT_MIN, hence voxel 0), voxels
         whose two members tie exactly, in both orders, and once as a surface row and a shell row.
  p2v    the reference's p2v on a binary grid (voxel_min -0.25, voxel_size 2^-8, 128^3), float32 and float64 points: indices on
         k + 1/2 for even and odd k, on -1/2 and dim - 1/2, -0.0, NaN, +-inf, +-3e9, 2147483647.5 and 2147483647.4.

Below: the fixture's loader and a numpy restatement of every decision with the operator (or the rounding, the order) as a
parameter -- what the generator uses to prove that the record tells the reference's form from the opposite one, and the host test
to hold the record.  numpy and CPU torch only; nothing from the GPU side."""
import ast
import os

import numpy as np

F = np.float32
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FIXTURE = os.path.join(GOLDEN, "refine_edges.npz")
FILES = ("select_p", "select_o", "min_loss", "filter_unvisible", "filter_unvisible_ori")

COS = F(0.95)
COS_LO, COS_HI = np.nextafter(COS, F(0)), np.nextafter(COS, F(1))
DIST = 0.04
DIST_LO, DIST_HI = np.nextafter(DIST, 0.0), np.nextafter(DIST, 1.0)
VOXEL_MIN = np.array([-0.32, -0.32, -0.24])
VOXEL_SIZE = 0.005 / 2
GRID = np.array([256, 256, 192], np.int32)
BIN_MIN = np.array([-0.25, -0.25, -0.25])
BIN_SIZE = 2.0 ** -8
BIN_GRID = np.array([128, 128, 128], np.int32)
FIT_THR = 0.05
INT_MIN = -2 ** 31
N_SURFACE, N_SHELL, N_CLUSTER = 600, 200, 120

OPS = {"lt": np.less, "le": np.less_equal, "gt": np.greater, "ge": np.greater_equal}


def load():
    z = np.load(FIXTURE, allow_pickle=False)
    return ast.literal_eval(str(z["meta"])), z


def eq(a, b):
    """plain equality of every element, NaN == NaN"""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f")


# ---------------------------------------------------------------------------------------------------------------------------
# the decisions, restated
# ---------------------------------------------------------------------------------------------------------------------------
def max_cos(center, ori):
    """maximum(cosine_similarity(c, o), cosine_similarity(c, -o)) of PMVO.py:631-633 by the installed CPU torch"""
    import torch

    c, o = torch.from_numpy(np.ascontiguousarray(center, F)), torch.from_numpy(np.ascontiguousarray(ori, F))
    return torch.maximum(torch.cosine_similarity(c, o, dim=-1), torch.cosine_similarity(c, -o, dim=-1)).numpy()


def replace_rule(similar, center, ori, op="lt"):
    """PMVO.py:634-636: rows whose similarity is below 0.95 (as float32, the dtype of the tensor) take the medoid"""
    out = np.array(ori, F)
    idx = OPS[op](similar, COS)
    out[idx] = center[idx]
    return out


def head_top_rule(dist, z, L, dist_op="lt", z_form="f64_lt"):
    """PMVO.py:105-106: nearer than 4 cm to the scalp AND below L = scalp_max[2] - 0.01.  z is float32, L a float64 scalar:
    "f64_lt" is NumPy 2's evaluation (the one recorded), "f32_lt" what value-based casting (NumPy 1.x) gives."""
    z = np.asarray(z, F)
    below = {"f64_lt": lambda: z.astype(np.float64) < L, "f64_le": lambda: z.astype(np.float64) <= L,
             "f32_lt": lambda: z < F(L)}[z_form]()
    return np.logical_and(OPS[dist_op](np.asarray(dist, np.float64), DIST), below)


def keep_rule(loss, threshold, op="lt"):
    """PMVO.py:656: the rows the loss threshold keeps (float32 comparison; NaN is never kept)"""
    return np.flatnonzero(OPS[op](np.asarray(loss, F), F(threshold)))


def canon_rule(ori, op="gt"):
    """PMVO.py:702-703: rows that point up are negated (`* -1`: a zero changes its sign bit)"""
    out = np.array(ori, F)
    out[OPS[op](out[:, 1], 0)] *= F(-1)
    return out


def cast_i32(v):
    """float64 -> int32 as the reference's host converts (cvttsd2si: NaN and everything outside [-2^31, 2^31) give INT_MIN)"""
    v = np.asarray(v, np.float64)
    ok = (v >= -2.0 ** 31) & (v < 2.0 ** 31)
    out = np.full(v.shape, INT_MIN, np.int64)
    out[ok] = v[ok].astype(np.int64)
    return out


def p2v_rule(points, voxel_min, voxel_size, grid, rounding="rint", clip_first=False):
    """PMVO_utils.py:386-404 -> [N,3] int64: y and z negated, float64 (p - min) / size, round half to even, cast, clip.
    rounding "floor": floor(x + 1/2); clip_first: the clip applied to the float64 value, before the cast."""
    g = np.asarray(grid).astype(np.int64)
    p = np.array(points)
    p[:, 1:] *= -1
    v = (p.astype(np.float64) - np.asarray(voxel_min)) / voxel_size
    v = np.rint(v) if rounding == "rint" else np.floor(v + 0.5)
    if clip_first:
        return cast_i32(np.clip(v, 0, g - 1))
    return np.clip(cast_i32(v), 0, g - 1)


def on_a_half(points, voxel_min, voxel_size):
    """[N,3] bool: the float64 index value is exactly k + 1/2"""
    p = np.array(points)
    p[:, 1:] *= -1
    v = (p.astype(np.float64) - np.asarray(voxel_min)) / voxel_size
    with np.errstate(invalid="ignore"):
        return np.isfinite(v) & (v - np.floor(v) == 0.5)


def outside_int32(points, voxel_min, voxel_size):
    """[N,3] bool: the rounded index is NaN or outside [-2^31, 2^31)"""
    p = np.array(points)
    p[:, 1:] *= -1
    v = np.rint((p.astype(np.float64) - np.asarray(voxel_min)) / voxel_size)
    return ~((v >= -2.0 ** 31) & (v < 2.0 ** 31))


def mean_similarity(rows):
    """compute_points_similarity's score of every member of one group (PMVO_utils.py:366-379) by the installed CPU torch"""
    import torch

    t = torch.from_numpy(np.ascontiguousarray(rows, F))
    K = t.shape[0]
    a = t[None, :, None, :].expand(1, K, K, 3)
    b = a.permute(0, 2, 1, 3)
    s = torch.maximum(torch.cosine_similarity(a, b, dim=-1), torch.cosine_similarity(-a, b, dim=-1))
    return torch.mean(s, dim=-1)[0].numpy()


def fit_rule(points, ori, n_surface, voxel_min=VOXEL_MIN, voxel_size=VOXEL_SIZE, grid=GRID, flip="gt", rounding="rint",
             clip_first=False, tie="first", shell_first=False):
    """PMVO.py:689-726 on the concatenation (surface rows [0, n_surface), then the shell rows): canonicalise, p2v, the members
    of a voxel in point order, the FIRST member of maximal score.  -> (voxels [G,3] int64 ascending by (x, y, z),
    orientations [G,3] float32, scores: the list of each group's member scores)"""
    g = np.asarray(grid).astype(np.int64)
    o = canon_rule(ori, flip)
    k = p2v_rule(points, voxel_min, voxel_size, grid, rounding, clip_first)
    key = (k[:, 0] * g[1] + k[:, 1]) * g[2] + k[:, 2]
    rows = np.arange(len(key))
    if shell_first:
        rows = np.concatenate([rows[n_surface:], rows[:n_surface]])
    order = rows[np.argsort(key[rows], kind="stable")]
    ks = key[order]
    starts = np.flatnonzero(np.concatenate([[True], ks[1:] != ks[:-1]]))
    ends = np.concatenate([starts[1:], [len(ks)]])
    vox, med, scores = [], [], []
    for a, b in zip(starts, ends):
        members = o[order[a:b]]
        s = mean_similarity(members)
        i = int(np.argmax(s)) if tie == "first" else len(s) - 1 - int(np.argmax(s[::-1]))
        vox.append(k[order[a]])
        med.append(members[i])
        scores.append(s)
    return np.array(vox, np.int64).reshape(-1, 3), np.array(med, F).reshape(-1, 3), scores


def voxel_list(occ, ori):
    """dense (occ [X,Y,Z], ori [X,Y,Z,3]) -> (voxels [G,3] int64 ascending, orientations [G,3] float64)"""
    v = np.argwhere(np.asarray(occ) != 0).astype(np.int64)
    return v, np.asarray(ori)[v[:, 0], v[:, 1], v[:, 2]].astype(np.float64)


def bits_equal(a, b):
    """float arrays equal element for element, the sign of every zero included, NaN == NaN"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all(((a == b) & (np.signbit(a) == np.signbit(b))) | (np.isnan(a) & np.isnan(b))))


# ---------------------------------------------------------------------------------------------------------------------------
# inputs that need no reference: the p2v points, the sweep of the 0.95 rule, its degenerate rows
# ---------------------------------------------------------------------------------------------------------------------------
P2V_TARGETS = np.array([0.5, 1.5, 2.5, 3.5, 62.5, 63.5, 126.5, 127.5, -0.5, -1.5, 128.5, 0.0, 127.0, 2147483647.5, 2147483647.4,
                        -2147483648.5, -2147483649.5])


def p2v_points(dtype):
    """[N,3] points of the binary grid: every target index value and every special coordinate on each axis in turn, the two
    other coordinates inside (index 64 and 65)"""
    coords = list(P2V_TARGETS * BIN_SIZE + BIN_MIN[0]) + [-0.0, np.nan, np.inf, -np.inf, 3e9, -3e9]
    rows = []
    for axis in range(3):
        for c in coords:
            p = [0.0, -BIN_SIZE, 2 * BIN_SIZE]
            p[axis] = c if axis == 0 else -c          # (p2v negates y and z)
            rows.append(p)
    return np.array(rows, np.float64).astype(dtype)


DEGENERATE = (0.0, -0.0, 1e-45, 1e-30, float(np.nextafter(F(1e-8), F(0))), 1e-8, float(np.nextafter(F(1e-8), F(1))), 3e19, 3e38,
              np.inf, -np.inf, np.nan)


def cos_sweep(n=20000, seed=5):
    """-> (center [M,3], ori [M,3]) float32: n pairs rotated by acos(0.95) +- 2e-7 with random lengths and signs, then the
    degenerate rows: every DEGENERATE value as a whole row and as one component, in either operand"""
    rng = np.random.default_rng(seed)
    b = rng.normal(size=(n, 3))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    t = rng.normal(size=(n, 3))
    t -= (t * b).sum(1, keepdims=True) * b
    t /= np.linalg.norm(t, axis=1, keepdims=True)
    ang = np.arccos(0.95) + rng.uniform(-2e-7, 2e-7, n)
    a = (np.cos(ang)[:, None] * b + np.sin(ang)[:, None] * t) * rng.uniform(0.3, 3.0, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    b = b * rng.uniform(0.3, 3.0, (n, 1))
    c, o = [b.astype(F)], [a.astype(F)]
    plain = np.array([[0.3, -0.8, 0.52], [1.0, 0.0, 0.0], [-2.0, 1.0, 0.5]], F)
    deg_c, deg_o = [], []
    for v in DEGENERATE:
        for p in plain:
            whole = np.full(3, v, F)
            for k in range(3):
                one = p.copy()
                one[k] = F(v)
                deg_c += [one, p, one, whole, p]
                deg_o += [p, one, one, p, whole]
            deg_c.append(whole)
            deg_o.append(whole)
    with np.errstate(over="ignore"):
        c.append(np.array(deg_c, F))
        o.append(np.array(deg_o, F))
    return np.concatenate(c), np.concatenate(o)
