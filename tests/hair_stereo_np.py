"""The photo-consistent carve of include/mh_pmvo.h ("Photo-consistent carve") restated in numpy from the header text alone: what
the HIP kernels of csrc/hairstereo.hip must equal on every quantity.  The per-(voxel, view) terms are those of
tests/hair_fill_np.py (view_terms: the abstention, `front` = free, `hair`) on the oracle's projection of the float32 voxel
centres, which also gives the rounded and clamped pixel and z'; everything after them is integer arithmetic, written as plain
loops over the views with numpy over the voxels.  tests/test_hair_stereo_host.py holds this file to hand-computed cases."""
import numpy as np

import hair_fill_np as FILL

F = np.float32
NONE = np.uint64(0xFFFFFFFFFFFFFFFF)
centres, grid_voxels = FILL.centres, FILL.grid_voxels


# ------------------------------------------------------------------------------------------------- 1. reduced images, census
def reduce_gray(gray, cell):
    """uint8 [V,H,W] -> uint8 [V,Hc,Wc]: (2*sum + n) // (2*n) over the n existing pixels of each block"""
    gray = np.asarray(gray, np.uint8)
    V, H, W = gray.shape
    cell = int(cell)
    Hc, Wc = -(-H // cell), -(-W // cell)
    out = np.zeros((V, Hc, Wc), np.uint8)
    for i in range(Hc):
        for j in range(Wc):
            block = gray[:, i * cell:(i + 1) * cell, j * cell:(j + 1) * cell].astype(np.int64).reshape(V, -1)
            n = block.shape[1]
            out[:, i, j] = (2 * block.sum(1) + n) // (2 * n)
    return out


def census(g, radius):
    """uint8 [V,Hc,Wc] -> uint64 [V,Hc,Wc]: bit b = g[clamped neighbour b] < g[centre], row-major offsets, centre left out"""
    g = np.asarray(g, np.uint8)
    V, Hc, Wc = g.shape
    rows, cols = np.arange(Hc)[:, None], np.arange(Wc)[None, :]
    code = np.zeros(g.shape, np.uint64)
    b = 0
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            near = g[:, np.clip(rows + dy, 0, Hc - 1), np.clip(cols + dx, 0, Wc - 1)]
            code |= (near < g).astype(np.uint64) << np.uint64(b)
            b += 1
    return code


def popcount(a):
    a = np.ascontiguousarray(a, np.uint64)
    return np.unpackbits(a.view(np.uint8).reshape(a.shape + (8,)), axis=-1).sum(-1).astype(np.int64)


# ------------------------------------------------------------------------------------------------- 2. per (voxel, view) terms
class Terms:
    """of every voxel of the grid in every view: seen (does not abstain), free (seen and not hidden by the bust), takes (free
    and hair) bool [V,N]; cell int64 [V,N] = (row // cell) * Wc + col // cell; z255 float32 [V,N]"""

    def __init__(self, records, mask, bust, voxel_min, voxel_size, dims, cell):
        import oracle

        mask, bust = np.asarray(mask, F), np.asarray(bust, F)
        V, H, W = mask.shape
        self.V, self.H, self.W, self.cell_size = V, H, W, int(cell)
        self.Hc, self.Wc = -(-H // self.cell_size), -(-W // self.cell_size)
        self.dims = tuple(int(d) for d in dims)
        self.nvox = self.dims[0] * self.dims[1] * self.dims[2]
        pts = centres(grid_voxels(self.dims), voxel_min, voxel_size)
        nowhere = np.zeros((H, W), F)
        self.seen, self.free, self.takes = (np.zeros((V, self.nvox), bool) for _ in range(3))
        self.cell, self.z255 = np.zeros((V, self.nvox), np.int64), np.zeros((V, self.nvox), F)
        batch = np.concatenate([pts, np.zeros((1, 3), F)])          # (view_terms: a point alone is projected otherwise)
        for v in range(V):
            inside, _, free, hair = FILL.view_terms(records[v], nowhere, mask[v], bust[v], pts)
            rc, zp, _, _ = (a[:-1] for a in oracle.project_points(records[v], batch, H, W))
            self.seen[v], self.free[v], self.takes[v] = inside, inside & free, inside & free & hair
            self.cell[v] = (rc[:, 0] // self.cell_size) * self.Wc + rc[:, 1] // self.cell_size
            with np.errstate(invalid="ignore"):
                self.z255[v] = (zp * F(255.0)).astype(F)


# ------------------------------------------------------------------------------------------------- 3. cost and winners
def costs(t, codes, neighbours, radius, keep, cand):
    """-> (cost int64 [V,C], has bool [V,C]) of the candidates `cand` (linear indices) in every view"""
    nb = np.asarray(neighbours, np.int64).reshape(t.V, -1)
    B = (2 * int(radius) + 1) ** 2 - 1
    codes = np.asarray(codes, np.uint64).reshape(t.V, -1)
    cand = np.asarray(cand, np.int64).reshape(-1)
    cost, has = np.zeros((t.V, len(cand)), np.int64), np.zeros((t.V, len(cand)), bool)
    big = 1 << 20
    for r in range(t.V):
        mine = codes[r][t.cell[r][cand]]
        h = []
        for n in nb[r]:
            if n < 0 or n >= t.V or n == r:
                continue
            d = popcount(mine ^ codes[n][t.cell[n][cand]])
            h.append(np.where(t.takes[n][cand], d, big))
        if not h:
            continue
        h = np.sort(np.stack(h, 1), axis=1)
        enough = (h < big).sum(1) >= keep
        S = h[:, :keep].sum(1)
        has[r] = t.takes[r][cand] & enough
        cost[r] = np.where(has[r], (1024 * S) // (B * keep), 0)
    return cost, has


def winners(t, codes, neighbours, radius, keep, cand):
    """-> uint64 [V,Hc,Wc]: per (view, cell) the minimum of (cost << 32) | linear index, all ones where there is none"""
    cand = np.asarray(cand, np.int64).reshape(-1)
    cand = cand[(cand >= 0) & (cand < t.nvox)]
    cost, has = costs(t, codes, neighbours, radius, keep, cand)
    keys = np.full((t.V, t.Hc * t.Wc), NONE, np.uint64)
    for r in range(t.V):
        w = cand[has[r]]
        k = (cost[r][has[r]].astype(np.uint64) << np.uint64(32)) | w.astype(np.uint64)
        np.minimum.at(keys[r], t.cell[r][w], k)
    return keys.reshape(t.V, t.Hc, t.Wc)


def valid_keys(t, keys, max_cost):
    """-> (valid bool [V,Hc*Wc], index int64 [V,Hc*Wc]) of every cell's key"""
    keys = np.asarray(keys, np.uint64).reshape(t.V, -1)
    idx = (keys & np.uint64(0xFFFFFFFF)).astype(np.int64)
    ok = (keys != NONE) & ((keys >> np.uint64(32)).astype(np.int64) <= int(max_cost)) & (idx < t.nvox)
    return ok, np.where(ok, idx, 0)


# ------------------------------------------------------------------------------------------------- 4. agreement
def agree(t, flags, keys, max_cost, m255):
    """-> int32 [X*Y*Z]"""
    f = np.asarray(flags).reshape(-1) != 0
    ok, idx = valid_keys(t, keys, max_cost)
    out = np.zeros(t.nvox, np.int32)
    for r in range(t.V):
        c = t.cell[r]
        star = t.z255[r][idx[r][c]]
        with np.errstate(invalid="ignore"):
            near = np.abs((t.z255[r] - star).astype(F)) <= F(m255)
        out += f & t.takes[r] & ok[r][c] & near
    return out


# ------------------------------------------------------------------------------------------------- 5. refinement
def through(t, flags, keys, agreement, max_cost, m255, min_agree):
    f = np.asarray(flags).reshape(-1) != 0
    ok, idx = valid_keys(t, keys, max_cost)
    agreement = np.asarray(agreement).reshape(-1)
    out = np.zeros(t.nvox, np.int32)
    for r in range(t.V):
        c = t.cell[r]
        confirmed = ok[r][c] & (agreement[idx[r][c]] >= int(min_agree))
        with np.errstate(invalid="ignore"):
            front = (t.z255[r] + F(m255)).astype(F) < t.z255[r][idx[r][c]]
        out += f & t.free[r] & confirmed & front
    return out


def refine(t, flags, keys, agreement, max_cost, m255, min_agree, min_through):
    """-> (refined uint8 [X*Y*Z], depth float32 [V,Hc,Wc])"""
    f = np.asarray(flags).reshape(-1) != 0
    n = through(t, flags, keys, agreement, max_cost, m255, min_agree)
    ok, idx = valid_keys(t, keys, max_cost)
    confirmed = ok & (np.asarray(agreement).reshape(-1)[idx] >= int(min_agree))
    depth = np.full(ok.shape, 255.0, F)
    for r in range(t.V):
        depth[r] = np.where(confirmed[r], t.z255[r][idx[r]], F(255.0))
    return (f & (n < int(min_through))).astype(np.uint8), depth.reshape(t.V, t.Hc, t.Wc)


def stereo(records, gray, mask, bust, voxel_min, voxel_size, dims, flags, neighbours, cell, radius, keep, max_cost, m255,
           min_agree, min_through):
    """every stage -> dict(reduced, census, keys, agree, refined, depth, terms)"""
    t = Terms(records, mask, bust, voxel_min, voxel_size, dims, cell)
    g = reduce_gray(gray, cell)
    codes = census(g, radius)
    cand = np.flatnonzero(np.asarray(flags).reshape(-1) != 0)
    keys = winners(t, codes, neighbours, radius, keep, cand)
    a = agree(t, flags, keys, max_cost, m255)
    refined, depth = refine(t, flags, keys, a, max_cost, m255, min_agree, min_through)
    return dict(reduced=g, census=codes, keys=keys, agree=a, refined=refined, depth=depth, terms=t)
