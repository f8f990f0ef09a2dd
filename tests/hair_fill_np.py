"""The inner-fill rule of include/mh_pmvo.h ("Inner fill") restated in numpy: what the HIP kernels of csrc/hairfill.hip must
equal on every quantity.  The votes are float32 comparisons on the oracle's projection of the float32 voxel centres; the sweeps
are vectorised gathers over a padded map with the six additions in the stated order, float64 elementwise (numpy fuses nothing;
+ - * / sqrt are correctly rounded); np.rint rounds half to even.  tests/test_hair_fill_host.py holds this file to hand-computed
cases."""
import numpy as np

F = np.float32
MAXQ = 2.0 ** 26
NEIGHBOURS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))


# ------------------------------------------------------------------------------------------------- 1. domain votes
def centres(voxels, voxel_min, voxel_size):
    """float32 [n,3]: the world point of each voxel (x, y, z), float64 arithmetic rounded once"""
    v = np.asarray(voxels, np.int64).reshape(-1, 3).astype(np.float64)
    m, vs = np.asarray(voxel_min, np.float64), np.float64(voxel_size)
    return np.stack([m[0] + v[:, 0] * vs, -(m[1] + v[:, 1] * vs), -(m[2] + v[:, 2] * vs)], 1).astype(F)


def grid_voxels(dims, x0=0, x1=None):
    """int64 [(x1 - x0)*Y*Z,3]: the voxels of the slab x0 <= x < x1 (default: the grid) ascending by (x*Y + y)*Z + z"""
    X, Y, Z = (int(d) for d in dims)
    xs = np.arange(x0, X if x1 is None else x1)
    return np.stack(np.meshgrid(xs, np.arange(Y), np.arange(Z), indexing="ij"), -1).reshape(-1, 3).astype(np.int64)


def view_terms(record, depth, mask, bust, pts):
    """one view -> bool [N] x 4: takes part, visible, front, hair.  depth / mask / bust: float32 [H,W] planes"""
    import oracle

    H, W = depth.shape
    # (a point alone in its batch is projected by another product form, include/mh_pmvo.h; the fill projects voxel centres as
    # points of a batch, so one more row goes in and is dropped again)
    pts = np.concatenate([np.asarray(pts, F).reshape(-1, 3), np.zeros((1, 3), F)])
    rc, zp, oob, _ = (a[:-1] for a in oracle.project_points(record, pts, H, W))
    r, c = rc[:, 0], rc[:, 1]
    with np.errstate(invalid="ignore"):
        inside = ~oob & (zp > F(0))
        z255 = (zp * F(255.0)).astype(F)
        visible = ~((z255 - depth[r, c]).astype(F) > F(0.9))
        front = z255 <= bust[r, c]
        hair = mask[r, c] > F(0.2)
    return inside, visible, front, hair


def votes(records, depth, mask, bust, pts):
    """int32 [N,4] = n_in, n_vis, n_front, n_bad over the views.  depth / mask / bust: float32 [V,H,W]"""
    out = np.zeros((len(pts), 4), np.int32)
    for v in range(len(records)):
        inside, visible, front, hair = view_terms(records[v], depth[v], mask[v], bust[v], pts)
        out[:, 0] += inside
        out[:, 1] += inside & visible
        out[:, 2] += inside & front
        out[:, 3] += inside & front & ~hair
    return out


def domain_flags(counts, max_bad=0):
    c = np.asarray(counts).reshape(-1, 4)
    return (c[:, 0] >= 1) & (c[:, 1] <= 2) & (c[:, 2] >= 1) & (c[:, 3] <= int(max_bad))


def domain(counts, dims, ext_voxels=None, max_bad=0):
    """the domain voxels int64 [D,3], ascending by (x*Y + y)*Z + z; counts [X*Y*Z,4] in that order"""
    X, Y, Z = (int(d) for d in dims)
    flags = domain_flags(counts, max_bad).reshape(X, Y, Z).copy()
    if ext_voxels is not None and len(ext_voxels):
        e = np.asarray(ext_voxels, np.int64).reshape(-1, 3)
        flags[e[:, 0], e[:, 1], e[:, 2]] = False
    x, y, z = np.nonzero(flags)          # C order of [X,Y,Z]: ascending key
    return np.stack([x, y, z], 1).astype(np.int64).reshape(-1, 3)


# ------------------------------------------------------------------------------------------------- 2. orientation sweeps
def source_tensors(ext_ori):
    """-> (tensor float64 [G,6] = xx, yy, zz, xy, xz, yz of q = rint(4096 a), source bool [G])"""
    a = np.asarray(ext_ori, F).reshape(-1, 3).astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.rint(4096.0 * a)
        ok = (np.abs(f) <= MAXQ).all(1) & ~(f == 0.0).all(1)          # (NaN fails the first)
    q = np.where(ok[:, None], f, 0.0).astype(np.int64)
    t = np.stack([q[:, 0] * q[:, 0], q[:, 1] * q[:, 1], q[:, 2] * q[:, 2], q[:, 0] * q[:, 1], q[:, 0] * q[:, 2],
                  q[:, 1] * q[:, 2]], 1)
    return t.astype(np.float64), ok


def diffuse(ext_voxels, ext_ori, dom_voxels, dims, sweeps):
    """-> (tensor float64 [D,6], known uint8 [D], depth int32 [D]) after `sweeps` sweeps"""
    X, Y, Z = (int(d) for d in dims)
    ev = np.asarray(ext_voxels, np.int64).reshape(-1, 3)
    dv = np.asarray(dom_voxels, np.int64).reshape(-1, 3)
    G, D = len(ev), len(dv)
    both = np.concatenate([ev, dv])
    if len(both) and (((both < 0) | (both >= np.array([X, Y, Z])[None, :])).any() or len(np.unique(both, axis=0)) != len(both)):
        raise ValueError("the exterior and domain voxels must be unique, disjoint and inside the grid")
    ext_t, src = source_tensors(ext_ori)
    ext_t = np.concatenate([ext_t, np.zeros((1, 6))])          # (a row to gather where there is no exterior)
    src = np.concatenate([src, [False]])
    vmap = np.zeros((X + 2, Y + 2, Z + 2), np.int64)           # padded: a neighbour outside the grid is "none"
    vmap[ev[:, 0] + 1, ev[:, 1] + 1, ev[:, 2] + 1] = -(np.arange(G) + 1)
    vmap[dv[:, 0] + 1, dv[:, 1] + 1, dv[:, 2] + 1] = np.arange(D) + 1
    T, known, depth = np.zeros((D + 1, 6)), np.zeros(D + 1, bool), np.zeros(D, np.int32)
    near = [vmap[dv[:, 0] + 1 + dx, dv[:, 1] + 1 + dy, dv[:, 2] + 1 + dz] for dx, dy, dz in NEIGHBOURS]
    for k in range(1, int(sweeps) + 1):
        S, c = np.zeros((D, 6)), np.zeros(D, np.int64)
        for m in near:                                          # the fixed order
            e = np.where(m < 0, -m - 1, G)
            d = np.where(m > 0, m - 1, D)
            use_e, use_d = src[e], known[d]
            S = S + np.where(use_e[:, None], ext_t[e], np.where(use_d[:, None], T[d], 0.0))
            c += use_e | use_d
        hit = c > 0
        newT = np.where(hit[:, None], S / np.maximum(c, 1).astype(np.float64)[:, None], T[:D])
        depth[hit & ~known[:D]] = k
        T[:D], known[:D] = newT, known[:D] | hit
    return T[:D].copy(), known[:D].astype(np.uint8), depth


# ------------------------------------------------------------------------------------------------- 3. resolve
def resolve(T, known, min_coh=0.0):
    """-> (ori float32 [D,3], coh float64 [D], emit uint8 [D]): the Resolve rule of "Strand volume" on the known rows"""
    T = np.asarray(T, np.float64).reshape(-1, 6)
    xx, yy, zz, xy, xz, yz = (T[:, k] for k in range(6))
    trace = (xx + yy) + zz
    has = (np.asarray(known).reshape(-1) != 0) & (trace > 0.0)
    first = (xx >= yy) & (xx >= zz)
    second = ~first & (yy >= zz)
    vx = np.where(first, xx, np.where(second, xy, xz))
    vy = np.where(first, xy, np.where(second, yy, yz))
    vz = np.where(first, xz, np.where(second, yz, zz))

    def mul(vx, vy, vz):
        return (xx * vx + xy * vy) + xz * vz, (xy * vx + yy * vy) + yz * vz, (xz * vx + yz * vy) + zz * vz

    with np.errstate(all="ignore"):
        for _ in range(24):
            mx, my, mz = mul(vx, vy, vz)
            ln = np.sqrt((mx * mx + my * my) + mz * mz)
            vx, vy, vz = mx / ln, my / ln, mz / ln
        mx, my, mz = mul(vx, vy, vz)
        coh = ((vx * mx + vy * my) + vz * mz) / trace
        flip = vy > 0.0
        v = np.stack([np.where(flip, -vx, vx), np.where(flip, -vy, vy), np.where(flip, -vz, vz)], 1)
        ori = np.where(has[:, None], v, 0.0).astype(F)
        coh = np.where(has, coh, 0.0)
        emit = has & (coh >= np.float64(min_coh))
    return ori.reshape(-1, 3), coh, emit.astype(np.uint8)


def fill(ext_voxels, ext_ori, dom_voxels, dims, sweeps, min_coh=0.0, voxel_min=(-0.32, -0.32, -0.24), voxel_size=0.0025):
    """-> dict(tensor, known, depth, ori, coh, emit, world, rows float32 [M,7])"""
    T, known, depth = diffuse(ext_voxels, ext_ori, dom_voxels, dims, sweeps)
    ori, coh, emit = resolve(T, known, min_coh)
    world = centres(dom_voxels, voxel_min, voxel_size)
    keep = emit != 0
    rows = np.ones((int(keep.sum()), 7), F)
    rows[:, 0:3], rows[:, 3:6] = world[keep], ori[keep]
    return dict(tensor=T, known=known, depth=depth, ori=ori, coh=coh, emit=emit, world=world, rows=rows)
