"""Shared by tests/test_hair_fill_host.py and tests/test_hair_fill_gpu.py: the hand-made cases of the inner fill
(include/mh_pmvo.h, "Inner fill") and the seeded ones.  numpy only; nothing from the GPU side.

The hand-made vote scene.  An 8 x 8 x 2 grid of 1/16 voxels from (-0.25, -0.25, -0.5), seen by eight views of 8 x 8 pixels: five
copies of camera A (at (0, 0, 1), looking down -z, ndc_prj [2, 2, 0, 0]) and three of camera B (at (0, 0, 0.5 + 1/128)).  Every
number is dyadic, so in an A view the centre of voxel (x, y, 0) lands exactly on pixel (row y, column x) with z' * 255 = 63.75,
and in a B view the centre of voxel (4, 4, 0) lands on pixel (4, 4) with z' * 255 = 255/256 while the rest of that layer lies
outside the image.  The planes differ per view and per pixel, so each voxel of the layer z = 0 is one case."""
import numpy as np

F = np.float32
HAND_DIMS, HAND_VMIN, HAND_VS = (8, 8, 2), (-0.25, -0.25, -0.5), 1.0 / 16.0
HAND_H = HAND_W = 8
N_A, N_B = 5, 3
Z255_A, Z255_B = F(63.75), F(255.0 / 256.0)
GAP = F(0.9)
GAPS_B = (np.nextafter(GAP, F(0)), GAP, np.nextafter(GAP, F(1)))       # per B view: below, on and above the bound


def hand_cameras():
    cams = []
    for i in range(N_A + N_B):
        c2w = np.eye(4)
        c2w[2, 3] = 1.0 if i < N_A else 0.5 + 1.0 / 128.0
        cams.append(dict(file="view_%d" % i, pose=c2w.tolist(), ndc_prj=[2.0, 2.0, 0.0, 0.0]))
    return cams


def hand_planes(mask_lut):
    """-> (depth, mask, bust float32 [8,8,8], expected: {(x, y): (n_in, n_vis, n_front, n_bad)} for voxels of the layer z = 0).
    mask_lut: float32 [256], what the loaders make of a mask code.  By default a pixel has a surface far in front of the voxel
    (not visible), no bust (in front of it) and hair: an A-view default voxel counts (5, 0, 5, 0)."""
    V = N_A + N_B
    depth = np.zeros((V, HAND_H, HAND_W), F)
    bust = np.full((V, HAND_H, HAND_W), 255.0, F)
    mask = np.ones((V, HAND_H, HAND_W), F)
    want = {}
    # n_vis of 2 and 3: visible in views 0, 1 (, 2)
    depth[0:2, 0, 0] = Z255_A
    want[(0, 0)] = (5, 2, 5, 0)
    depth[0:3, 0, 1] = Z255_A
    want[(1, 0)] = (5, 3, 5, 0)
    # n_front of 0 and 1: the bust's surface in front of the voxel in every view / in all but view 0
    bust[:N_A, 0, 2] = 0.0
    want[(2, 0)] = (5, 0, 0, 0)
    bust[1:N_A, 0, 3] = 0.0
    want[(3, 0)] = (5, 0, 1, 0)
    # n_bad of 1 (in front of the bust on a pixel that is not hair) and of 0 (not hair, but behind the bust)
    mask[0, 0, 4] = 0.0
    want[(4, 0)] = (5, 0, 5, 1)
    mask[0, 0, 5] = 0.0
    bust[0, 0, 5] = 0.0
    want[(5, 0)] = (5, 0, 4, 0)
    # z255 equal to the bust plane (in front) and one float32 ulp behind it, in view 0; behind it in the others
    bust[:N_A, 1, 0] = 0.0
    bust[0, 1, 0] = Z255_A
    want[(0, 1)] = (5, 0, 1, 0)
    bust[:N_A, 1, 1] = 0.0
    bust[0, 1, 1] = np.nextafter(Z255_A, F(0))
    want[(1, 1)] = (5, 0, 0, 0)
    # mask codes 51 (float32(51 / 255) is float32(0.2): not hair) and 52
    mask[0, 1, 2] = mask_lut[51]
    want[(2, 1)] = (5, 0, 5, 1)
    mask[0, 1, 3] = mask_lut[52]
    want[(3, 1)] = (5, 0, 5, 0)
    # a gap of exactly 0.9f and its two neighbours: voxel (4, 4, 0) in the three B views
    for k, g in enumerate(GAPS_B):
        d = F(Z255_B - g)
        assert F(Z255_B - d) == g and np.float64(Z255_B) - np.float64(g) == np.float64(d)      # the gap is exact
        depth[N_A + k, 4, 4] = d
    want[(4, 4)] = (8, 2, 8, 0)
    want[(6, 6)] = (5, 0, 5, 0)
    return depth, mask, bust, want


def plates():
    """Two parallel exterior plates x = 0 (direction (1, 0, 0)) and x = 4 (direction (0, -1, 0)) of a 5 x 3 x 3 grid, three voxels
    apart, and the domain: the line (1..3, 1, 1) between them.  a = 4096^2; A = (a, 0, 0, 0, 0, 0), B = (0, a, 0, 0, 0, 0).
    -> (dims, ext_voxels, ext_ori, dom_voxels, expected: sweeps -> (tensor rows, known, depth))"""
    dims = (5, 3, 3)
    yz = [(y, z) for y in range(3) for z in range(3)]
    ext = np.array([(0, y, z) for y, z in yz] + [(4, y, z) for y, z in yz], np.int64)
    ori = np.array([(1, 0, 0)] * 9 + [(0, -1, 0)] * 9, F)
    dom = np.array([(1, 1, 1), (2, 1, 1), (3, 1, 1)], np.int64)
    a = 4096.0 * 4096.0

    def t(xx, yy):
        return [xx * a, yy * a, 0.0, 0.0, 0.0, 0.0]

    want = {0: ([t(0, 0), t(0, 0), t(0, 0)], [0, 0, 0], [0, 0, 0]),
            1: ([t(1, 0), t(0, 0), t(0, 1)], [1, 0, 1], [1, 0, 1]),
            2: ([t(1, 0), t(0.5, 0.5), t(0, 1)], [1, 1, 1], [1, 2, 1]),
            3: ([t(0.75, 0.25), t(0.5, 0.5), t(0.25, 0.75)], [1, 1, 1], [1, 2, 1])}
    return dims, ext, ori, dom, want


def seeded_sparse(dims, n_ext, n_dom, seed, faces=False):
    """a seeded sparse exterior (unit directions, a few of them zero, NaN or tiny: no sources) and a disjoint domain of n_dom
    voxels clustered around it; faces: the domain also holds the centre voxel of each of the six faces of the grid"""
    rng = np.random.default_rng([seed, dims[0], n_ext, n_dom])
    X, Y, Z = dims
    nvox = X * Y * Z
    lin = rng.permutation(nvox)
    must = []
    if faces:
        must = [(0, Y // 2, Z // 2), (X - 1, Y // 2, Z // 2), (X // 2, 0, Z // 2), (X // 2, Y - 1, Z // 2), (X // 2, Y // 2, 0),
                (X // 2, Y // 2, Z - 1), (0, 0, 0), (X - 1, Y - 1, Z - 1)]
        key = [(x * Y + y) * Z + z for x, y, z in must]
        lin = np.concatenate([key, lin[~np.isin(lin, key)]])
    assert n_ext + n_dom <= nvox and n_dom >= len(must)
    dom_lin, ext_lin = lin[:n_dom], lin[n_dom:n_dom + n_ext]

    def vox(l):
        return np.stack([l // (Y * Z), (l // Z) % Y, l % Z], 1).astype(np.int64).reshape(-1, 3)

    ori = rng.normal(size=(n_ext, 3))
    ori /= np.linalg.norm(ori, axis=1, keepdims=True)
    ori = ori.astype(F)
    for k, bad in enumerate(((0, 0, 0), (np.nan, 0, 1), (1e-5, -1e-5, 0), (np.inf, 0, 0), (0, 3e4, 0))):
        if k < n_ext:
            ori[k * max(1, n_ext // 7)] = bad
    return vox(ext_lin), ori, vox(np.sort(dom_lin))
