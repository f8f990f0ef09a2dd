"""Cases for the exact-rational rasteriser reference (tests/raster_exact.py), shared by test_raster_exact_host.py and
test_raster_exact_gpu.py (helper module: no tests, no markers).

A case is a primitive whose window positions are written as integers in 1/256 pixel RELATIVE TO THE CENTRE OF PIXEL (0, 0)
(so 256 * c is the centre of column c whatever "pixel_center" is); `place` turns them into absolute grid positions for a
pixel_center and a sub-pixel grid, and `vertices` into float32 world points of a camera whose projection is benign in
float32 (identity pose, ndc_prj (1, 1, 0, 0), points on planes z = -depth), with the precondition that every vertex
lands within 1/8 of a sub-pixel step of the grid point it is meant for."""
import numpy as np

from monohair_amd.camera import camera_records, cameras_from_list

SIZES = ((32, 64), (32, 48))             # (H, W): powers of two, and one width that is not
CONFIGS = ((0.5, 8), (0.0, 8), (0.5, 4), (0.0, 4))        # (pixel_center, sub-pixel bits)


def camera_record():
    cam = dict(file="front", pose=np.eye(4).tolist(), ndc_prj=[1.0, 1.0, 0.0, 0.0])
    return camera_records(cameras_from_list([cam]))[0]


def place(points, pixel_center, bits):
    """relative 1/256-pixel positions -> absolute ones on the grid of 2^-bits pixel (halves of a coarse step go up)"""
    off, step = int(pixel_center * 256), 256 >> bits
    return [tuple(((int(v) + off + step // 2) // step) * step for v in p) for p in points]


def vertices(points_abs, H, W, bits, depth=1.0):
    """absolute grid positions -> float32 world points [N,3]; depth: one value or one per point"""
    k = np.asarray(points_abs, np.float64).reshape(-1, 2)
    z = -np.broadcast_to(np.asarray(depth, np.float64), (len(k),))
    u, v = 1.0 - 2.0 * (k[:, 0] / 256.0) / W, 2.0 * (k[:, 1] / 256.0) / H - 1.0        # as world() of test_raster_host
    out = np.stack([u * z, v * z, z], 1).astype(np.float32)                            # fx = fy = 1, cx = cy = 0
    # precondition (asserted for every vertex, never skipped): the float64 projection of the float32 vertex is within 1/8
    # of a sub-pixel step of the intended grid point, so that the rasterisers' rintf cannot snap it elsewhere
    p = out.astype(np.float64)
    col = ((-(p[:, 0] / p[:, 2]) + 1.0) / 2.0) * W
    row = (((p[:, 1] / p[:, 2]) + 1.0) / 2.0) * H
    err = max(np.abs(col * 256.0 - k[:, 0]).max(), np.abs(row * 256.0 - k[:, 1]).max()) if len(k) else 0.0
    assert err <= (256 >> bits) / 8.0, "a vertex is %.3g / 256 pixel from its grid point" % err
    return out


def P(c, r, dc=0, dr=0):
    return (256 * c + dc, 256 * r + dr)


def _biased(rng, span):
    """an offset in 1/256 pixel within +-span pixel: multiples of 1/2 and 1/4 pixel strongly over-represented"""
    kind = rng.random()
    if kind < 0.5:
        return int(rng.integers(-2 * span, 2 * span + 1)) * 128
    if kind < 0.8:
        return int(rng.integers(-4 * span, 4 * span + 1)) * 64
    return int(rng.integers(-256 * span, 256 * span + 1))


# ---------------------------------------------------------------------------------------------------------------------
# triangles
# ---------------------------------------------------------------------------------------------------------------------
def fan(centre, ring):
    return [(centre, ring[k], ring[(k + 1) % len(ring)]) for k in range(len(ring))]


def tessellation(H, W):
    """a rectangle with its corners on pixel centres, cut into a 5 x 4 grid of cells whose inner nodes sit on half and
    quarter pixels, every cell split along alternating diagonals -> (corners (x0, y0, x1, y1), triangles)"""
    x0, y0, x1, y1 = 3 * 256, 2 * 256, 23 * 256, 14 * 256
    xs = [x0, x0 + 4 * 256 + 128, x0 + 8 * 256, x0 + 11 * 256 + 64, x0 + 16 * 256 - 128, x1]
    ys = [y0, y0 + 3 * 256, y0 + 5 * 256 + 128, y0 + 9 * 256 - 64, y1]
    tris = []
    for j in range(len(ys) - 1):
        for i in range(len(xs) - 1):
            a, b, c, d = (xs[i], ys[j]), (xs[i + 1], ys[j]), (xs[i + 1], ys[j + 1]), (xs[i], ys[j + 1])
            tris += [(a, b, c), (a, c, d)] if (i + j) % 2 == 0 else [(a, b, d), (b, c, d)]
    return (x0, y0, x1, y1), tris


def triangle_families(H, W, seed=0):
    fam = {}
    ring8 = [P(14, 10), P(14, 14), P(10, 14), P(6, 14), P(6, 10), P(6, 6), P(10, 6), P(14, 6)]
    ring7 = [P(45, 16, 37, -11), P(43, 21, 128, 0), P(38, 22, 0, 64), P(34, 18, -64, 0), P(35, 12, 5, 77), P(40, 9, 0, 128),
             P(44, 11, -128, 128)]
    fam["fan around a vertex on a pixel centre"] = fan(P(10, 10), ring8) + fan(P(40, 16), ring7)
    fam["shared edges through pixel centres"] = [
        (P(5, 3), P(5, 12), P(1, 7)), (P(5, 3), P(5, 12), P(9, 8)),                     # vertical
        (P(12, 6), P(22, 6), P(16, 2)), (P(12, 6), P(22, 6), P(18, 11)),                # horizontal
        (P(25, 3), P(33, 11), P(33, 3)), (P(25, 3), P(33, 11), P(25, 11)),              # 45 degrees, down-right
        (P(44, 3), P(36, 11), P(36, 3)), (P(44, 3), P(36, 11), P(44, 11)),              # 45 degrees, down-left
        (P(12, 16), P(20, 20), P(12, 24)), (P(20, 20), P(12, 24), P(22, 28)),           # slope 1/2 through every 2nd centre
    ]
    fam["tessellated rectangle"] = tessellation(H, W)[1]
    fam["slivers without a centre"] = [
        (P(10, 5, 16, 32), P(16, 5, 16, 64), P(10, 5, 16, 96)),                         # between two rows of centres
        (P(10, 8), P(15, 8), P(12, 8, 0, -96)),                                        # its bottom edge on a row of centres
        (P(20, 3), P(20, 8), P(20, 5, -96, 0)),                                        # its right edge on a column of centres
        (P(30, 10), P(34, 14), P(30, 10, 0, 96)),                                      # its 45-degree upper right edge on centres
        (P(3, 20), P(9, 20), P(15, 20)),                                                # zero area, on the centres
        (P(3, 22), P(3, 22), P(8, 25)),                                                 # two equal vertices
        (P(40, 20, 16, 16), P(40, 20, 240, 16), P(40, 20, 128, 240)),                      # inside the gap of four centres
    ]
    fam["a vertex outside each border"] = [
        (P(-5, 10), P(8, 4), P(8, 16)), (P(20, -6), P(14, 6), P(27, 6)),
        (P(W + 4, 12), P(W - 8, 5), P(W - 8, 20)), (P(30, H + 5), P(24, H - 6), P(37, H - 6)),
        (P(-3, -3), P(6, 0), P(0, 6)), (P(W + 2, H + 2), P(W - 1, H - 7), P(W - 7, H - 1)),
        (P(-40, 5), P(W + 40, 5), P(W // 2, H + 30)),                                   # the whole image below row 5
        (P(-9, 3), P(-2, 3), P(-2, 9)), (P(W - 1, 2, 1, 0), P(W + 5, 2), P(W + 5, 9)),   # entirely outside
    ]
    fam["boxes of 24 and 25 pixels"] = [
        (P(2, 2), P(25, 2), P(2, 2, 0, 200)), (P(2, 4), P(26, 4), P(2, 4, 0, 208)),     # 24 x 1 and, scaled 24/23, 25 x 1
        (P(30, 2), P(30, 25), P(30, 2, 200, 0)), (P(34, 2), P(34, 26), P(34, 2, 208, 0)),   # 1 x 24, 1 x 25
        (P(40, 2), P(45, 2), P(40, 5)), (P(40, 8), P(44, 8), P(40, 12)),                # 6 x 4 and 5 x 5
        (P(W - 5, H - 4), P(W + 1, H - 4), P(W - 5, H)),                                # 7 x 5 clamped to 5 x 4 ... 20
        (P(W - 5, H - 10), P(W + 3, H - 10), P(W - 5, H - 5)),                          # 9 x 6 clamped to 5 x 6 = 30
        (P(-1, 10), P(5, 10), P(-1, 14)), (P(-1, 16), P(4, 16, 64, 0), P(-1, 20, 0, 64)),   # 7 x 5 clamped to 6 x 4 = 24; 25
        (P(8, 12), P(15, 12), P(8, 14)), (P(8, 16), P(15, 16, 1, 0), P(8, 18, 0, 1)),   # 8 x 3 = 24 and just beyond it
    ]
    rng = np.random.default_rng(seed)
    sweep = []
    for _ in range(160):
        c, r = int(rng.integers(-2, W + 2)), int(rng.integers(-2, H + 2))
        sweep.append(tuple(P(c, r, _biased(rng, 3), _biased(rng, 3)) for _ in range(3)))
    fam["seeded sweep"] = sweep
    return fam


# ---------------------------------------------------------------------------------------------------------------------
# segments
# ---------------------------------------------------------------------------------------------------------------------
DIRS = [(5, 0), (5, 2), (5, 5), (2, 5), (0, 5), (-2, 5), (-5, 5), (-5, 2), (-5, 0), (-5, -2), (-5, -5), (-2, -5), (0, -5),
        (2, -5), (5, -5), (5, -2)]          # eight octants and the exact 0, 45 and 90 degrees between them, both senses
# end-point positions relative to a pixel centre: the centre, the four corners of its diamond, points on its four edges
# (both halves), exactly between two pixels in either coordinate and diagonally, and two positions off every tie
SPOTS = [(0, 0), (128, 0), (-128, 0), (0, 128), (0, -128), (64, 64), (-64, 64), (64, -64), (-64, -64), (32, 96), (-96, 32),
         (96, -32), (-32, -96), (128, 128), (-128, 128), (128, 64), (37, -11), (-90, 101)]


def polyline(H, W):
    """a chain whose consecutive segments share end points, the joints on centres, diamond corners and diamond edges"""
    pts = [P(3, 20), P(8, 20), P(12, 22, 128, 0), P(15, 25, 0, 128), P(15, 28, 64, 64), P(20, 28, -64, 64), P(24, 24),
           P(24, 20, 0, -128), P(28, 16, 32, 96), P(33, 16, -128, 0), P(33, 12), P(29, 12, 37, -11), P(26, 9, 128, 128),
           P(26, 9, 200, 150), P(27, 9, 0, 100), P(30, 6), P(36, 6, 128, 0), P(36, 6, 230, 40), P(40, 10), P(44, 11), P(45, 15),
           P(41, 17)]      # (the last three: crossings half-way between two rows, two columns, two rows)
    return [(pts[i], pts[i + 1]) for i in range(len(pts) - 1)]


def segment_families(H, W, seed=1):
    fam = {}
    fam["octants, 0, 45 and 90 degrees, both directions"] = [
        (P(20, 14, *s), P(20 + dx, 14 + dy, *e)) for dx, dy in DIRS for s, e in (((0, 0), (0, 0)), ((64, 64), (-64, 64)),
                                                                                 ((128, 0), (0, 128)), ((37, -11), (128, 128)))]
    ends = []
    for k, s in enumerate(SPOTS):
        for dx, dy in (DIRS[(3 * k) % 16], DIRS[(3 * k + 5) % 16], DIRS[(3 * k + 10) % 16]):
            far = P(30 + dx, 16 + dy, 45, 23)
            ends += [(P(30, 16, *s), far), (far, P(30, 16, *s))]
    for s in SPOTS:
        for e in SPOTS[1:9]:
            ends.append((P(8, 8, *s), P(13, 10, *e)))
    fam["end points on centres, corners, edges and half-way"] = ends
    one = [((-50, 0), (50, 10)), ((-128, 0), (128, 0)), ((0, -128), (0, 128)), ((-64, -64), (64, 64)), ((128, 0), (0, 128)),
           ((0, 128), (-128, 0)), ((-128, 0), (0, -128)), ((0, -128), (128, 0)), ((0, 0), (64, 64)), ((64, 64), (0, 0)),
           ((-30, 40), (20, -70)), ((0, 0), (128, 0)), ((128, 0), (0, 0)), ((0, 0), (-128, 0)), ((0, 0), (0, 128)),
           ((0, 128), (0, 0)), ((0, 0), (0, -128)), ((-64, 64), (64, 64)), ((64, -64), (64, 64)), ((10, 10), (10, 10))]
    fam["inside one diamond"] = [(P(12, 9, *s), P(12, 9, *e)) for s, e in one]
    short = [((100, 0), (300, 30)), ((128, 0), (384, 0)), ((127, 0), (129, 0)), ((0, 127), (0, 129)), ((128, 128), (250, 200)),
             ((-20, 100), (180, 140)), ((0, 128), (200, 128)), ((200, 128), (0, 128)), ((128, -60), (128, 190)),
             ((64, 64), (192, 192)), ((192, 192), (64, 64)), ((64, 192), (192, 64)), ((0, 0), (255, 255)), ((255, 0), (0, 255)),
             ((128, 0), (128, 255)), ((129, 255), (128, 1)), ((-1, 128), (254, 128)), ((120, 100), (140, 160))]
    fam["major length below one pixel"] = [(P(40, 20, *s), P(40, 20, *e)) for s, e in short]
    fam["crossing each image border"] = [
        (P(-4, 10), P(5, 12)), (P(5, 12), P(-4, 10)), (P(W + 3, 8, 0, 128), P(W - 6, 8, 0, 128)), (P(W - 6, 3), P(W + 3, 7)),
        (P(20, -5), P(22, 6)), (P(22, 6, 128, 0), P(22, -5, 128, 0)), (P(30, H + 4), P(33, H - 7)), (P(33, H - 7), P(30, H + 4)),
        (P(-3, -3), P(6, 6)), (P(W + 2, H + 2), P(W - 6, H - 6)), (P(-6, H - 3), P(5, H + 4)), (P(W - 4, -5), P(W + 5, 4)),
        (P(-20, 16, 0, 128), P(W + 20, 18, 0, 128)), (P(W // 2, -20), P(W // 2 + 3, H + 20)),
        (P(0, 3, -128, 0), P(4, 3)), (P(4, 5), P(0, 5, -128, 0)), (P(W - 1, 3, 128, 0), P(W - 5, 3)),
        (P(W - 5, 5), P(W - 1, 5, 128, 0)), (P(7, 0, 0, -128), P(7, 4)), (P(9, 4), P(9, 0, 0, -128)),
        (P(7, H - 1, 0, 128), P(7, H - 5)), (P(9, H - 5), P(9, H - 1, 0, 128)), (P(-9, 5), P(-2, 7)), (P(5, H + 1), P(12, H + 2)),
    ]
    fam["bands cut by the first and last row and column"] = [
        (P(3, 0), P(12, 0)), (P(12, 0, 0, 128), P(3, 1)), (P(14, 0, 0, -128), P(22, 2)), (P(22, -1), P(30, 1)),
        (P(3, H - 1), P(12, H - 1)), (P(12, H - 1, 0, 128), P(3, H - 2)), (P(14, H - 2, 0, 128), P(22, H - 1)), (P(22, H), P(30, H - 2)),
        (P(0, 4), P(0, 12)), (P(0, 12, 128, 0), P(1, 4)), (P(-1, 14), P(1, 22)), (P(0, 22, -128, 0), P(2, 28)),
        (P(W - 1, 4), P(W - 1, 12)), (P(W - 1, 12, 128, 0), P(W - 2, 4)), (P(W, 14), P(W - 2, 22)), (P(W - 2, 22, 128, 0), P(W, 28)),
        (P(-2, 0), P(3, 0)), (P(W - 3, H - 1), P(W + 2, H - 1)), (P(0, -2), P(0, 3)), (P(W - 1, H - 3), P(W - 1, H + 2)),
        (P(W - 3, 0), P(W + 2, 2)), (P(1, H - 3), P(-2, H + 2)),
    ]
    fam["polyline with shared end points"] = polyline(H, W)
    rng = np.random.default_rng(seed)
    sweep = []
    for _ in range(260):
        c, r = int(rng.integers(-2, W + 2)), int(rng.integers(-2, H + 2))
        sweep.append((P(c, r, _biased(rng, 1), _biased(rng, 1)), P(c, r, _biased(rng, 4), _biased(rng, 4))))
    fam["seeded sweep"] = sweep
    return fam


def disjoint_groups(sets):
    """greedy partition of primitive indices into groups whose pixel sets are pairwise disjoint (non-empty sets only)"""
    groups = []
    for i, s in enumerate(sets):
        if not s:
            continue
        for g in groups:
            if not (g[1] & s):
                g[0].append(i)
                g[1] |= s
                break
        else:
            groups.append([[i], set(s)])
    return [g[0] for g in groups]
