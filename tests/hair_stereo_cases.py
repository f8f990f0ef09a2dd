"""Shared by tests/test_hair_stereo_host.py and tests/test_hair_stereo_gpu.py: the cases of the photo-consistent carve
(include/mh_pmvo.h, "Photo-consistent carve").  numpy only; nothing from the GPU side.

1. The hand-made scenes, on the dyadic cameras of tests/hair_fill_cases.py (five copies of camera A, views 0..4, three of camera
B, views 5..7; 8 x 8 pixels; the 8 x 8 x 2 grid).  In an A view the voxels (x, y, 0) and (x, y, 1) both land on pixel (row y,
column x), with z255 = Z0 = 63.75 and Z1 = 71.71875; in a B view only (4, 4, 0) and (4, 4, 1) are inside the image, on pixel
(4, 4), with z255 = 255/256 and 255/256 + GAP.  GAP = Z1 - Z0 = 7.96875 in every view.  The voxel (x, y, z) has the linear
index (x*8 + y)*2 + z.  The neighbour table NB gives view 4 no neighbour, views 1 and 6 one and a padding -1, the rest two.
The images are flat (100) except where a case needs a census code; with radius 1 (B = 8 bits, offsets (-1,-1) (-1,0) (-1,1)
(0,-1) (0,1) (1,-1) (1,0) (1,1) = bits 0..7) a pixel brighter than its eight neighbours has the code 0xFF and leaves theirs 0.

hand_scene_wide has tables of four (HAND_NB4) and seven (HAND_NB7) columns and census codes whose distances are known by hand.

2. The textured sphere: 12 views of 48 x 48 on a ring round a sphere whose images are evaluated analytically from the
ray-sphere intersection through a seeded smooth 3D texture, with a grid of 32^3 voxels of 1/128; a control with a texture of
its own per view; neighbour tables of any width with shuffled columns (sphere_table); a thirteenth view inside the grid
(inside_cameras)."""
import numpy as np

import hair_fill_cases as C

F = np.float32
Z0, Z1 = F(63.75), F(71.71875)
GAP = F(7.96875)
assert F(Z1 - Z0) == GAP
HAND_NB = np.array([[1, 2], [0, -1], [3, 4], [2, 4], [-1, -1], [6, 7], [5, -1], [0, 1]], np.int32)
V_HAND = C.N_A + C.N_B


def idx(x, y, z):
    return (x * 8 + y) * 2 + z


def key(cost, x, y, z):
    return np.uint64((cost << 32) | idx(x, y, z))


NONE = np.uint64(0xFFFFFFFFFFFFFFFF)


def hand_scene_one():
    """cell 1.  -> dict(gray uint8 [8,8,8], mask, bust float32 [8,8,8], flags uint8 [8,8,2], keys: {keep: {(view, row, col):
    expected key}}, agree: {(keep, max_cost, margin name): {(x, y, z): count}})"""
    gray = np.full((V_HAND, 8, 8), 100, np.uint8)
    gray[0, 2, 2] = gray[2, 2, 2] = 110          # views 0 and 2: pixel (2, 2) has the code 0xFF; view 1 and the rest: 0
    gray[3, 4, 4:7] = 90                         # view 3: pixel (5, 5) sees three darker pixels above it -> bits 0, 1, 2
    mask = np.ones((V_HAND, 8, 8), F)
    mask[2, 6, 1] = 0.0                          # view 2 takes no part in the voxels (1, 6, .)
    bust = np.full((V_HAND, 8, 8), 255.0, F)
    flags = np.ones((8, 8, 2), np.uint8)
    flags[3, 6, 0] = 0                           # cell (6, 3) has the layer-1 voxel alone
    k1 = {
        # view 0, row [1, 2]: at (2, 2) h_1 = popcount(0xFF ^ 0) = 8, h_2 = popcount(0xFF ^ 0xFF) = 0; the smallest is 0
        (0, 2, 2): key(0, 2, 2, 0), (0, 0, 0): key(0, 0, 0, 0), (0, 6, 1): key(0, 1, 6, 0),
        (0, 6, 3): key(0, 3, 6, 1),              # the only candidate of its cell
        # view 1, row [0, -1]: h_0 = 8 -> 1024 * 8 // (8 * 1)
        (1, 2, 2): key(1024, 2, 2, 0), (1, 7, 7): key(0, 7, 7, 0),
        # view 2, row [3, 4]: both neighbours are flat at (2, 2): 8 and 8; no hair at (6, 1): no winner
        (2, 2, 2): key(1024, 2, 2, 0), (2, 6, 1): NONE, (2, 5, 5): key(0, 5, 5, 0),
        # view 3, row [2, 4]: three bits against two flat views: 1024 * 3 // 8; pixel (3, 3) sees (4, 4) at (+1, +1): one bit
        (3, 5, 5): key(384, 5, 5, 0), (3, 3, 3): key(128, 3, 3, 0), (3, 4, 4): key(0, 4, 4, 0),
        (3, 2, 2): key(0, 2, 2, 0),              # h_2 = 8, h_4 = 0
        (3, 6, 1): key(0, 1, 6, 0),              # view 2 takes no part: view 4 alone, enough for keep = 1
        (4, 0, 0): NONE, (4, 4, 4): NONE,        # a row of -1: never a cost
        (5, 4, 4): key(0, 4, 4, 0), (5, 0, 0): NONE, (6, 4, 4): key(0, 4, 4, 0), (7, 4, 4): key(0, 4, 4, 0),
    }
    k2 = dict(k1)
    k2.update({
        (0, 2, 2): key(512, 2, 2, 0),            # 1024 * (0 + 8) // (8 * 2)
        (0, 6, 1): NONE,                         # one neighbour takes part: fewer than keep
        (1, 2, 2): NONE, (1, 7, 7): NONE,        # a padded row has one neighbour at most
        (2, 5, 5): key(192, 5, 5, 0),            # h_3 = 3, h_4 = 0 -> 1024 * 3 // 16
        (3, 5, 5): key(384, 5, 5, 0),            # 1024 * 6 // 16
        (3, 3, 3): key(128, 3, 3, 0), (3, 2, 2): key(512, 2, 2, 0), (3, 6, 1): NONE, (6, 4, 4): NONE,
    })
    below, above = np.nextafter(GAP, F(0)), np.nextafter(GAP, F(100))
    agree = {
        # keep 1, every cost valid: the A views 0..3 hold a key in every cell (view 2 not at (6, 1)), the B views at (4, 4)
        (1, 1024, GAP): {(0, 0, 0): 4, (0, 0, 1): 4, (4, 4, 0): 7, (4, 4, 1): 7, (1, 6, 0): 3, (1, 6, 1): 3, (3, 6, 1): 4,
                         (3, 6, 0): 0},
        # a margin one float32 below the gap: a layer-1 voxel agrees with no layer-0 winner; a winner agrees with itself
        (1, 1024, below): {(0, 0, 0): 4, (0, 0, 1): 0, (4, 4, 0): 7, (4, 4, 1): 0, (3, 6, 1): 4},
        (1, 1024, above): {(0, 0, 1): 4, (4, 4, 1): 7},
        # max_cost on the cost of view 3's cell (5, 5) and one below it; (2, 2) costs 1024 in views 1 and 2
        (1, 384, GAP): {(5, 5, 0): 4, (5, 5, 1): 4, (2, 2, 0): 2},
        (1, 383, GAP): {(5, 5, 0): 3, (5, 5, 1): 3, (2, 2, 0): 2},
        # keep 2: views 0, 2 and 3 hold keys among the A views, 5 and 7 among the B views
        (2, 1024, GAP): {(0, 0, 0): 3, (0, 0, 1): 3, (4, 4, 0): 5, (1, 6, 0): 0},
    }
    return dict(gray=gray, mask=mask, bust=bust, flags=flags, keys={1: k1, 2: k2}, agree=agree, cell=1, radius=1)


def hand_scene_two():
    """cell 2, keep 2, flat images (every census 0, every cost 0): the through test.  Pixel (0, 0) is no hair in the A views, so
    the candidate w = (0, 0, 0) takes part nowhere but is free everywhere; the winner of its cell (0, 0) is w* = (0, 1, 1), a
    layer behind it, in the views 0, 2 and 3 that hold keys; u = (1, 1, 0) of the same cell takes part and loses on the index;
    (6, 6, 0) wins cell (3, 3) and (6, 6, 1) lies behind it."""
    gray = np.full((V_HAND, 8, 8), 100, np.uint8)
    mask = np.ones((V_HAND, 8, 8), F)
    mask[:C.N_A, 0, 0] = 0.0
    bust = np.full((V_HAND, 8, 8), 255.0, F)
    flags = np.zeros((8, 8, 2), np.uint8)
    for v in ((0, 0, 0), (0, 1, 1), (1, 1, 0), (6, 6, 0), (6, 6, 1)):
        flags[v] = 1
    keys = {(r, 0, 0): key(0, 0, 1, 1) for r in (0, 2, 3)}
    keys.update({(r, 3, 3): key(0, 6, 6, 0) for r in (0, 2, 3)})
    keys.update({(r, 0, 0): NONE for r in (1, 4, 5, 6, 7)})
    keys.update({(0, 1, 1): NONE, (2, 2, 2): NONE})
    # the float32 sum Z0 + m is Z1 for m = GAP and for the float32 below GAP (it rounds up); it is one float32 below Z1 for
    # m = sum_below, and one above Z1 for sum_above
    sum_below, sum_above = F(np.nextafter(Z1, F(0)) - Z0), F(np.nextafter(Z1, F(100)) - Z0)
    assert F(Z0 + sum_below) == np.nextafter(Z1, F(0)) and F(Z0 + np.nextafter(GAP, F(0))) == Z1
    return dict(gray=gray, mask=mask, bust=bust, flags=flags, keys=keys, cell=2, radius=1, keep=2, w=(0, 0, 0), star=(0, 1, 1),
                u=(1, 1, 0), margins=dict(zero=F(0), on=GAP, rounds_to_on=np.nextafter(GAP, F(0)), sum_below=sum_below,
                                          sum_above=sum_above))


# Wider neighbour tables for hand_scene_wide.  NB4: every A row names the other four A views, in an order chosen per row; the B
# rows are padded with -1 (before, between and behind the entries), and row 7 names view 5 twice.  NB7: every row names the other
# seven views, in an order of its own.
HAND_NB4 = np.array([[1, 2, 3, 4], [4, 0, 3, 2], [0, 1, 3, 4], [0, 1, 2, 4], [0, 1, 2, 3],
                     [6, 7, -1, -1], [-1, 5, -1, 7], [5, 5, 6, -1]], np.int32)
HAND_NB7 = np.array([[(r + s) % 8 for s in (3, 1, 7, 5, 2, 6, 4)] for r in range(8)], np.int32)


def hand_scene_wide():
    """cell 1, radius 1, for the tables of four and of seven columns.  Every voxel is a candidate; in each cell the layer-0
    voxel wins on the index, as both layers have the cell's cost.  Three pixels carry census codes:

    P = (row 1, col 5), the voxels (5, 1, .), seen by the A views alone.  Codes of the views 0..4: 0x00, 0x01, 0x07, 0x3F, 0xFF
    (0, 1, 3, 6 and 8 bits, each set of bits inside the next), so the distance of two views is the difference of their bit
    counts.  In the order of NB4 the four distances arrive
        view 0, [1, 2, 3, 4]: 1 3 6 8 (ascending)        view 1, [4, 0, 3, 2]: 7 1 5 2
        view 2, [0, 1, 3, 4]: 3 2 3 5 (two equal)        view 3, [0, 1, 2, 4]: 6 5 3 2 (descending)
        view 4, [0, 1, 2, 3]: 8 7 5 2 (descending)
    Q = (row 6, col 1), the voxels (1, 6, .): view 2 sees no hair there and view 4 has the code 0xFF, the rest 0.  Three of a
    row's four neighbours take part: exactly keep for keep = 3, one fewer than keep for keep = 4.
    M = (row 4, col 4), the voxels (4, 4, .), which all eight views see: view 0 has the code 0xFF, view 5 0x03, view 6 0x01, the
    rest 0.

    -> dict(gray, mask, bust, flags, keys4: {keep: {(view, row, col): key}} for NB4, keys7: the same for NB7, codes: {(view,
    row, col): census code})"""
    gray = np.full((V_HAND, 8, 8), 100, np.uint8)
    dark = {1: [(0, 4)], 2: [(0, 4), (0, 5), (0, 6)], 3: [(0, 4), (0, 5), (0, 6), (1, 4), (1, 6), (2, 4)]}      # bits 0.. of P
    for v, pixels in dark.items():
        for p in pixels:
            gray[(v,) + p] = 90
    gray[4, 1, 5] = gray[4, 6, 1] = gray[0, 4, 4] = 110
    gray[5, 3, 3] = gray[5, 3, 4] = gray[6, 3, 3] = 90          # bits 0 and 1 of M in view 5, bit 0 in view 6
    mask = np.ones((V_HAND, 8, 8), F)
    mask[2, 6, 1] = 0.0
    bust = np.full((V_HAND, 8, 8), 255.0, F)
    flags = np.ones((8, 8, 2), np.uint8)
    codes = {(0, 1, 5): 0x00, (1, 1, 5): 0x01, (2, 1, 5): 0x07, (3, 1, 5): 0x3F, (4, 1, 5): 0xFF,
             (4, 6, 1): 0xFF, (0, 6, 1): 0, (1, 6, 1): 0, (3, 6, 1): 0,
             (0, 4, 4): 0xFF, (5, 4, 4): 0x03, (6, 4, 4): 0x01, (1, 4, 4): 0, (2, 4, 4): 0, (3, 4, 4): 0, (4, 4, 4): 0,
             (7, 4, 4): 0}
    p, q, m = (5, 1, 0), (1, 6, 0), (4, 4, 0)
    # the key is 1024 * S // (8 * keep), S the sum of the keep smallest distances
    k4 = {
        1: {(0, 1, 5): key(128, *p), (4, 1, 5): key(256, *p), (2, 1, 5): key(256, *p),          # 1024 * 1 // 8, 1024 * 2 // 8
            (7, 4, 4): key(128, *m)},                                                             # 2 2 1 -> 1
        2: {(0, 1, 5): key(256, *p), (4, 1, 5): key(448, *p), (2, 1, 5): key(320, *p),          # 4, 7 and 5 of 16
            (5, 4, 4): key(192, *m),                                                              # view 5, [6, 7]: 1 2 -> 3 of 16
            (7, 4, 4): key(192, *m)},                                                             # 1 + 2
        3: {
            (0, 1, 5): key(426, *p),          # 1 + 3 + 6 = 10: 10240 // 24
            (1, 1, 5): key(341, *p),          # 1 + 2 + 5 = 8: 8192 // 24
            (2, 1, 5): key(341, *p),          # 2 + 3 + 3 = 8: the equal pair counts twice
            (3, 1, 5): key(426, *p),          # 2 + 3 + 5 = 10
            (4, 1, 5): key(597, *p),          # 2 + 5 + 7 = 14: 14336 // 24
            # Q: exactly keep neighbours take part.  Views 0, 1 and 3: 0 0 8 -> 8; view 4: 8 8 8 -> 24; view 2 sees no hair
            (0, 6, 1): key(341, *q), (1, 6, 1): key(341, *q), (3, 6, 1): key(341, *q), (4, 6, 1): key(1024, *q), (2, 6, 1): NONE,
            # M.  View 0 against four flat views: 8 8 8; view 1, [4, 0, 3, 2]: 0 8 0 0 -> 0
            (0, 4, 4): key(1024, *m), (1, 4, 4): key(0, *m),
            (5, 4, 4): NONE, (6, 4, 4): NONE,          # two neighbours take part: keep - 1
            # view 7, [5, 5, 6, -1]: view 5 counts twice, have = 3: 2 + 2 + 1 = 5: 5120 // 24
            (7, 4, 4): key(213, *m),
            (0, 0, 0): key(0, 0, 0, 0), (5, 0, 0): NONE,
        },
        4: {
            (0, 1, 5): key(576, *p),          # 18: 18432 // 32
            (1, 1, 5): key(480, *p),          # 1 + 2 + 5 + 7 = 15
            (2, 1, 5): key(416, *p),          # 2 + 3 + 3 + 5 = 13
            (3, 1, 5): key(512, *p),          # 16
            (4, 1, 5): key(704, *p),          # 22
            # Q: keep - 1 neighbours take part
            (0, 6, 1): NONE, (1, 6, 1): NONE, (2, 6, 1): NONE, (3, 6, 1): NONE, (4, 6, 1): NONE,
            (0, 4, 4): key(1024, *m), (1, 4, 4): key(256, *m),          # 0 0 0 8 -> 8192 // 32
            (5, 4, 4): NONE, (6, 4, 4): NONE, (7, 4, 4): NONE,          # view 7: have = 3
            (0, 0, 0): key(0, 0, 0, 0),
        },
    }
    k7 = {
        7: {
            # M, all seven neighbours take part.  View 5 (0x03): view 0: 6, views 1..4 and 7: 2 each, view 6: 1 -> 17: 17408 // 56
            (5, 4, 4): key(310, *m),
            # view 0 (0xFF): views 1..4 and 7: 8 each, view 5: 6, view 6: 7 -> 53: 54272 // 56
            (0, 4, 4): key(969, *m),
            # view 7 (0): 8 0 0 0 0 2 1 -> 11: 11264 // 56
            (7, 4, 4): key(201, *m),
            # P and a flat pixel: the four other A views take part, the B views do not
            (0, 1, 5): NONE, (4, 1, 5): NONE, (0, 0, 0): NONE,
        },
        4: {
            (0, 1, 5): key(576, *p), (4, 1, 5): key(704, *p), (2, 1, 5): key(416, *p),          # as under NB4: the same four
            (0, 6, 1): NONE,                                                                    # three take part
            (5, 4, 4): key(224, *m),          # the four smallest of 6 2 2 2 2 1 2: 1 + 2 + 2 + 2 = 7: 7168 // 32
        },
    }
    return dict(gray=gray, mask=mask, bust=bust, flags=flags, keys4=k4, keys7=k7, codes=codes, cell=1, radius=1)


def census_image():
    """a 5 x 7 image for cell 2 (Hc = 3, Wc = 4: neither a multiple) and the reduced image and radius-1 codes worked out by hand"""
    gray = np.array([[10, 11, 20, 20, 30, 31, 7],
                     [10, 12, 20, 21, 30, 30, 8],
                     [50, 50, 60, 61, 70, 70, 9],
                     [50, 51, 60, 60, 71, 70, 9],
                     [90, 91, 80, 81, 75, 76, 200]], np.uint8)[None]
    # block sums / n, rounded half up: 43/4 -> 11 (10.75); 81/4 -> 20 (20.25); 121/4 -> 30; 15/2 -> 8 (7.5 rounds up)
    reduced = np.array([[11, 20, 30, 8],
                        [50, 60, 70, 9],
                        [91, 81, 76, 200]], np.uint8)[None]
    # 201/4 = 50.25 -> 50; 241/4 = 60.25 -> 60; 281/4 = 70.25 -> 70; 18/2 = 9; 181/2 = 90.5 -> 91; 161/2 = 80.5 -> 81;
    # 151/2 = 75.5 -> 76; 200
    bits = {(-1, -1): 0, (-1, 0): 1, (-1, 1): 2, (0, -1): 3, (0, 1): 4, (1, -1): 5, (1, 0): 6, (1, 1): 7}

    def code(*offsets):
        return np.uint64(sum(1 << bits[o] for o in offsets))

    want = {
        (0, 0): code(),                                              # 11: the clamped window holds 11, 20, 50, 60 only
        # 8 at the upper right corner: nothing is smaller (the clamped copies of itself are equal, not smaller)
        (0, 3): code(),
        # 60 in the middle: smaller are 11 (-1,-1), 20 (-1,0), 30 (-1,1), 50 (0,-1)
        (1, 1): code((-1, -1), (-1, 0), (-1, 1), (0, -1)),
        # 91 at the lower left corner: (-1,-1) clamps to 50, (-1,0) = 50, (-1,1) = 60, (0,-1) clamps to itself, (0,1) = 81,
        # (1,-1) and (1,0) clamp to itself, (1,1) clamps to 81
        (2, 0): code((-1, -1), (-1, 0), (-1, 1), (0, 1), (1, 1)),
        # 200 at the lower right corner: (-1,-1) = 70, (-1,0) = 9, (-1,1) clamps to 9, (0,-1) = 76, (0,1) itself,
        # (1,-1) clamps to 76, (1,0) and (1,1) itself
        (2, 3): code((-1, -1), (-1, 0), (-1, 1), (0, -1), (1, -1)),
        # 30 on the upper border: (-1,.) clamp to row 0: 20, 30, 8; (0,-1) = 20, (0,1) = 8; row 1: 60, 70, 9
        (0, 2): code((-1, -1), (-1, 1), (0, -1), (0, 1), (1, 1)),
    }
    return gray, reduced, want


# ------------------------------------------------------------------------------------------------- 2. the textured sphere
SPHERE_V, SPHERE_HW, SPHERE_F, SPHERE_D = 12, 48, 10.0, 1.0
SPHERE_R = 0.085          # 10.9 voxels: five voxels are left for the spike
SPHERE_DIMS, SPHERE_VS = (32, 32, 32), 1.0 / 128.0
SPHERE_VMIN = tuple(-0.5 * (d - 1) * SPHERE_VS for d in SPHERE_DIMS)
SPHERE_CELL, SPHERE_RADIUS = 2, 2
# The texture's wavelengths lie around WL.  Views 30 degrees apart see a 5 x 5 window of 2-pixel cells (35 mm on a sphere of 85
# mm) quite differently: with wavelengths of 35 mm and a sphere of 62 mm the restatement confirmed 134 of 3 099 cells and removed
# nothing of the spike; the scene was made larger and smoother until the rule at its default bounds had something to confirm.
WL = 0.2


def sphere_cameras():
    cams = []
    for i in range(SPHERE_V):
        a = 2.0 * np.pi * i / SPHERE_V
        back = np.array([np.cos(a), 0.0, np.sin(a)])          # from the centre to the camera: the camera looks down -back
        up = np.array([0.0, 1.0, 0.0])
        right = np.cross(up, back)
        c2w = np.eye(4)
        c2w[:3, 0], c2w[:3, 1], c2w[:3, 2], c2w[:3, 3] = right, up, back, SPHERE_D * back
        cams.append(dict(file="ring_%02d" % i, pose=c2w.tolist(), ndc_prj=[SPHERE_F, SPHERE_F, 0.0, 0.0]))
    return cams


def _texture(seed):
    rng = np.random.default_rng([41, seed])
    k = rng.normal(size=(6, 3)) * (2.0 * np.pi / WL)
    phase, amp = rng.uniform(0, 2 * np.pi, 6), rng.uniform(0.5, 1.0, 6)

    def f(p):
        return (np.sin(p @ k.T + phase) * amp).sum(-1) / amp.sum()
    return f


def sphere_views(control=False):
    """-> (gray uint8 [V,H,W], mask float32 [V,H,W], z255 float32 [V,H,W]: the analytic depth on the scale of the depth planes,
    255 off the sphere).  Pixel (row, col) looks along the ray through ndc (1 - 2 col / W, 2 row / H - 1)."""
    H = W = SPHERE_HW
    gray, mask = np.zeros((SPHERE_V, H, W), np.uint8), np.zeros((SPHERE_V, H, W), F)
    z255 = np.full((SPHERE_V, H, W), 255.0, F)
    rows, cols = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    nx, ny = 1.0 - 2.0 * cols / W, 2.0 * rows / H - 1.0
    shared = _texture(0)
    for v, cam in enumerate(sphere_cameras()):
        c2w = np.array(cam["pose"])
        d_cam = -np.stack([nx / SPHERE_F, ny / SPHERE_F, np.ones_like(nx)], -1)          # z_camera = -1 along each ray
        d = d_cam @ c2w[:3, :3].T
        o = c2w[:3, 3]
        # |o + t d|^2 = R^2, the nearer root
        a, b, c = (d * d).sum(-1), 2.0 * (d @ o), o @ o - SPHERE_R ** 2
        disc = b * b - 4.0 * a * c
        hit = disc > 0.0
        t = np.where(hit, (-b - np.sqrt(np.where(hit, disc, 0.0))) / (2.0 * a), 0.0)      # depth along -z_camera
        p = o + t[..., None] * d
        tex = (_texture(100 + v) if control else shared)(p)
        gray[v] = np.where(hit, np.clip(np.rint(128.0 + 110.0 * tex), 1, 255), 0).astype(np.uint8)
        mask[v] = hit.astype(F)
        z255[v] = np.where(hit, t / 2.0 * 255.0, 255.0).astype(F)
    return gray, mask, z255


def sphere_neighbours(k=2):
    """the k nearest camera centres, ties by view index: the two ring neighbours for k = 2"""
    centres = np.array([np.array(c["pose"])[:3, 3] for c in sphere_cameras()])
    d = np.linalg.norm(centres[:, None] - centres[None], axis=2)
    out = np.zeros((SPHERE_V, k), np.int32)
    for r in range(SPHERE_V):
        order = sorted((round(d[r, n], 9), n) for n in range(SPHERE_V) if n != r)
        out[r] = [n for _, n in order[:k]]
    return out


def sphere_table(k, keep, seed=0):
    """sphere_neighbours(k) with the columns of every row in a seeded order of the row's own, so that the distances do not
    arrive nearest view first; row 3 is padded with -1 down to `keep` entries and row 8 down to keep - 1"""
    rng = np.random.default_rng([43, k, keep, seed])
    nb = sphere_neighbours(k)
    nb = np.stack([row[rng.permutation(k)] for row in nb]).astype(np.int32)
    for row, valid in ((3, keep), (8, keep - 1)):
        gone = rng.permutation(k)[:k - valid]
        nb[row, gone] = -1
    return nb


INSIDE_VIEW = SPHERE_V          # the index of the view of inside_cameras that sits inside the grid


def inside_cameras():
    """the twelve ring cameras and a thirteenth inside the grid: the pose of ring view 0 (it looks down -x) with its centre at
    x = SPHERE_VS / 2, which is the plane of the voxel centres x = 16 (world x = (16 - 15.5) / 128): those 32 x 32 centres have
    z' = 0 exactly, the 15 layers x = 17..31 lie behind the view, the 16 layers x = 0..15 in front of it.  Its focal length of 2
    is short enough for the pixels of many voxels behind it to fall inside the image."""
    cams = sphere_cameras()
    c2w = np.array(cams[0]["pose"])
    c2w[:3, 3] = (0.5 * SPHERE_VS, 0.0, 0.0)
    cams.append(dict(file="inside_00", pose=c2w.tolist(), ndc_prj=[2.0, 2.0, 0.0, 0.0]))
    return cams


def inside_views():
    """-> (gray, mask) of sphere_views() with the thirteenth view's planes behind them: a flat gray image, hair everywhere"""
    gray, mask, _ = sphere_views()
    H = W = SPHERE_HW
    return (np.concatenate([gray, np.full((1, H, W), 128, np.uint8)]), np.concatenate([mask, np.ones((1, H, W), F)]))


def inside_table():
    """int32 [13,3]: the three nearest ring views of each ring view, with view 12 in place of the third in the rows of the views 0
    and 6; view 12 itself has the neighbours 0, 6 and 3"""
    nb = np.concatenate([sphere_neighbours(3), np.array([[0, 6, 3]], np.int32)])
    nb[0, 2] = nb[6, 2] = INSIDE_VIEW
    return nb


def sphere_world():
    """float64 [X,Y,Z,3]: the voxel centres"""
    x, y, z = np.meshgrid(*(np.arange(d) for d in SPHERE_DIMS), indexing="ij")
    m = SPHERE_VMIN
    return np.stack([m[0] + x * SPHERE_VS, -(m[1] + y * SPHERE_VS), -(m[2] + z * SPHERE_VS)], -1)


def spike_voxels():
    """bool [X,Y,Z]: a column one voxel thick from the sphere's surface towards camera 0 (which sits on +x), to the grid's end"""
    w = sphere_world()
    r = np.linalg.norm(w, axis=-1)
    out = np.zeros(SPHERE_DIMS, bool)
    out[:, SPHERE_DIMS[1] // 2, SPHERE_DIMS[2] // 2] = True
    return out & (r > SPHERE_R) & (w[..., 0] > 0)
