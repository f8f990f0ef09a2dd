"""CPU: the C statements of both rasterisers (oracle/raster_oracle.c) against an exact-rational reference written from the
specification alone (tests/raster_exact.py: fractions.Fraction, the top-left rule as an infinitesimal shift of the sample,
OpenGL 4.6 14.5.1's diamond-exit rule as an exact clip of the shifted segment against every diamond of its bounding box).

Where tests/test_raster_gpu.py compares the kernel with a C restatement written the same way, this pins the tie rules
themselves: centres exactly on edges and shared vertices, end points on diamond corners and edges, crossings half-way
between two pixels, |dx| == |dy|, segments inside one diamond, wide-line offset and replication, clipping at the borders.
The cases (tests/raster_exact_cases.py) land exactly where intended -- a precondition asserted for every vertex -- and the
reference counts the ties it met; every family of cases must meet some.  Run with -s for the counts and the running time."""
import time
from fractions import Fraction

import numpy as np
import pytest

import oracle
import raster_exact as exact
from raster_exact_cases import (CONFIGS, SIZES, camera_record, disjoint_groups, place, segment_families, tessellation,
                                triangle_families, vertices)

RUNS = [SIZES[0] + c for c in CONFIGS] + [SIZES[1] + CONFIGS[0]]
NONE_V, NONE_F = np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32)
REF_SECONDS = {}


def _timed(key, fn, *a):
    t0 = time.perf_counter()
    out = fn(*a)
    REF_SECONDS[key] = REF_SECONDS.get(key, 0.0) + time.perf_counter() - t0
    return out


def _pixels(mask):
    return set(zip(*(x.tolist() for x in np.nonzero(mask))))


def _tri_prim(rec, tris_abs, H, W, pc, bits):
    v = vertices([p for t in tris_abs for p in t], H, W, bits)
    f = np.arange(3 * len(tris_abs), dtype=np.int32).reshape(-1, 3)
    prim = oracle.render_strands(rec, v, f, NONE_V, NONE_V, H, W, pc, 1, -1, 2, 0.0)[1]
    depth, covered = oracle.render_depth(rec, v, f, H, W, pc)
    assert np.array_equal(depth < 255, prim >= 0) and covered == (prim >= 0).sum()      # the two statements agree
    return prim


def _seg_prim(rec, segs_abs, H, W, pc, bits, width, rule):
    p = vertices([q for s in segs_abs for q in s], H, W, bits)
    t = np.repeat(p[1::2] - p[0::2], 2, axis=0)
    return oracle.render_strands(rec, NONE_V, NONE_F, p, t, H, W, pc, width, 3, 1, 0.0, line_rule=rule)[1]


@pytest.mark.parametrize("H,W,pc,bits", RUNS)
def test_triangles_equal_the_exact_reference(H, W, pc, bits):
    rec, before = camera_record(), REF_SECONDS.get("triangles", 0.0)
    oracle.set_subpixel_bits(bits)
    try:
        report = {}
        for name, tris in triangle_families(H, W).items():
            placed = [place(t, pc, bits) for t in tris]
            ref = [_timed("triangles", exact.triangle, t, H, W, pc) for t in placed]
            sets, ties = [r[0] for r in ref], sum(r[1] for r in ref)
            report[name] = (len(tris), sum(len(s) for s in sets), ties)
            assert ties > 0, "%s: no pixel centre lies exactly on an edge or a vertex" % name
            for k, (t, want) in enumerate(zip(placed, sets)):
                assert _pixels(_tri_prim(rec, [t], H, W, pc, bits) == 0) == want, (name, k, t)
                back = t[::-1]                                               # the other winding: same pixels
                assert _timed("triangles", exact.triangle, back, H, W, pc)[0] == want, (name, k)
                assert _pixels(_tri_prim(rec, [back], H, W, pc, bits) == 0) == want, (name, k, back)
            for group in disjoint_groups(sets):                              # together, where no pixel is claimed twice
                prim = _tri_prim(rec, [placed[i] for i in group], H, W, pc, bits)
                for n, i in enumerate(group):
                    assert _pixels(prim == n) == sets[i], (name, i)
                assert (prim >= 0).sum() == sum(len(sets[i]) for i in group)
            # an identical triangle drawn twice: the first index owns every pixel
            k = max(range(len(sets)), key=lambda i: len(sets[i]))
            twice = _tri_prim(rec, [placed[k], placed[k]], H, W, pc, bits)
            assert _pixels(twice == 0) == sets[k] and not (twice == 1).any(), name
            if name == "fan around a vertex on a pixel centre":              # the shared centre vertex has exactly one owner
                assert sum(len(s) for s in sets) == len(set().union(*sets))
                assert len([i for i, s in enumerate(sets[:8]) if (10, 10) in s]) == 1
                assert len([i for i, s in enumerate(sets[8:]) if (16, 40) in s]) == 1
            if name == "slivers without a centre":
                assert not any(sets)
            if name == "tessellated rectangle":                              # union == the rectangle, no pixel owned twice
                (x0, y0, x1, y1), _ = tessellation(H, W)
                (x0, y0), (x1, y1) = place([(x0, y0), (x1, y1)], pc, bits)
                p = Fraction(pc)
                inside = {(r, c) for r in range(H) for c in range(W)
                          if Fraction(x0, 256) <= c + p < Fraction(x1, 256) and Fraction(y0, 256) <= r + p < Fraction(y1, 256)}
                assert set().union(*sets) == inside and sum(len(s) for s in sets) == len(inside)
                all_prim = _tri_prim(rec, placed, H, W, pc, bits)
                assert _pixels(all_prim >= 0) == inside and all(_pixels(all_prim == i) == s for i, s in enumerate(sets))
            if name == "boxes of 24 and 25 pixels":                          # the one-lane / one-wave switch of the kernel
                boxes = set()
                for t in placed:
                    off = int(pc * 256)
                    cs = [-((off - min(x for x, _ in t)) // 256), (max(x for x, _ in t) - off) // 256]
                    rs = [-((off - min(y for _, y in t)) // 256), (max(y for _, y in t) - off) // 256]
                    boxes.add((min(cs[1], W - 1) - max(cs[0], 0) + 1) * (min(rs[1], H - 1) - max(rs[0], 0) + 1))
                assert {24, 25} <= boxes, boxes
        print("\ntriangles H %d W %d pixel_center %.1f bits %d: family: primitives, pixels, centres on an edge or vertex" %
              (H, W, pc, bits))
        for name, row in report.items():
            print("  %-50s %4d %6d %5d" % ((name,) + row))
        print("  exact reference: %.2f s" % (REF_SECONDS.get("triangles", 0.0) - before))
    finally:
        oracle.set_subpixel_bits(8)


@pytest.mark.parametrize("H,W,pc,bits", RUNS)
def test_segments_equal_the_exact_reference(H, W, pc, bits):
    rec, before = camera_record(), REF_SECONDS.get("segments", 0.0)
    oracle.set_subpixel_bits(bits)
    try:
        report = {}
        for name, segs in segment_families(H, W).items():
            placed = [place(s, pc, bits) for s in segs]
            tie_e = tie_h = 0
            for width, rule in ((1, 0), (2, 0), (3, 0), (1, 1)):
                ref = [_timed("segments", exact.line, s[0], s[1], width, H, W, pc, rule) for s in placed]
                sets = [set(r) for r in ref]
                if (width, rule) == (1, 0):
                    ties = [_timed("segments", exact.line_ties, s[0], s[1], H, W, pc) for s in placed]
                    tie_e, tie_h = sum(t["endpoint"] for t in ties), sum(t["halfway"] for t in ties)
                    report[name] = (len(segs), sum(len(s) for s in sets), tie_e, tie_h)
                for k, (s, want) in enumerate(zip(placed, sets)):
                    got = _pixels(_seg_prim(rec, [s], H, W, pc, bits, width, rule) == 0)
                    assert got == want, (name, k, s, width, rule, sorted(got - want), sorted(want - got))
                for group in disjoint_groups(sets):
                    prim = _seg_prim(rec, [placed[i] for i in group], H, W, pc, bits, width, rule)
                    for n, i in enumerate(group):
                        assert _pixels(prim == n) == sets[i], (name, i, width, rule)
                    assert (prim >= 0).sum() == sum(len(sets[i]) for i in group)
                if name == "polyline with shared end points" and rule == 0 and width == 1:
                    # the point of the diamond-exit rule: no pixel is produced by two consecutive segments of a chain, in the
                    # reference and in the statement; what the chain leaves out is what the reference leaves out (above)
                    for i in range(len(sets) - 1):
                        assert not (sets[i] & sets[i + 1]), i
                        a = _pixels(_seg_prim(rec, [placed[i]], H, W, pc, bits, 1, 0) == 0)
                        b = _pixels(_seg_prim(rec, [placed[i + 1]], H, W, pc, bits, 1, 0) == 0)
                        assert not (a & b), i
            # (a segment inside one closed diamond can reach a half-way point, a corner of the diamond, only with an end point)
            assert tie_e > 0 and (tie_h > 0 or name == "inside one diamond"), "%s: end points on a diamond boundary %d, half-way crossings %d" % (name, tie_e, tie_h)
        print("\nsegments H %d W %d pixel_center %.1f bits %d: family: primitives, pixels (width 1), end points on a diamond "
              "boundary, half-way crossings" % (H, W, pc, bits))
        for name, row in report.items():
            print("  %-55s %4d %6d %5d %5d" % ((name,) + row))
        print("  exact reference: %.2f s" % (REF_SECONDS.get("segments", 0.0) - before))
    finally:
        oracle.set_subpixel_bits(8)


def interpolation_cases(H, W):
    """segments of 5 to 20 pixels in every octant, their ends off the centres so that t leaves [0, 1] at the first fragment"""
    from raster_exact_cases import DIRS, P

    segs = []
    for k, (dx, dy) in enumerate(DIRS):
        s = (90, -30) if k % 2 else (-60, 50)
        segs.append((P(30, 15, *s), P(30 + dx * (1 + k % 3), 15 + dy * (1 + k % 3), 50, 30)))
    return segs


def check_interpolation(draw, H, W, pc, bits):
    """draw(points_abs, depths, width) -> rgb [H,W,3] of one segment in colour option 0 on clear colour 1.

    The colour of a fragment is depth/2 with depth perspective-correct in t: 1 / ((1 - t)/d_a + t/d_b), d_a = 1, d_b = 1.25,
    t the reference's exact Fraction.  Bound: the rasterisers evaluate t as a quotient of two integers converted to float32
    (two conversions and a division: 3 roundings), then (1-t) w_a, t w_b, their sum, two products with the end-point depths,
    their sum and the quotient, and the halving is exact (about 8 roundings, all on quantities of the size of the result
    because t, 1 - t >= -0.1 and the depths are within 25 % of each other): some 11 half-ulps of float32 = 11 * 6e-8 < 7e-7
    relative.  1e-5 relative is more than tenfold that sum.  A t taken one pixel off, clamped to [0, 1] or used without the
    perspective division moves the value by more than 1e-3 relative on these segments (at most 20 pixels for a quarter of
    the depth; first fragments with t < -0.01)."""
    worst, n, outside = 0.0, 0, 0
    for seg in interpolation_cases(H, W):
        s = place(seg, pc, bits)
        for width in (1, 3):
            frags = exact.line(s[0], s[1], width, H, W, pc, 0)
            rgb = draw(s, (1.0, 1.25), width)
            assert _pixels(rgb[..., 0] != 1.0) == set(frags)
            for (r, c), t in frags.items():
                t = float(t)
                want = 0.5 / ((1.0 - t) / 1.0 + t / 1.25)
                rel = abs(float(rgb[r, c, 0]) - want) / want
                print("interpolation t %+.6f want %.8f got %.8f rel %.2e" % (t, want, rgb[r, c, 0], rel))
                worst, n, outside = max(worst, rel), n + 1, outside + (t < -0.01 or t > 1.01)
                assert rel <= 1e-5, (seg, width, r, c, t, want, float(rgb[r, c, 0]))
                assert rgb[r, c, 0] == rgb[r, c, 1] == rgb[r, c, 2]
    assert n > 300 and outside >= 8, (n, outside)
    return worst


@pytest.mark.parametrize("pc,bits", [(0.5, 8), (0.0, 4)])
def test_interpolation_at_the_exact_t(pc, bits):
    H, W = SIZES[0]
    rec = camera_record()

    def draw(seg_abs, depths, width):
        p = vertices(seg_abs, H, W, bits, depth=depths)
        t = np.repeat(p[1::2] - p[0::2], 2, axis=0)
        return oracle.render_strands(rec, NONE_V, NONE_F, p, t, H, W, pc, width, 0, 1, 1.0)[0]

    oracle.set_subpixel_bits(bits)
    try:
        print("worst relative error %.2e" % check_interpolation(draw, H, W, pc, bits))
    finally:
        oracle.set_subpixel_bits(8)
