"""Exact-rational reference of the two rasterisers' coverage rules (helper module: no tests, no markers).

Plain Python on fractions.Fraction, written from the written specification -- the header comments of
monohair_amd/csrc/raster.hip and OpenGL 4.6 (core) 14.5.1 (basic line segment rasterisation), 14.5.2.2 (wide lines) and
14.6.1 (basic polygon rasterisation) -- and not from the integer code of the kernel or of oracle/raster_oracle.c: no
per-column walk, no nearest-row rounding, no case analysis of ties.  Every tie is decided by the specification's own
device, an infinitesimal shift, carried out in exact arithmetic.

Coordinates: window positions already on the sub-pixel grid, as integers in 1/256 pixel, (column to the right, row
downwards).  The centre of pixel (r, c) is (c + pc, r + pc) pixel, pc = the "pixel_center" of the renderers (0.5 = OpenGL).
OpenGL's window y grows upwards and the images here are flipped to a top-left origin, so a shift of (-e, -e^2) in GL window
coordinates is (-e in column, +e^2 in row) here.

  * triangle (14.6.1: a fragment iff its centre is inside; a centre on an edge is left to a rule that draws a shared edge
    once -- raster.hip: "top-left fill rule"): pixel (r, c) is covered iff the point (c + pc + e, r + pc + e^2) is strictly
    inside.  A centre on a left or a top edge is in, on a right or a bottom edge out, a shared vertex has one owner; the
    winding does not matter; zero area draws nothing.
  * thin line (14.5.1, the diamond-exit rule, literally): with p_a, p_b shifted by (-e, -e^2) in window coordinates, a
    fragment for pixel f iff the segment meets the open diamond R_f = { |dx| + |dy| < 1/2 } around f's centre and R_f
    does not contain the shifted p_b.  rule 1 (raster.hip "line_rule" 1): without that exception.  The intersection is an
    exact parametric clip of the segment against the four half-planes of R_f, evaluated for every pixel of the segment's
    bounding box +- 1.
  * wide line (14.5.2.2, as the comment of mh_setup_seg states it): x-major iff |dx| >= |dy|; the minor coordinate is
    offset by (width - 1)/2 towards smaller window coordinates (x-major: larger rows; y-major: smaller columns), the
    offset segment is rasterised thin, and every fragment is replicated `width` times towards larger window coordinates
    (x-major: rows r-(width-1) .. r; y-major: columns c .. c+width-1); the result is clipped to the image.
  * t of a fragment (14.5.1): (p_r - p_a).(p_b - p_a) / |p_b - p_a|^2 with p_r the centre of the (thin) fragment and the
    unshifted end points -- the foot of the perpendicular, not clamped.

e = 2^-40: coordinates live on a 2^-8 grid inside +-2^10 pixel, so every quantity compared below is either exactly tied or
apart by more than 2^-30, terms in e are at least 2^-48 where they do not vanish and terms in e^2 at most 2^-69: the shift
decides ties, and only ties, in the lexicographic order the specification intends.

Arithmetic: exact, in units of 1/256 pixel, so that positions, centres and half a pixel (128) are whole numbers -- kept as
Python integers -- and only the shift, the clip parameters and t are Fractions.  Edge functions and half-plane functions
are affine, so their value at a shifted point is their value at the unshifted one plus a constant: the shift is folded into
constants computed once per primitive -- the same numbers, fewer big fractions.

The functions also COUNT the ties they met (what the suite reports and requires to be non-zero): a pixel centre exactly on
an edge or vertex of a triangle; an end point of a segment exactly on a diamond's boundary; a segment crossing a column's
(x-major) or a row's (y-major) sample line exactly half-way between two pixel centres.
"""
from fractions import Fraction
from functools import lru_cache

SUB = 256                          # units per pixel
E = SUB * Fraction(1, 2 ** 40)     # the specification's infinitesimal e (pixel), in units
E2 = SUB * Fraction(1, 2 ** 80)    # e^2 (pixel), in units
HALF = SUB // 2


def _pt(p):
    return int(p[0]), int(p[1])


def _off(pixel_center):
    off = Fraction(pixel_center) * SUB
    assert off.denominator == 1
    return int(off)


def _span(lo, hi, off, pad, first, last):
    """pixel indices i whose centre i * 256 + off lies in [lo, hi], `pad` more on either side, within first .. last"""
    return range(max((lo - off) // SUB - pad, first), min(-((off - hi) // SUB) + pad, last) + 1)


def triangle(tri, H, W, pixel_center=0.5):
    """tri: three (col, row) in 1/256 pixel -> (set of covered (r, c), number of pixel centres exactly on its boundary)"""
    off = _off(pixel_center)
    a, b, c = (_pt(p) for p in tri)
    area = (b[0] - a[0]) * (c[1] - a[1]) - (b[1] - a[1]) * (c[0] - a[0])
    if area == 0:
        return set(), 0
    sign = 1 if area > 0 else -1
    # edge function of s -> t at q, positive inside: dx (q_row - s_row) - dy (q_col - s_col); at the shifted sample it is its
    # value at the centre plus the constant dx e^2 - dy e
    edges = [(s, (t[0] - s[0]) * sign, (t[1] - s[1]) * sign) for s, t in ((a, b), (b, c), (c, a))]
    edges = [(s, dx, dy, dx * E2 - dy * E) for s, dx, dy in edges]
    xs, ys = (a[0], b[0], c[0]), (a[1], b[1], c[1])
    covered, ties = set(), 0
    for r in _span(min(ys), max(ys), off, 1, 0, H - 1):
        for col in _span(min(xs), max(xs), off, 1, 0, W - 1):
            at = [dx * (r * SUB + off - s[1]) - dy * (col * SUB + off - s[0]) for s, dx, dy, _ in edges]     # the centre itself
            if min(at) >= 0 and 0 in at:
                ties += 1
            if all(v + e[3] > 0 for v, e in zip(at, edges)):
                covered.add((r, col))
    return covered, ties


_DIAMOND = ((1, 1), (1, -1), (-1, 1), (-1, -1))       # the four half-planes n . (p - centre) < 1/2 pixel of a diamond


def _box(pa, pb, off, clip):
    """the pixels of the segment's bounding box +- 1, cut to clip = (r_lo, r_hi, c_lo, c_hi) (only to bound the work)"""
    rs = _span(min(pa[1], pb[1]), max(pa[1], pb[1]), off, 1, clip[0], clip[1])
    cs = _span(min(pa[0], pb[0]), max(pa[0], pb[0]), off, 1, clip[2], clip[3])
    return [(r, c) for r in rs for c in cs]


@lru_cache(maxsize=None)
def _thin(pa, pb, off, clip):
    """-> ({(r, c): t} of every pixel whose open diamond the shifted segment meets, the pixels whose diamond holds the
    shifted p_b).  The segment is { p_a' + t d, 0 < t < 1 } with p_a' = p_a + (-e, +e^2); half-plane n of the diamond around
    `centre` reads n.(p_a - centre) + t n.d < 1/2 - n.(-e, e^2): the left side is evaluated for the unshifted end points
    (whole numbers), the shift sits in the four constants on the right."""
    d = (pb[0] - pa[0], pb[1] - pa[1])
    len2 = d[0] * d[0] + d[1] * d[1]
    frags, last = {}, set()
    if len2 == 0:
        return frags, last
    planes = [(nx, ny, nx * d[0] + ny * d[1], HALF - (-nx * E + ny * E2)) for nx, ny in _DIAMOND]
    for r, c in _box(pa, pb, off, clip):
        ax, ay = pa[0] - (c * SUB + off), pa[1] - (r * SUB + off)
        t0, t1 = Fraction(0), Fraction(1)     # exact clip of the parameter interval (0, 1) against the four open half-planes
        for nx, ny, slope, bound in planes:
            at = nx * ax + ny * ay
            if slope == 0:
                if not at < bound:
                    break
            elif slope > 0:
                if not at < bound:            # outside at t = 0 and moving further out
                    break
                t1 = min(t1, (bound - at) / slope)
            else:
                if not at + slope < bound:    # still outside at t = 1
                    break
                t0 = max(t0, (bound - at) / slope)
            if not t0 < t1:
                break
        else:
            frags[(r, c)] = Fraction(-(ax * d[0] + ay * d[1]), len2)
            if all(nx * (ax + d[0]) + ny * (ay + d[1]) < bound for nx, ny, _, bound in planes):
                last.add((r, c))
    return frags, last


def thin_line(pa, pb, pixel_center=0.5, rule=0, clip=(-4, 1 << 12, -4, 1 << 12)):
    """pa, pb: (col, row) as integers in 1/256 pixel -> {(r, c): t}.  clip = (r_lo, r_hi, c_lo, c_hi) bounds the pixels
    examined (inclusive); fragments are not clipped otherwise."""
    frags, last = _thin(_pt(pa), _pt(pb), _off(pixel_center), clip)
    return {k: t for k, t in frags.items() if rule != 0 or k not in last}


def _offset(a, b, width):
    pa, pb = _pt(a), _pt(b)
    xmajor = abs(pb[0] - pa[0]) >= abs(pb[1] - pa[1])
    shift = (width - 1) * HALF
    if xmajor:
        return xmajor, (pa[0], pa[1] + shift), (pb[0], pb[1] + shift)
    return xmajor, (pa[0] - shift, pa[1]), (pb[0] - shift, pb[1])


def line(a, b, width, H, W, pixel_center=0.5, rule=0):
    """a, b: (col, row) in 1/256 pixel -> {(r, c) inside the image: t of its thin fragment}"""
    xmajor, pa, pb = _offset(a, b, width)
    thin = thin_line(pa, pb, pixel_center, rule, clip=(-width - 1, H + width, -width - 1, W + width))
    out = {}
    for (r, c), t in sorted(thin.items()):
        for k in range(width):
            rr, cc = (r - k, c) if xmajor else (r, c + k)
            if 0 <= rr < H and 0 <= cc < W:
                assert (rr, cc) not in out, "two thin fragments replicate onto one pixel"
                out[(rr, cc)] = t
    return out


def line_ties(a, b, H, W, pixel_center=0.5):
    """the ties of a thin segment among the pixels line() examines -> dict(endpoint=, halfway=): (end point, pixel) pairs
    with the end point exactly on the pixel's diamond boundary; crossings of a sample line (the column's if x-major, else the
    row's), strictly between the end points, exactly half-way between two pixel centres"""
    off = _off(pixel_center)
    xmajor, pa, pb = _offset(a, b, 1)
    d = (pb[0] - pa[0], pb[1] - pa[1])
    len2 = d[0] * d[0] + d[1] * d[1]
    ties = dict(endpoint=0, halfway=0)
    if len2 == 0:
        return ties
    for r, c in _box(pa, pb, off, (-2, H + 1, -2, W + 1)):
        ax, ay = pa[0] - (c * SUB + off), pa[1] - (r * SUB + off)
        ties["endpoint"] += (abs(ax) + abs(ay) == HALF) + (abs(ax + d[0]) + abs(ay + d[1]) == HALF)
        hx, hy = (-ax, HALF - ay) if xmajor else (HALF - ax, -ay)      # from p_a to the point half-way to the next pixel
        ties["halfway"] += d[0] * hy == d[1] * hx and 0 < hx * d[0] + hy * d[1] < len2
    return ties
