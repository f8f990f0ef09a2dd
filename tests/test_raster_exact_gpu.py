"""GPU: mh_render_depth and mh_render_strands (csrc/raster.hip) on the tie cases of tests/raster_exact_cases.py: every image
bit-equal to the C statement's (oracle/raster_oracle.c) and, independently of that statement, `image != clear` equal to the
coverage of the exact-rational reference (tests/raster_exact.py) -- primitives alone, together where their pixel sets are
disjoint, both windings, widths 1 to 3, both line rules, pixel_center 0.5 and 0.0, 8 and 4 sub-pixel bits; triangles whose
clamped boxes have 24 and 25 pixels go through the one-lane and the one-wave pass (MH_R_SMALL)."""
import numpy as np
import pytest
import torch

import oracle
import raster_exact as exact
from raster_exact_cases import camera_record, disjoint_groups, place, segment_families, triangle_families, vertices
from test_raster_exact_host import NONE_F, NONE_V, RUNS, _pixels, check_interpolation

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _set_bits(bits):
    from monohair_amd import _lib
    from monohair_amd.pmvo_utils import _ctx_for

    _lib.check(_lib.lib().mh_ctx_set_option(_ctx_for(torch.device(DEV)), b"raster_subpixel_bits", bits))
    oracle.set_subpixel_bits(bits)


class _Lines:
    """one StrandRenderer without a mesh whose segment buffers are swapped per case"""

    def __init__(self):
        from monohair_amd.render import StrandRenderer

        self.r = StrandRenderer([], NONE_V, NONE_F, DEV)

    def draw(self, rec, p, H, W, pc, width, rule, colour, clear):
        t = np.repeat(p[1::2] - p[0::2], 2, axis=0)
        self.r.line_pts, self.r.line_tan = torch.from_numpy(p).to(DEV), torch.from_numpy(t).to(DEV)
        self.r.nseg = len(p) // 2
        got = self.r.render(rec, H, W, colour, 1, clear, pixel_center=pc, line_width=width, line_rule=rule).cpu().numpy()
        want = oracle.render_strands(rec, NONE_V, NONE_F, p, t, H, W, pc, width, colour, 1, clear, line_rule=rule)[0]
        assert np.array_equal(got, want)                       # bit for bit the C statement's image
        return got


@pytest.mark.parametrize("H,W,pc,bits", RUNS)
def test_hip_triangles_equal_the_statement_and_the_exact_reference(H, W, pc, bits):
    from monohair_amd.render import DepthRenderer, StrandRenderer

    rec = camera_record()

    def check(tris_abs, want_pixels):
        v = vertices([p for t in tris_abs for p in t], H, W, bits)
        f = np.arange(3 * len(tris_abs), dtype=np.int32).reshape(-1, 3)
        got = DepthRenderer([(v, f)], DEV).render(rec, H, W, pc).cpu().numpy()
        assert np.array_equal(got, oracle.render_depth(rec, v, f, H, W, pc)[0])
        assert _pixels(got != 255.0) == want_pixels
        rgb = StrandRenderer([], v, f, DEV).render(rec, H, W, 3, 0, 1.0, draw_strands=False, pixel_center=pc).cpu().numpy()
        assert np.array_equal(rgb, oracle.render_strands(rec, v, f, NONE_V, NONE_V, H, W, pc, 3, -1, 0, 1.0)[0])
        assert _pixels(rgb[..., 0] != 1.0) == want_pixels
        return got

    _set_bits(bits)
    try:
        for name, tris in triangle_families(H, W).items():
            placed = [place(t, pc, bits) for t in tris]
            sets = [exact.triangle(t, H, W, pc)[0] for t in placed]
            for t, want in zip(placed, sets):
                alone = check([t], want)
                check([t[::-1]], want)
                assert np.array_equal(check([t, t], want), alone)          # drawn twice: the same image as alone
            for group in disjoint_groups(sets):
                check([placed[i] for i in group], set().union(*(sets[i] for i in group)))
    finally:
        _set_bits(8)


@pytest.mark.parametrize("H,W,pc,bits", RUNS)
def test_hip_segments_equal_the_statement_and_the_exact_reference(H, W, pc, bits):
    rec, lines = camera_record(), _Lines()
    _set_bits(bits)
    try:
        for name, segs in segment_families(H, W).items():
            placed = [place(s, pc, bits) for s in segs]
            for width, rule in ((1, 0), (2, 0), (3, 0), (1, 1)):
                sets = [set(exact.line(s[0], s[1], width, H, W, pc, rule)) for s in placed]
                for k, (s, want) in enumerate(zip(placed, sets)):
                    img = lines.draw(rec, vertices(s, H, W, bits), H, W, pc, width, rule, 3, 0.0)
                    assert _pixels(img[..., 0] != 0.0) == want, (name, k, s, width, rule)
                for group in disjoint_groups(sets):
                    p = vertices([q for i in group for q in placed[i]], H, W, bits)
                    img = lines.draw(rec, p, H, W, pc, width, rule, 3, 0.0)
                    assert _pixels(img[..., 0] != 0.0) == set().union(*(sets[i] for i in group)), (name, width, rule)
    finally:
        _set_bits(8)


@pytest.mark.parametrize("pc,bits", [(0.5, 8), (0.0, 4)])
def test_hip_interpolation_at_the_exact_t(pc, bits):
    """check_interpolation of tests/test_raster_exact_host.py (the derivation of the 1e-5 bound is there) on the HIP image"""
    H, W = RUNS[0][:2]
    rec, lines = camera_record(), _Lines()
    _set_bits(bits)
    try:
        worst = check_interpolation(lambda s, depths, width: lines.draw(rec, vertices(s, H, W, bits, depth=depths), H, W, pc,
                                                                        width, 0, 0, 1.0), H, W, pc, bits)
        print("worst relative error %.2e" % worst)
    finally:
        _set_bits(8)
