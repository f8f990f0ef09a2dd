"""Helper (not a test): the guarded C-ABI calls of the photo-consistent carve, entered into the ledger of tests/guard_cases.py
when this module is imported, the way tests/hair_carve_guard_cases.py enters the silhouette carve.
tests/test_hair_stereo_guard_gpu.py imports this module and runs the cases on the arena of tests/guard_arena.py; pytest imports
every test module before it runs any test, so a run of the suite finds the four entry points in the ledger.  (A run of
tests/test_guard_host.py ALONE does not import this file: name tests/test_hair_stereo_guard_gpu.py beside it.)"""
import numpy as np

import guard_cases as G
from guard_cases import B, CTX, STREAM, Call, F_GRIDS, In, Out, case, f64, i32

ENTRIES = ("mh_stereo_census", "mh_stereo_winners", "mh_stereo_agree", "mh_stereo_refine")
VMIN, VS = (-0.06, -0.1, -0.1), 0.03
CELL, RADIUS, KEEP, MAX_COST, M255, MIN_AGREE, MIN_THROUGH = 4, 1, 1, 640, np.float32(3.0), 2, 1
_cache = {}


def _scene(dims):
    """the PMVO scene of the guard cases (22 views of 32 x 64), a bust plane in half of its pixels, seeded photographs, a ring
    of neighbours (one row padded), seeded candidate flags -> everything the restatement makes of them"""
    import hair_stereo_np as R

    if dims not in _cache:
        p = G._pm(False, 3)
        rng = np.random.default_rng([7] + list(dims))
        V, H, W = p.views.mask.shape
        bust = p.views.depth.copy()
        bust[rng.random(bust.shape) < 0.5] = 255
        gray = np.repeat(np.repeat(rng.integers(0, 256, (V, H // 4, W // 4), dtype=np.uint8), 4, 1), 4, 2)
        gray[:, ::3, ::5] += 9
        nb = np.stack([(np.arange(V) + 1) % V, (np.arange(V) - 1) % V], 1).astype(np.int32)
        nb[5, 1] = -1
        flags = (rng.random(dims) < 0.7).astype(np.uint8)
        want = R.stereo(p.views.cams, gray, p.views.mask, bust, f64(VMIN), VS, dims, flags, nb, CELL, RADIUS, KEEP, MAX_COST,
                        M255, MIN_AGREE, MIN_THROUGH)
        assert (want["keys"] != R.NONE).any() and want["agree"].max() >= MIN_AGREE and (want["depth"] != 255).any()
        _cache[dims] = (p, bust, gray, nb, flags, want)
    return _cache[dims]


@case("F", "mh_stereo_census", "32x64-cell3")
def _():
    import hair_stereo_np as R

    gray = np.random.default_rng(11).integers(0, 256, (5, 32, 64), dtype=np.uint8)
    g = R.reduce_gray(gray, 3)
    return Call("mh_stereo_census", [CTX, B("gray", In(gray)), 5, 32, 64, 3, 2, B("reduced", Out(g.shape, np.uint8)),
                                     B("census", Out(g.shape, np.uint64)), STREAM], {"reduced": g, "census": R.census(g, 2)})


for _dims in F_GRIDS:
    _id = "%dx%dx%d" % _dims

    @case("F", "mh_stereo_winners", _id)
    def _(dims=_dims):
        p, bust, gray, nb, flags, want = _scene(dims)
        cand = i32(np.flatnonzero(flags.reshape(-1)))
        return Call("mh_stereo_winners", [CTX, B("bust", In(bust)), f64(VMIN), VS, i32(dims), B("candidates", In(cand)), len(cand),
                                          B("census", In(want["census"])), B("neighbours", In(nb)), nb.shape[1], CELL, RADIUS,
                                          KEEP, B("keys", Out(want["keys"].shape, np.uint64)), STREAM], {"keys": want["keys"]},
                    ctx=p.ctx)

    @case("F", "mh_stereo_agree", _id)
    def _(dims=_dims):
        p, bust, gray, nb, flags, want = _scene(dims)
        return Call("mh_stereo_agree", [CTX, B("bust", In(bust)), f64(VMIN), VS, i32(dims), B("flags", In(flags.reshape(-1))),
                                        B("keys", In(want["keys"])), CELL, MAX_COST, float(M255),
                                        B("agree", Out(flags.size, np.int32)), STREAM], {"agree": want["agree"]}, ctx=p.ctx)

    @case("F", "mh_stereo_refine", _id)
    def _(dims=_dims):
        p, bust, gray, nb, flags, want = _scene(dims)
        return Call("mh_stereo_refine", [CTX, B("bust", In(bust)), f64(VMIN), VS, i32(dims), B("flags", In(flags.reshape(-1))),
                                         B("keys", In(want["keys"])), B("agree", In(want["agree"])), CELL, MAX_COST, float(M255),
                                         MIN_AGREE, MIN_THROUGH, B("refined", Out(flags.size, np.uint8)),
                                         B("depth", Out(want["depth"].shape, np.float32)), STREAM],
                    {"refined": want["refined"], "depth": want["depth"]}, ctx=p.ctx)
