"""Helper (not a test): the guarded C-ABI calls of the silhouette carve, entered into the ledger of tests/guard_cases.py when
this module is imported -- GUARDED and FAMILY there are the tables tests/test_guard_host.py holds against include/mh_pmvo.h, and
`case` is the decorator that fills them.  tests/test_hair_carve_guard_gpu.py imports this module and runs the cases on the arena
of tests/guard_arena.py; pytest imports every test module before it runs any test, so a run of the suite finds the four entry
points in the ledger.  (A run of tests/test_guard_host.py ALONE does not import this file: name
tests/test_hair_carve_guard_gpu.py beside it.)"""
import ctypes

import numpy as np

import guard_cases as G
from guard_cases import B, CTX, STREAM, Call, F_GRIDS, In, Out, Scratch, Size, case, f64, i32, i64

ENTRIES = ("mh_carve_votes", "mh_carve_inside", "mh_carve_mesh_count", "mh_carve_mesh")
VMIN, VS = (-0.06, -0.1, -0.1), 0.03


def _scene(dims):
    import hair_carve_np as hc

    p = G._pm(False, 3)
    rng = np.random.default_rng(2)
    bust = p.views.depth.copy()
    bust[rng.random(bust.shape) < 0.5] = 255
    want = hc.votes(p.views.cams, p.views.mask, bust, hc.centres(hc.grid_voxels(dims), f64(VMIN), VS))
    assert (want[:, 1] > 0).any()
    return p, bust, want


def _flags(dims):
    return (np.random.default_rng(sum(dims)).random(dims) < 0.4).astype(np.uint8)


def _scratch(dims):
    d = i32(dims)
    return Scratch(G._lib_().mh_carve_mesh_scratch_bytes(d.ctypes.data_as(ctypes.c_void_p)))


for _dims in F_GRIDS:
    _id = "%dx%dx%d" % _dims

    @case("F", "mh_carve_votes", _id)
    def _(dims=_dims):
        p, bust, want = _scene(dims)
        return Call("mh_carve_votes", [CTX, B("bust", In(bust)), f64(VMIN), VS, i32(dims),
                                       B("counts", Out((len(want), 3), np.int32)), STREAM], {"counts": want}, ctx=p.ctx)

    for _early in (0, 1):
        @case("F", "mh_carve_inside", "%s-early%d" % (_id, _early))
        def _(dims=_dims, early=_early):
            import hair_carve_np as hc

            p, bust, want = _scene(dims)
            flags = hc.inside_flags(want, 12, 5)          # bounds at which both clauses decide on this scene
            assert 0 < flags.sum() < len(flags)
            p.pm.set_lab_option("carve_early_exit", early)          # the two forms of the kernel; the default is put back
            call = Call("mh_carve_inside", [CTX, B("bust", In(bust)), f64(VMIN), VS, i32(dims), 12, 5,
                                            B("flags", Out(len(want), np.uint8)), STREAM], {"flags": flags}, ctx=p.ctx)
            call.after = lambda: p.pm.set_lab_option("carve_early_exit", 1)
            return call

    @case("F", "mh_carve_mesh_count", _id, scratch=True)
    def _(dims=_dims):
        import hair_carve_np as hc

        flags = _flags(dims)
        v, t = hc.mesh(flags, VMIN, VS)
        return Call("mh_carve_mesh_count", [CTX, B("flags", In(flags.reshape(-1))), i32(dims), B("counts", Out(2, np.int64)),
                                            B("scratch", _scratch(dims)), Size("scratch"), STREAM],
                    {"counts": i64([len(v), len(t)])})

    @case("F", "mh_carve_mesh", _id, scratch=True)
    def _(dims=_dims):
        import hair_carve_np as hc

        flags = _flags(dims)
        v, t = hc.mesh(flags, VMIN, VS)
        return Call("mh_carve_mesh", [CTX, B("flags", In(flags.reshape(-1))), f64(VMIN), VS, i32(dims), len(v), len(t),
                                      B("vertices", Out((len(v), 3), np.float32)), B("faces", Out((len(t), 3), np.int32)),
                                      B("scratch", _scratch(dims)), Size("scratch"), STREAM], {"vertices": v, "faces": t})
