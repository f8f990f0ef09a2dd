"""Helper (not a test): the table of guarded C-ABI calls for tests/test_guard_gpu.py and the ledger tests/test_guard_host.py
checks against include/mh_pmvo.h.

A case names an entry point and builds one Call: the argument list in the header's order, where every device buffer is a
B(name, role) with a role of tests/guard_arena.py, every host array a numpy array, and the number that states a scratch's size
a Size(name).  `expect` maps output names to what they must hold, taken from the modules the existing tests of that entry point
compare with (oracle.*, the *_np restatements, numpy one-liners): a plain array is required everywhere; a numpy MaskedArray is
required where it is not masked and must still hold the arena's FILL where it is (capacity an entry point is documented not to
write: seg_start behind G + 1, trace rows outside [first, first + len), untouched voxels).  Outputs without an entry are still
guarded and still have to come out the same for two fills.

GUARDED = {entry point: [Case]}; NOT_GUARDED = {entry point: reason} (empty: every entry point is guarded); FAMILY = {entry
point: letter of the issue's family}."""
import ctypes

import numpy as np

from guard_arena import In, InOut, Out, Scratch       # noqa: F401

MH_ERR_ARG = -1
CTX, STREAM = "<ctx>", "<stream>"

GUARDED = {}
NOT_GUARDED = {}
FAMILY = {}


class B:
    def __init__(self, name, role):
        self.name, self.role = name, role


class Size:
    def __init__(self, name, delta=0):
        self.name, self.delta = name, delta


class Pinned:
    """a page-locked host source (mh_upload_pinned)"""

    def __init__(self, array):
        self.array = np.ascontiguousarray(array)


class Outside:
    """a large read-only device input kept OUTSIDE the arena (a whole 256 x 256 x 192 volume of 16-byte voxels): uploaded
    once; nothing checks that it comes back unchanged"""

    def __init__(self, array):
        self.array, self.tensor = np.ascontiguousarray(array), None


class PtrArray:
    """a HOST array of device pointers, one per named buffer (the nei_* arguments of mh_connect_candidates)"""

    def __init__(self, names):
        self.names = list(names)


class Call:
    def __init__(self, entry, args, expect=None, rc=0, ctx=None, before=()):
        self.entry, self.args, self.expect, self.rc, self.ctx = entry, list(args), dict(expect or {}), rc, ctx
        self.before = list(before)      # calls that run first on the same arena (buffers of one name are one buffer)
        self.after = None               # called when the case is over (puts an option of a shared context back)

    def buffers(self):
        out = {}
        for c in self.before + [self]:
            for a in c.args:
                if isinstance(a, B) and a.name not in out:
                    out[a.name] = a.role
            for name, role in getattr(c, "extra", {}).items():       # buffers reached through a PtrArray
                out.setdefault(name, role)
        return out

    def undersized(self):
        """the same call stating one byte less than its scratch holds: the slice keeps its size, the call must refuse"""
        assert any(isinstance(a, Size) for a in self.args)
        args = [Size(a.name, a.delta - 1) if isinstance(a, Size) else a for a in self.args]
        return Call(self.entry, args, {}, MH_ERR_ARG, self.ctx)


class Partial:
    """an expectation in three parts: `values` (a MaskedArray: required where not masked, the arena's fill where masked) and
    `free`, elements whose value no reference states.  same=True: they are written, and must come out the same for both
    fills; same=False: the header leaves open whether they are written at all, and they are compared with nothing"""

    def __init__(self, values, free, same=False):
        self.values, self.free, self.same = values, np.asarray(free, bool), same


class Case:
    def __init__(self, entry, id, build, scratch):
        self.entry, self.id, self.build, self.scratch = entry, id, build, scratch


def case(family, entry, id, scratch=False):
    def deco(build):
        FAMILY.setdefault(entry, family)
        assert FAMILY[entry] == family
        GUARDED.setdefault(entry, []).append(Case(entry, id, build, scratch))
        return build
    return deco


def not_guarded(family, entry, reason):
    FAMILY[entry] = family
    NOT_GUARDED[entry] = reason


def bare_ctx():
    from monohair_amd.pmvo_utils import _ctx_for

    return _ctx_for("cuda:0")


def execute(call, seed, device="cuda:0"):
    """one call on a fresh arena filled with `seed` -> (return code, checked arena)"""
    import torch

    from guard_arena import Arena
    from monohair_amd import _lib

    arena = Arena(call.buffers(), seed, device)
    alive = []

    def run(c):
        cargs = []
        for a in c.args:
            if isinstance(a, B):
                cargs.append(arena.ptr(a.name))
            elif isinstance(a, Size):
                cargs.append(arena.roles[a.name].nbytes + a.delta)
            elif isinstance(a, np.ndarray):
                assert a.flags.c_contiguous
                cargs.append(a.ctypes.data_as(ctypes.c_void_p))
            elif isinstance(a, Outside):
                if a.tensor is None:
                    a.tensor = torch.from_numpy(a.array).to(device)
                cargs.append(ctypes.c_void_p(a.tensor.data_ptr()))
            elif isinstance(a, PtrArray):
                alive.append((ctypes.c_void_p * len(a.names))(*[arena.ptr(n).value for n in a.names]))
                cargs.append(ctypes.cast(alive[-1], ctypes.c_void_p))
            elif isinstance(a, Pinned):
                alive.append(torch.from_numpy(a.array.reshape(-1).view(np.uint8).copy()).pin_memory())
                cargs.append(ctypes.c_void_p(alive[-1].data_ptr()))
            elif isinstance(a, str) and a == CTX:
                cargs.append(c.ctx if c.ctx is not None else bare_ctx())
            elif isinstance(a, str) and a == STREAM:
                cargs.append(ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
            else:
                cargs.append(a)
        return getattr(_lib.lib(), c.entry)(*cargs)

    for c in call.before:
        rc = run(c)
        assert rc == 0, (c.entry, rc, _lib.lib().mh_last_error())
    rc = run(call)
    arena.check()
    return rc, arena


def f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def u8(a):
    return np.ascontiguousarray(a, dtype=np.uint8)


def f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def head(values, capacity):
    """values in front of a buffer of `capacity` elements (first axis) whose rest the entry point does not write"""
    values = np.asarray(values)
    full = np.zeros((capacity,) + values.shape[1:], values.dtype)
    full[:len(values)] = values
    mask = np.ones(full.shape, bool)
    mask[:len(values)] = False
    return np.ma.MaskedArray(full, mask)


SIZES = (1, 63, 64, 65, 255, 256, 257, 1023, 1025, 4097)


def _lib_():
    from monohair_amd import _lib

    return _lib.lib()


# ============================================================================ A. selection and sorting (csrc/sortgroup.hip)
def _cloud(n, seed=0):
    rng = np.random.default_rng(1000 + n + seed)
    pts = (rng.normal(size=(n, 3)) * np.array([1.0, 1e-3, 50.0]) + np.array([-3.0, 0.0, 7.0])).astype(np.float32)
    pts[rng.integers(0, n)] = [-0.0, 0.0, -1e-30]
    return pts


for _n in SIZES:
    @case("A", "mh_points_bbox", "n%d" % _n)
    def _(n=_n):
        pts = _cloud(n)
        return Call("mh_points_bbox", [CTX, B("points", In(pts)), n, B("out6", Out(6, np.float32)), STREAM],
                    {"out6": np.concatenate([pts.min(0), pts.max(0)])})

    for _dims in ((1, 1, 1), (5, 3, 2)):
        @case("A", "mh_grid_build", "n%d-%dx%dx%d" % ((_n,) + _dims), scratch=True)
        def _(n=_n, dims=_dims):
            rng = np.random.default_rng(n)
            pts = rng.uniform(-0.02, 0.07, (n, 3)).astype(np.float32)       # some outside the grid: clamped
            grid, d = f32([0.0, 0.0, 0.0, 0.0125]), i32(dims)
            c = np.clip(np.floor((pts - grid[:3]) / grid[3]), 0, d.astype(np.float32) - 1).astype(np.int64)     # in float32
            key = (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0]
            order = np.argsort(key, kind="stable")
            ncell = dims[0] * dims[1] * dims[2]
            return Call("mh_grid_build",
                        [CTX, grid, d, B("points", In(pts)), n, B("scratch", Scratch(_lib_().mh_grid_scratch_bytes(n))),
                         Size("scratch"), B("pts_sorted", Out((n, 3), np.float32)), B("order", Out(n, np.int32)),
                         B("cell_start", Out(ncell + 1, np.int32)), B("n_occupied", Out(1, np.int32)), STREAM],
                        {"pts_sorted": pts[order], "order": i32(order),
                         "cell_start": i32(np.searchsorted(key[order], np.arange(ncell + 1))),
                         "n_occupied": i32([len(np.unique(key))])})

    @case("A", "mh_sort_keys", "n%d" % _n, scratch=True)
    def _(n=_n):
        rng = np.random.default_rng(n)
        end_bit = 13
        keys = rng.integers(0, 1 << 40, n).astype(np.uint64)        # bits above end_bit do not take part
        order = np.argsort(keys & np.uint64((1 << end_bit) - 1), kind="stable")
        return Call("mh_sort_keys", [CTX, B("keys", In(keys)), n, end_bit,
                                     B("scratch", Scratch(_lib_().mh_sort_scratch_bytes(n))), Size("scratch"),
                                     B("keys_out", Out(n, np.uint64)), B("order", Out(n, np.int32)), STREAM],
                    {"keys_out": keys[order], "order": i32(order)})

    for _f64 in (0, 1):
        @case("A", "mh_voxel_group", "n%d-%s" % (_n, "f64" if _f64 else "f32"), scratch=True)
        def _(n=_n, is64=_f64):
            from monohair_amd.pmvo_utils import p2v

            rng = np.random.default_rng(n + is64)
            g, vmin, vs = np.array([7, 5, 3], np.int64), np.array([-0.02, -0.01, -0.005]), 0.0025
            pts = rng.uniform(-0.03, 0.03, (n, 3))
            k = rng.integers(0, 3, (n, 3))
            tie = (vmin + (k + 0.5) * vs) * np.array([1.0, -1.0, -1.0])       # round half to even
            pts[::3] = tie[::3]
            if n > 8:
                pts[1], pts[2] = [np.nan, 0, 0], [0, np.inf, -1e30]
            pts = pts.astype(np.float64 if is64 else np.float32)
            ori = rng.normal(size=(n, 3)).astype(np.float32)
            ori[::7, 1] = 0.0
            ori[3::11, 1] = -0.0
            with np.errstate(all="ignore"):
                x, y, z = p2v(pts.copy(), vmin, vs, g)
            key = (x.astype(np.int64) * int(g[1]) + y.astype(np.int64)) * int(g[2]) + z.astype(np.int64)
            order = np.argsort(key, kind="stable")
            want = ori.copy()
            want[want[:, 1] > 0] *= -1
            return Call("mh_voxel_group",
                        [CTX, B("points", In(pts)), is64, B("ori", In(ori)), n, f64(vmin), vs, i32(g),
                         B("scratch", Scratch(_lib_().mh_voxel_group_scratch_bytes(n))), Size("scratch"),
                         B("keys_sorted", Out(n, np.uint64)), B("order", Out(n, np.int32)),
                         B("ori_sorted", Out((n, 3), np.float32)), STREAM],
                        {"keys_sorted": key[order].astype(np.uint64), "order": i32(order), "ori_sorted": want[order]})

    for _mode in ("all", "plain"):
        @case("A", "mh_select_rows", "n%d-%s" % (_n, _mode), scratch=True)
        def _(n=_n, mode=_mode):
            rng = np.random.default_rng(n)
            flags = (rng.random(n) < 0.6).astype(np.uint8) * rng.integers(1, 255, n).astype(np.uint8)
            veto = (rng.random(n) < 0.3).astype(np.uint8)
            a, b = rng.normal(size=(n, 3)).astype(np.float32), rng.normal(size=(n, 3)).astype(np.float32)
            base, cap = 5, n + 5                     # rows [0, base) belong to an earlier selection: not written
            full = mode == "all"
            sel = ~((flags != 0) & (veto == 0)) if full else (flags != 0)           # inverted with the veto, or plain
            keep = np.flatnonzero(sel)

            def rows(x):
                m = np.ma.MaskedArray(np.zeros((cap,) + x.shape[1:], x.dtype), True)
                m[base:base + len(keep)] = x[keep]
                return m
            args = [CTX, B("flags", In(flags)), B("veto", In(veto)) if full else None, 1 if full else 0, n,
                    B("a", In(a)), B("b", In(b)) if full else None, B("a_out", Out((cap, 3), np.float32)),
                    B("b_out", Out((cap, 3), np.float32)) if full else None,
                    B("index_out", Out(cap, np.int32)) if full else None, B("base", In(i32([base]))),
                    B("count", Out(1, np.int32)), B("scratch", Scratch(_lib_().mh_select_scratch_bytes(n))),
                    Size("scratch"), STREAM]
            exp = {"a_out": rows(a), "count": i32([base + len(keep)])}
            if full:
                exp.update(b_out=rows(b), index_out=rows(i32(np.arange(n))))
            return Call("mh_select_rows", args, exp)

    @case("A", "mh_segment_heads", "n%d" % _n, scratch=True)
    def _(n=_n):
        rng = np.random.default_rng(n + 3)
        keys = (np.sort(rng.integers(0, max(1, n // 3), n)).astype(np.uint64) * np.uint64(7) + np.uint64(3))
        starts = np.flatnonzero(np.concatenate([[True], keys[1:] != keys[:-1]]))
        runs = np.diff(np.concatenate([starts, [n]]))
        return Call("mh_segment_heads", [CTX, B("keys_sorted", In(keys)), n, B("seg_start", Out(n + 1, np.int32)),
                                         B("head_keys", Out(n, np.uint64)), B("meta", Out(2, np.int32)),
                                         B("scratch", Scratch(_lib_().mh_select_scratch_bytes(n))), Size("scratch"), STREAM],
                    {"seg_start": head(i32(np.concatenate([starts, [n]])), n + 1), "head_keys": head(keys[starts], n),
                     "meta": i32([len(starts), runs.max()])})

    @case("A", "mh_flag_less", "n%d" % _n)
    def _(n=_n):
        rng = np.random.default_rng(n)
        x = rng.normal(size=n).astype(np.float32)
        x[::5] = np.float32(0.25)
        if n > 10:
            x[rng.integers(0, n, 3)] = np.nan
        return Call("mh_flag_less", [CTX, B("x", In(x)), 0.25, n, B("out", Out(n, np.uint8)), STREAM],
                    {"out": (x < np.float32(0.25)).astype(np.uint8)})

    for _same in (True, False):
        @case("A", "mh_buffers_differ", "n%d-%s" % (_n, "same" if _same else "last"))
        def _(n=_n, same=_same):
            a = np.random.default_rng(n).normal(size=n).astype(np.float32)
            a[0] = np.nan
            b = a.copy()
            if not same:
                b.view(np.uint32)[n - 1] ^= 1
            return Call("mh_buffers_differ", [CTX, B("a", In(a)), B("b", In(b)), ctypes.c_size_t(4 * n),
                                              B("flag", Out(1, np.int32)), STREAM], {"flag": i32([0 if same else 1])})


# ============================================================================ C. PMVO (22 views of 32 x 64, patches 3 and 7)
PV, PH, PW, THR, VIS_THR = 22, 32, 64, 0.15, 1
PMVO_N = (1, 3, 63, 65, 257)
_pmvo_cache = {}


class _Pm:
    """one resident context (fp32 planes or 8-bit codes) with the oracle's view of the same maps"""

    def __init__(self, codes, patch):
        import torch

        import oracle
        from monohair_amd import synth
        from monohair_amd.camera import camera_records, cameras_from_list
        from monohair_amd.pmvo import PMVO, depth_offsets

        kw = dict(device="cuda:0", patch_size=patch, visible_threshold=VIS_THR, conf_threshold=THR)
        if codes:       # the hand-written 8-bit scene of tests/test_search_staging_gpu.py, its context and its decoded views
            from test_search_staging_gpu import THR as SCENE_THR, Scene

            assert SCENE_THR == THR
            sc = Scene(PV, PH, PW, patch, 1, 0, codes=True)
            self.pm, self.views = sc.context(), sc.views()
        else:
            sc = synth.make_scene(PV, PH, PW, seed=1)
            cams = cameras_from_list(sc["cams"])
            rec = camera_records(cams)
            t = lambda x: x.contiguous().to("cuda:0")       # noqa: E731
            self.pm = PMVO.from_planes(rec, t(sc["depth"]), t(sc["ori"]), t(sc["conf"]), t(sc["mask"]), camera=cams, **kw)
            self.views = oracle.Views(rec, sc["depth"].numpy(), sc["ori"].numpy(), sc["conf"].numpy(), sc["mask"].numpy())
        torch.cuda.synchronize()
        self.ctx, self.patch, self.offsets = self.pm._ctx, patch, depth_offsets(90)
        self._front = {}

    def points(self, n):
        from monohair_amd import synth

        cand = synth.candidate_points(res=48, seed=2).astype(np.float32)
        assert len(cand) >= n
        return np.ascontiguousarray(cand[np.random.default_rng(7).permutation(len(cand))[:n]])

    def front(self, n):
        """the oracle's Compute_Visible_and_Ori and ranking of points(n)"""
        import oracle

        if n not in self._front:
            o = oracle.visible_and_ori(self.views, self.points(n), self.patch)
            o["base_idx"], o["base_val"] = oracle.topk_views(o["visible"], o["Conf"], 20)
            self._front[n] = o
        return self._front[n]


def _pm(codes=False, patch=3):
    if (codes, patch) not in _pmvo_cache:
        _pmvo_cache[(codes, patch)] = _Pm(codes, patch)
    return _pmvo_cache[(codes, patch)]


def _search_outs(n):
    return [B("line_ori", Out((n, 3), np.float32)), B("min_loss", Out(n, np.float32)), B("high_conf", Out(n, np.uint8)),
            B("best_sample", Out((n, 3), np.float32)), B("best_rank", Out(n, np.int32)), B("best_s", Out(n, np.int32))]


def _search_expect(p, n, own_ranking=True):
    import oracle

    o = p.front(n)
    _, lo, ml, hc, ex = oracle.forward(p.views, p.points(n), p.patch, THR, p.offsets, base_idx=o["base_idx"],
                                       base_val=o["base_val"], extra=True)
    return {"line_ori": lo, "min_loss": ml, "high_conf": hc.astype(np.uint8), "best_sample": ex["best_sample"],
            "best_rank": ex["best_rank"], "best_s": ex["best_s"]}


def _search_scratch(p, n):
    return Scratch(_lib_().mh_search_scratch_bytes(p.ctx, n, p.patch))


_GATHER = (("vis", "visible", ()), ("ori", "Ori", (2,)), ("conf", "Conf", ()), ("mask", "mask", ()),
           ("ori_patch", "Ori_patch", None), ("conf_patch", "Conf_patch", None), ("pixf", "pixf", (2,)))


def _project_gather(patch, n, drop=None):
    p = _pm(False, patch)
    o = p.front(n)
    outs = [None if name == drop else B(name, Out(o[key].shape, np.float32)) for name, key, _ in _GATHER]
    return Call("mh_project_gather", [CTX, B("points", In(p.points(n))), n, patch] + outs + [STREAM],
                {name: o[key] for name, key, _ in _GATHER if name != drop}, ctx=p.ctx)


def _front_outs(p, n, mask=True):
    return [B("vis", Out((PV, n), np.float32)), B("ori", Out((PV, n, 2), np.float32)), B("conf", Out((PV, n), np.float32)),
            B("mask", Out((PV, n), np.float32)) if mask else None]


def _front_expect(p, n, mask=True):
    o = p.front(n)
    e = {"vis": o["visible"], "ori": o["Ori"], "conf": o["Conf"]}
    if mask:
        e["mask"] = o["mask"]
    return e


def _forward_prepare(p, n, mask=True):
    return Call("mh_forward_prepare", [CTX, B("points", In(p.points(n))), n, p.patch, THR] + _front_outs(p, n, mask) +
                [B("scratch", _search_scratch(p, n)), Size("scratch"), STREAM], _front_expect(p, n, mask), ctx=p.ctx)


for _patch in (3, 7):
    for _n in PMVO_N:
        @case("C", "mh_project_gather", "p%d-n%d" % (_patch, _n))
        def _(patch=_patch, n=_n):
            return _project_gather(patch, n)

        @case("C", "mh_topk_views", "p%d-n%d" % (_patch, _n))
        def _(patch=_patch, n=_n):
            p = _pm(False, patch)
            o = p.front(n)
            return Call("mh_topk_views", [CTX, B("vis", In(o["visible"])), B("conf", In(o["Conf"])), n,
                                          B("out_idx", Out((20, n), np.int32)), B("out_val", Out((20, n), np.float32)), STREAM],
                        {"out_idx": o["base_idx"], "out_val": o["base_val"]}, ctx=p.ctx)

        for _codes in (False, True):
            @case("C", "mh_forward", "%s-p%d-n%d" % ("u8" if _codes else "f32", _patch, _n), scratch=True)
            def _(patch=_patch, n=_n, codes=_codes):
                p = _pm(codes, patch)
                o = p.front(n)
                exp = dict(_front_expect(p, n), base_idx=o["base_idx"], base_val=o["base_val"], **_search_expect(p, n))
                return Call("mh_forward", [CTX, B("points", In(p.points(n))), n, patch, THR, 10, 2] + _front_outs(p, n) +
                            [B("scratch", _search_scratch(p, n)), Size("scratch"), B("base_idx", Out((20, n), np.int32)),
                             B("base_val", Out((20, n), np.float32))] + _search_outs(n) + [STREAM], exp, ctx=p.ctx)

        @case("C", "mh_forward_prepare", "p%d-n%d" % (_patch, _n), scratch=True)
        def _(patch=_patch, n=_n):
            return _forward_prepare(_pm(False, patch), n)

        @case("C", "mh_search_prepared", "p%d-n%d" % (_patch, _n))
        def _(patch=_patch, n=_n):
            p = _pm(False, patch)
            o = p.front(n)
            return Call("mh_search_prepared",
                        [CTX, B("points", In(p.points(n))), n, patch, THR, 10, 2, B("ori", Out((PV, n, 2), np.float32)),
                         B("base_idx", In(o["base_idx"])), B("base_val", In(o["base_val"])), B("scratch", _search_scratch(p, n))]
                        + _search_outs(n) + [STREAM], dict(_front_expect(p, n), **_search_expect(p, n)), ctx=p.ctx,
                        before=[_forward_prepare(p, n)])

        @case("C", "mh_search_forward", "p%d-n%d" % (_patch, _n), scratch=True)
        def _(patch=_patch, n=_n):
            p = _pm(False, patch)
            o = p.front(n)
            return Call("mh_search_forward",
                        [CTX, B("points", In(p.points(n))), n, patch, THR, 10, 2, B("vis", In(o["visible"])),
                         B("ori", In(o["Ori"])), B("pixf", In(o["pixf"])), B("ori_patch", In(o["Ori_patch"])),
                         B("conf_patch", In(o["Conf_patch"])), B("base_idx", In(o["base_idx"])),
                         B("base_val", In(o["base_val"])), B("scratch", _search_scratch(p, n)), Size("scratch")]
                        + _search_outs(n) + [STREAM], _search_expect(p, n), ctx=p.ctx)

        for _maps in (False, True):
            @case("C", "mh_refine_loss_maps" if _maps else "mh_refine_loss", "p%d-n%d" % (_patch, _n))
            def _(patch=_patch, n=_n, maps=_maps):
                import oracle

                p = _pm(False, patch)
                o = p.front(n)
                dirs = np.random.default_rng(n).normal(size=(n, 3)).astype(np.float32)
                loss, hc = oracle.refine_loss(p.views, p.points(n), dirs, patch, THR)
                head_ = [CTX, B("points", In(p.points(n))), B("dir", In(dirs)), 0.005, 4.0, n, patch, THR]
                outs = [B("loss", Out(n, np.float32)), B("high_conf", Out(n, np.uint8))]
                exp = {"loss": loss, "high_conf": hc.astype(np.uint8)}
                if maps:
                    return Call("mh_refine_loss_maps", head_ + outs + [0, 0, 0, STREAM], exp, ctx=p.ctx)
                return Call("mh_refine_loss", head_ + [B("vis", In(o["visible"])), B("ori_patch", In(o["Ori_patch"])),
                                                       B("conf_patch", In(o["Conf_patch"]))] + outs + [STREAM], exp, ctx=p.ctx)


for _drop in [g[0] for g in _GATHER]:
    @case("C", "mh_project_gather", "p3-n65-no-%s" % _drop)
    def _(drop=_drop):
        return _project_gather(3, 65, drop)


@case("C", "mh_forward_prepare", "p3-n65-no-mask")
def _():
    return _forward_prepare(_pm(False, 3), 65, mask=False)


_FLAGS = ("surface_index", "filter_index", "unvisible_index", "head_filter")


def _filter(n, patch, drop=None, ordered=False):
    import oracle

    p = _pm(False, patch)
    pts = p.points(n)
    votes = oracle.filter_votes(p.views, pts, patch, THR, VIS_THR)
    outs = [None if name == drop else B(name, Out(n, np.uint8)) for name in _FLAGS]
    exp = {name: v.astype(np.uint8) for name, v in zip(_FLAGS, votes) if name != drop}
    args = [CTX, B("points", In(pts)), n, patch, THR, float(VIS_THR)] + outs + [0, 0, 0]
    if ordered:
        args.append(B("order", In(i32(np.random.default_rng(n).permutation(n)))))
    return Call("mh_filter_points_ordered" if ordered else "mh_filter_points", args + [STREAM], exp, ctx=p.ctx)


for _ordered in (False, True):
    _e = "mh_filter_points_ordered" if _ordered else "mh_filter_points"
    for _patch in (3, 7):
        for _n in PMVO_N + (4097,):
            @case("C", _e, "p%d-n%d" % (_patch, _n))
            def _(patch=_patch, n=_n, ordered=_ordered):
                return _filter(n, patch, None, ordered)
    for _n in (65, 4097):
        for _drop in _FLAGS:
            @case("C", _e, "p3-n%d-no-%s" % (_n, _drop))
            def _(n=_n, drop=_drop, ordered=_ordered):
                return _filter(n, 3, drop, ordered)


# ---- the stand-alone pieces
for _n in PMVO_N:
    for _drop in (None, "row_col", "z_half", "out_of_image", "pixel_unrounded"):
        if _drop and _n != 65:
            continue

        @case("C", "mh_project_points", "n%d%s" % (_n, "-no-" + _drop if _drop else ""))
        def _(n=_n, drop=_drop):
            import oracle

            p, v = _pm(False, 3), 5
            rc, zp, oob, pixf = oracle.project_points(p.views.cams[v], p.points(n), PH, PW)
            exp = {"row_col": rc, "z_half": zp, "out_of_image": oob.astype(np.uint8), "pixel_unrounded": pixf}
            outs = [None if k == drop else B(k, Out(e.shape, e.dtype)) for k, e in exp.items()]
            exp.pop(drop, None)
            return Call("mh_project_points", [CTX, v, B("points", In(p.points(n))), n] + outs + [STREAM], exp, ctx=p.ctx)

    for _size in (1, 3, 7):
        @case("C", "mh_gather_pixels", "n%d-s%d" % (_n, _size))
        def _(n=_n, size=_size):
            p, v = _pm(False, 3), 7
            rng = np.random.default_rng(n + size)
            rc = np.stack([rng.integers(0, PH, n), rng.integers(0, PW, n)], 1).astype(np.int64)
            rc[0] = [0, 0]
            rc[-1] = [PH - 1, PW - 1]
            hp = size // 2
            taps = [(np.clip(rc[:, 0] + i, 0, PH - 1), np.clip(rc[:, 1] + j, 0, PW - 1)) for i in range(-hp, hp + 1)
                    for j in range(-hp, hp + 1)]
            w = p.views
            rec = np.stack([np.concatenate([w.ori[v][a, b], w.conf[v][a, b][:, None], w.depth[v][a, b][:, None]], 1)
                            for a, b in taps], 1)
            return Call("mh_gather_pixels", [CTX, v, B("row_col", In(rc)), n, size, B("records", Out((n, size * size, 4), np.float32)),
                                             B("mask", Out((n, size * size), np.float32)), STREAM],
                        {"records": f32(rec), "mask": f32(np.stack([w.mask[v][a, b] for a, b in taps], 1))}, ctx=p.ctx)

    @case("C", "mh_compute_visible", "n%d" % _n)
    def _(n=_n):
        rng = np.random.default_rng(n)
        depth = rng.uniform(0, 255, n).astype(np.float32)
        z = (depth + rng.choice(np.array([-3, -0.05, 0, 0.05, 0.1, 0.15, 7], np.float32), n)).astype(np.float32)
        d = z - depth
        with np.errstate(all="ignore"):
            vis = np.where(d < np.float32(0.1), np.float32(1.0) - d / np.float32(0.1), np.float32(-1.0)).astype(np.float32)
        return Call("mh_compute_visible", [CTX, B("depth", In(depth)), B("z", In(z)), ctypes.c_size_t(n),
                                           B("out", Out(n, np.float32)), STREAM], {"out": np.clip(vis, -1, 1).astype(np.float32)})

    @case("C", "mh_sample_next", "n%d" % _n)
    def _(n=_n):
        import oracle

        p = _pm(False, 3)
        o = p.front(n)
        base = i32(o["base_idx"][2])
        return Call("mh_sample_next", [CTX, B("points", In(p.points(n))), B("base_view", In(base)), B("ori", In(o["Ori"])),
                                       B("offsets", In(p.offsets)), n, 90, B("samples", Out((n, 90, 3), np.float32)), STREAM],
                    {"samples": oracle.sample_next(p.views, p.points(n), base, o["Ori"], p.offsets)}, ctx=p.ctx)

    @case("C", "mh_reproject_ori", "n%d" % _n)
    def _(n=_n):
        import oracle

        p = _pm(False, 3)
        o = p.front(n)
        s = oracle.sample_next(p.views, p.points(n), i32(o["base_idx"][0]), o["Ori"], p.offsets[:7])
        return Call("mh_reproject_ori", [CTX, B("points", In(p.points(n))), B("samples", In(s)), n, 7,
                                         B("D", Out((PV, n, 7, 2), np.float32)), STREAM],
                    {"D": oracle.reproject_ori(p.views, p.points(n), s)}, ctx=p.ctx)

    for _all in (False, True):
        @case("C", "mh_prj_loss", "n%d%s" % (_n, "-all" if _all else ""))
        def _(n=_n, want_all=_all):
            import oracle

            p = _pm(False, 3)
            o = p.front(n)
            s = oracle.sample_next(p.views, p.points(n), i32(o["base_idx"][0]), o["Ori"], p.offsets[:7])
            D = oracle.reproject_ori(p.views, p.points(n), s)
            r = oracle.prj_loss(D, o["Ori_patch"], o["Conf_patch"], o["visible"], THR, want_all=want_all)
            exp = {"loss": r[0], "index": i64(r[1]), "high_conf": r[2].astype(np.uint8)}
            if want_all:
                exp["all_loss"] = r[3]
            return Call("mh_prj_loss", [CTX, B("D", In(D)), B("ori_patch", In(o["Ori_patch"])), B("conf_patch", In(o["Conf_patch"])),
                                        B("vis", In(o["visible"])), PV, n, 7, 9, THR, B("loss", Out(n, np.float32)),
                                        B("index", Out(n, np.int64)), B("high_conf", Out(n, np.uint8)),
                                        B("all_loss", Out((n, 7), np.float32)) if want_all else None, STREAM], exp, ctx=p.ctx)


for _bytes in (4, 12, 252, 260, 60000, 60002):
    for _pinned in (False, True):
        @case("C", "mh_upload_pinned" if _pinned else "mh_upload_async", "b%d" % _bytes)
        def _(nbytes=_bytes, pinned=_pinned):
            src = np.frombuffer(np.random.default_rng(nbytes).bytes(nbytes), np.uint8).copy()
            return Call("mh_upload_pinned" if pinned else "mh_upload_async",
                        [CTX, Pinned(src) if pinned else src, B("device", Out(nbytes, np.uint8)), ctypes.c_size_t(nbytes), STREAM],
                        {"device": src})


# ---- a refused search (nrank * S = 12 * 90 > 1024) writes nothing
def _refused(entry):
    p, n = _pm(False, 3), 65
    o = p.front(n)
    pts = B("points", In(p.points(n)))
    if entry == "mh_forward":
        args = [CTX, pts, n, 3, THR, 12, 1] + _front_outs(p, n) + [B("scratch", _search_scratch(p, n)), Size("scratch"),
                B("base_idx", Out((20, n), np.int32)), B("base_val", Out((20, n), np.float32))] + _search_outs(n)
    elif entry == "mh_search_prepared":
        args = [CTX, pts, n, 3, THR, 12, 1, B("ori", In(o["Ori"])), B("base_idx", In(o["base_idx"])),
                B("base_val", In(o["base_val"])), B("scratch", _search_scratch(p, n))] + _search_outs(n)
    else:
        args = [CTX, pts, n, 3, THR, 12, 1, B("vis", In(o["visible"])), B("ori", In(o["Ori"])), B("pixf", In(o["pixf"])),
                B("ori_patch", In(o["Ori_patch"])), B("conf_patch", In(o["Conf_patch"])), B("base_idx", In(o["base_idx"])),
                B("base_val", In(o["base_val"])), B("scratch", _search_scratch(p, n)), Size("scratch")] + _search_outs(n)
    return Call(entry, args + [STREAM], {}, MH_ERR_ARG, ctx=p.ctx)


for _e in ("mh_forward", "mh_search_prepared", "mh_search_forward"):
    @case("C", _e, "refused-12-ranks-of-90")
    def _(entry=_e):
        return _refused(entry)


# ============================================================================ D. images
IMAGE_SHAPES = ((1, 50), (50, 1), (5, 7), (33, 129), (31, 65))


def _gray(H, W):
    rng = np.random.default_rng(H * 1000 + W)
    r, c = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (127 + 70 * np.cos(2 * np.pi * (r * 0.8 + c * 0.6) / 4.0) + rng.normal(0, 6, (H, W))).clip(0, 255).astype(np.uint8)


def _gabor_ctx(variant):
    """the bare context with the host-built bank installed and the kernel variant selected"""
    from monohair_amd.gabor import calOrientationGabor

    gab = calOrientationGabor(device="cuda:0", variant=variant)
    gab._install_bank(1.8, 2.4, 4.0)
    return gab._ctx, lambda: gab.set_variant("mfma2")


for _H, _W in IMAGE_SHAPES:
    for _kind in ("u8", "f64"):
        for _drop in (None, "out64", "out32"):
            @case("D", "mh_dog", "%dx%d-%s%s" % (_H, _W, _kind, "-no-" + _drop if _drop else ""))
            def _(H=_H, W=_W, kind=_kind, drop=_drop):
                from monohair_amd.gabor import _dog_weights, difference_of_gaussians

                img = _gray(H, W) if kind == "u8" else np.random.default_rng(H * W).normal(size=(H, W))
                want = difference_of_gaussians(img, 0.4, 10)
                w0, r0, w1, r1 = _dog_weights(0.4, 10)
                exp = {"out64": f64(want), "out32": want.astype(np.float32)}
                outs = [None if k == drop else B(k, Out((H, W), e.dtype)) for k, e in exp.items()]
                exp.pop(drop, None)
                return Call("mh_dog", [CTX, B("image", In(img)), 0 if kind == "u8" else 1, H, W, w0, r0, w1, r1,
                                       B("scratch", Scratch(_lib_().mh_dog_scratch_bytes(H, W)))] + outs + [STREAM], exp)

    for _variant in ("mfma2", "valu"):
        for _drop in (None, "conf", "codes"):
            @case("D", "mh_gabor_view", "%dx%d-%s%s" % (_H, _W, _variant, "-no-" + _drop if _drop else ""))
            def _(H=_H, W=_W, variant=_variant, drop=_drop):
                import oracle
                from monohair_amd.gabor import _dog_weights, difference_of_gaussians, gabor_bank

                im = _gray(H, W)
                ctx, after = _gabor_ctx(variant)
                o_idx, o_conf, o_var = oracle.gabor_bank(gabor_bank(), difference_of_gaussians(im, 0.4, 10).astype(np.float32))
                exp = {"orient_index": i32(o_idx), "conf": o_conf, "variance": o_var,
                       "k8": np.clip(o_idx, 0, 255).astype(np.uint8),
                       "c8": np.clip(o_conf * np.float32(255.0) + np.float32(0.5), 0, 255).astype(np.uint8)}
                gone = {"conf": ("conf",), "codes": ("k8", "c8"), None: ()}[drop]
                outs = [None if k in gone else B(k, Out((H, W), e.dtype)) for k, e in exp.items()]
                for k in gone:
                    exp.pop(k)
                w0, r0, w1, r1 = _dog_weights(0.4, 10)
                call = Call("mh_gabor_view", [CTX, B("gray", In(im)), H, W, w0, r0, w1, r1,
                                              B("scratch", Scratch(_lib_().mh_gabor_view_scratch_bytes(H, W)))] + outs +
                            [STREAM], exp, ctx=ctx)
                call.after = after
                return call

        @case("D", "mh_gabor_bank", "%dx%d-%s" % (_H, _W, _variant))
        def _(H=_H, W=_W, variant=_variant):
            import oracle
            from monohair_amd.gabor import gabor_bank

            img = np.random.default_rng(H + W).normal(size=(H, W)).astype(np.float32)
            ctx, after = _gabor_ctx(variant)
            o_idx, o_conf, o_var = oracle.gabor_bank(gabor_bank(), img)
            call = Call("mh_gabor_bank", [CTX, B("image", In(img)), H, W, B("orient_index", Out((H, W), np.int32)),
                                          B("conf", Out((H, W), np.float32)), B("variance", Out((H, W), np.float32)), STREAM],
                        {"orient_index": i32(o_idx), "conf": o_conf, "variance": o_var}, ctx=ctx)
            call.after = after
            return call


def _raster_setup(H, W):
    import oracle
    from monohair_amd import _lib, synth
    from monohair_amd.camera import camera_records, cameras_from_list
    from test_raster_host import uv_sphere

    ctx = bare_ctx()
    # (the defaults of a context: set here only in case an earlier test of the session left the shared context otherwise, so
    # there is nothing to put back afterwards)
    _lib.check(_lib.lib().mh_ctx_set_option(ctx, b"line_rule", 0))
    _lib.check(_lib.lib().mh_ctx_set_option(ctx, b"raster_subpixel_bits", 8))
    oracle.set_subpixel_bits(8)
    rec = camera_records(cameras_from_list(synth.make_cameras(4, H, W, scale=1.2, rings=2)))[1]
    v, f = uv_sphere(0.11, 12, 24)
    return np.ascontiguousarray(rec, np.float32), f32(v), i32(f)


for _H, _W in IMAGE_SHAPES:
    for _ch in (1, 3):
        @case("D", "mh_render_depth", "%dx%d-c%d" % (_H, _W, _ch), scratch=True)
        def _(H=_H, W=_W, ch=_ch):
            import oracle

            rec, v, f = _raster_setup(H, W)
            want, _ = oracle.render_depth(rec, v, f, H, W, 0.5, ch)
            return Call("mh_render_depth",
                        [CTX, rec, B("verts", In(v)), len(v), B("faces", In(f)), len(f), H, W, 0.5,
                         B("scratch", Scratch(_lib_().mh_render_scratch_bytes(len(v), len(f), H, W))), Size("scratch"),
                         B("out", Out((H, W, ch), np.float32)), ch, STREAM], {"out": f32(want).reshape(H, W, ch)})

    @case("D", "mh_render_strands", "%dx%d" % (_H, _W), scratch=True)
    def _(H=_H, W=_W):
        import oracle
        from monohair_amd.render import strand_line_buffers
        from test_raster_gpu import _random_strands

        rec, v, f = _raster_setup(H, W)
        strands = _random_strands(np.random.default_rng(H + W), 40)
        strands.append(np.array([[0.2, 0, 0], [0.2, 0, 0]]))
        lp, lt = (f32(x) for x in strand_line_buffers(strands))
        nseg = len(lp) // 2
        want, _, _ = oracle.render_strands(rec, v, f, lp, lt, H, W, 0.5, 3, 2, 1, 0.0)
        return Call("mh_render_strands",
                    [CTX, rec, B("verts", In(v)), len(v), B("faces", In(f)), len(f), B("line_pts", In(lp)),
                     B("line_tan", In(lt)), nseg, H, W, 0.5, 3, 2, 1, 0.0,
                     B("scratch", Scratch(_lib_().mh_render_strands_scratch_bytes(len(v), len(f), nseg, H, W))),
                     Size("scratch"), B("out", Out((H, W, 3), np.float32)), STREAM], {"out": want})


# ============================================================================ F. strand-set stages
STRAND_SETS = {"1x1": [1], "1x2": [2], "1x65": [65], "3": [1, 2, 65], "65x2": [2] * 65, "65": ([65, 1, 2] * 22)[:65]}
F_IMAGES = ((5, 7), (33, 17))
F_GRIDS = ((3, 5, 7), (5, 4, 3))
_hair_cache = {}


def _offsets(counts):
    return i64(np.concatenate([[0], np.cumsum(np.asarray(counts, np.int64))]))


def _hair(name):
    """(counts, world points float32 [n,3]) of a strand set: strands of monohair_amd.synth_hair.make_hairstyle cut to 1, 2
    and 65 points (a strand of two points spans the whole strand: one long segment)"""
    from monohair_amd import synth_hair as sh

    if name not in _hair_cache:
        counts = STRAND_SETS[name]
        _, p = sh.make_hairstyle(len(counts), 65, seed=4)
        p = p.reshape(len(counts), 65, 3)
        pts = [p[i, np.linspace(0, 64, c).astype(int) if c > 1 else [0]] for i, c in enumerate(counts)]
        _hair_cache[name] = (np.asarray(counts, np.int64), f32(np.concatenate(pts)))
    return _hair_cache[name]


def _view(H, W, name):
    """camera record, the oracle's vertices (row, col, z255) and valid flags of a strand set in a view, an occluder plane"""
    import oracle
    from monohair_amd import synth
    from monohair_amd.camera import camera_records, cameras_from_list

    counts, pts = _hair(name)
    rec = np.ascontiguousarray(camera_records(cameras_from_list(synth.make_cameras(3, H, W)))[1], np.float32)
    # (a point alone in its batch is projected by another product form: project with one more row)
    _, zp, _, pixf = (a[:-1] for a in oracle.project_points(rec, np.concatenate([pts, np.zeros((1, 3), np.float32)]), H, W))
    vert = f32(np.concatenate([pixf, (zp * np.float32(255.0)).astype(np.float32)[:, None]], 1))
    valid = ((-(zp * np.float32(2.0)) < np.float32(-0.1)) & (np.abs(vert[:, 0]) < 2.0 ** 20) &
             (np.abs(vert[:, 1]) < 2.0 ** 20)).astype(np.uint8)
    rng = np.random.default_rng(H * W)
    depth0 = None
    if H > 5:
        depth0 = rng.uniform(float(np.median(vert[:, 2])) - 2, float(vert[:, 2].max()) + 5, (H, W)).astype(np.float32)
        depth0[rng.random((H, W)) < 0.3] = 255
    return rec, counts, pts, vert, valid, depth0


def _opt(name, arr):
    return None if arr is None else B(name, In(arr))


def _project_call(H, W, name):
    rec, counts, pts, _, _, _ = _view(H, W, name)
    n = len(pts)
    return Call("mh_capture_project", [CTX, rec, B("points", In(pts)), n, H, W, B("vert", Out((n, 3), np.float32)),
                                       B("valid", Out(n, np.uint8)), STREAM])


def _observed(H, W):
    rng = np.random.default_rng(H + W)
    return (rng.integers(0, 200, (H, W)).astype(np.uint8), rng.integers(0, 256, (H, W)).astype(np.uint8),
            rng.choice(np.array([0, 51, 52, 255], np.uint8), (H, W)))


def _same(outs, want):
    for k, w in want.items():
        g = outs[k]
        w = np.asarray(w).reshape(g.shape)
        assert g.dtype == w.dtype and g.tobytes() == w.tobytes(), (k, int((g != w).sum()))


for (_H, _W) in F_IMAGES:
    for _set in STRAND_SETS:
        _id = "%dx%d-%s" % (_H, _W, _set)

        @case("F", "mh_capture_project", _id)
        def _(H=_H, W=_W, name=_set):
            import oracle

            call = _project_call(H, W, name)
            rec, counts, pts, _, _, _ = _view(H, W, name)

            def check(outs):
                # as tests/test_hair_capture_gpu.py holds the projection to PMVO's own: z255 = z_half * 255, the rounded pixel of
                # every in-bounds vertex, and the validity rule restated on the projected values
                vert, valid = outs["vert"], outs["valid"]
                more = np.concatenate([pts, np.zeros((1, 3), np.float32)])
                rc, zp, oob, _ = (a[:-1] for a in oracle.project_points(rec, more, H, W))
                assert (zp * np.float32(255.0)).astype(np.float32).tobytes() == vert[:, 2].tobytes()
                assert np.array_equal(np.rint(vert[~oob, :2]).astype(np.int64), rc[~oob])
                rule = (-(zp * np.float32(2.0)) < np.float32(-0.1)) & (np.abs(vert[:, 0]) < 2.0 ** 20) & \
                    (np.abs(vert[:, 1]) < 2.0 ** 20)
                assert np.array_equal(rule, valid != 0)
            call.expect = {"vert": check}
            return call

        @case("F", "mh_capture_zmin", _id)
        def _(H=_H, W=_W, name=_set):
            import hair_capture_np as hc

            rec, counts, pts, vert, valid, d0 = _view(H, W, name)
            ref = hc.capture(vert, valid, counts, H, W, radius=1, depth0=d0)
            return Call("mh_capture_zmin", [CTX, B("vert", In(vert)), B("valid", In(valid)), B("offsets", In(_offsets(counts))),
                                            len(counts), len(pts), H, W, 1, _opt("depth0", d0), B("zmin", Out((H, W), np.float32)),
                                            B("dropped", Out(1, np.int32)), STREAM],
                        {"zmin": ref["zmin"], "dropped": i32([ref["dropped"]])})

        @case("F", "mh_capture_accumulate", _id)
        def _(H=_H, W=_W, name=_set):
            import hair_capture_np as hc

            rec, counts, pts, vert, valid, d0 = _view(H, W, name)
            ref = hc.capture(vert, valid, counts, H, W, radius=1, depth0=d0)
            return Call("mh_capture_accumulate",
                        [CTX, B("vert", In(vert)), B("valid", In(valid)), B("offsets", In(_offsets(counts))), len(counts),
                         len(pts), H, W, 1, 0.25, _opt("depth0", d0), B("zmin", In(ref["zmin"])), B("cnt", Out((H, W), np.int32)),
                         B("c2", Out((H, W), np.int64)), B("s2", Out((H, W), np.int64)), STREAM],
                        {k: ref[k] for k in ("cnt", "c2", "s2")})

        @case("F", "mh_capture_resolve", _id)
        def _(H=_H, W=_W, name=_set):
            import hair_capture_np as hc

            rec, counts, pts, vert, valid, d0 = _view(H, W, name)
            ref = hc.capture(vert, valid, counts, H, W, radius=1, depth0=d0)
            return Call("mh_capture_resolve",
                        [CTX, B("zmin", In(ref["zmin"])), B("cnt", In(ref["cnt"])), B("c2", In(ref["c2"])), B("s2", In(ref["s2"])),
                         _opt("depth0", d0), hc.code_table(), 3, H, W, B("depth", Out((H, W), np.float32)),
                         B("ori_u8", Out((H, W), np.uint8)), B("conf_u8", Out((H, W), np.uint8)),
                         B("mask_u8", Out((H, W), np.uint8)), STREAM],
                        {k: ref[k] for k in ("depth", "ori_u8", "conf_u8", "mask_u8")})

        @case("F", "mh_capture_view", _id, scratch=True)
        def _(H=_H, W=_W, name=_set):
            import hair_capture_np as hc

            rec, counts, pts, _, _, d0 = _view(H, W, name)

            def check(outs):        # on the vertices the device projected (the call before), as the existing tests do
                ref = hc.capture(outs["vert"], outs["valid"], counts, H, W, radius=1, depth0=d0)
                _same(outs, {k: ref[k] for k in ("depth", "ori_u8", "conf_u8", "mask_u8")})
            return Call("mh_capture_view",
                        [CTX, rec, B("points", In(pts)), B("offsets", In(_offsets(counts))), len(counts), len(pts), H, W, 1, 0.25,
                         3, _opt("depth0", d0), hc.code_table(),
                         B("scratch", Scratch(_lib_().mh_capture_scratch_bytes(len(pts), H, W))), Size("scratch"),
                         B("depth", Out((H, W), np.float32)), B("ori_u8", Out((H, W), np.uint8)),
                         B("conf_u8", Out((H, W), np.uint8)), B("mask_u8", Out((H, W), np.uint8)), STREAM],
                        {"depth": check}, before=[_project_call(H, W, name)])

        # ---- the photograph
        @case("F", "mh_photo_shade", _id)
        def _(H=_H, W=_W, name=_set):
            import hair_photo_np as hp

            rec, counts, pts, vert, valid, d0 = _view(H, W, name)
            albedo = np.random.default_rng(len(counts)).uniform(0.35, 1.0, len(counts)).astype(np.float32)
            light = f64([0.6, 0.0, 0.8])
            return Call("mh_photo_shade", [CTX, B("points", In(pts)), B("valid", In(valid)), B("offsets", In(_offsets(counts))),
                                           len(counts), len(pts), B("albedo", In(albedo)), light, 0.3,
                                           B("shade", Out(len(pts), np.uint8)), STREAM],
                        {"shade": hp.segment_shades(pts, valid, counts, albedo, light, 0.3)})

        for _S in (1, 2):
            @case("F", "mh_photo_front", "%s-s%d" % (_id, _S))
            def _(H=_H, W=_W, name=_set, S=_S):
                import hair_photo_np as hp

                rec, counts, pts, vert, valid, d0 = _view(H, W, name)
                shade = np.random.default_rng(3).integers(0, 256, len(pts)).astype(np.uint8)
                ref = hp.photo(vert, valid, counts, shade, H, W, S=S, w=1, depth0=d0)
                return Call("mh_photo_front",
                            [CTX, B("vert", In(vert)), B("valid", In(valid)), B("offsets", In(_offsets(counts))), len(counts),
                             len(pts), B("shade", In(shade)), H, W, S, 1, _opt("depth0", d0),
                             B("keys", Out((S * H, S * W), np.uint64)), B("dropped", Out(1, np.int32)), STREAM],
                            {"keys": ref["keys"], "dropped": i32([ref["dropped"]])})

            for _cover in (True, False):
                _id2 = "%s-s%d%s" % (_id, _S, "" if _cover else "-no-cover")

                @case("F", "mh_photo_resolve", _id2)
                def _(H=_H, W=_W, name=_set, S=_S, cover=_cover):
                    import hair_photo_np as hp

                    rec, counts, pts, vert, valid, d0 = _view(H, W, name)
                    shade = np.random.default_rng(3).integers(0, 256, len(pts)).astype(np.uint8)
                    ref = hp.photo(vert, valid, counts, shade, H, W, S=S, w=1, depth0=d0, bust_code=64, background_code=32)
                    exp = {"gray_u8": ref["gray"]}
                    if cover:
                        exp["cover"] = ref["cover"]
                    return Call("mh_photo_resolve", [CTX, B("keys", In(ref["keys"])), _opt("depth0", d0), H, W, S, 64, 32,
                                                     B("gray_u8", Out((H, W), np.uint8)),
                                                     B("cover", Out((H, W), np.int32)) if cover else None, STREAM], exp)

                @case("F", "mh_photo_view", _id2, scratch=True)
                def _(H=_H, W=_W, name=_set, S=_S, cover=_cover):
                    import hair_photo_np as hp

                    rec, counts, pts, _, _, d0 = _view(H, W, name)
                    albedo = np.random.default_rng(len(counts)).uniform(0.35, 1.0, len(counts)).astype(np.float32)
                    light = f64([0.6, 0.0, 0.8])

                    def check(outs):
                        shade = hp.segment_shades(pts, outs["valid"], counts, albedo, light, 0.3)
                        ref = hp.photo(outs["vert"], outs["valid"], counts, shade, H, W, S=S, w=1, depth0=d0, bust_code=64,
                                       background_code=32)
                        _same(outs, dict({"gray_u8": ref["gray"]}, **({"cover": ref["cover"]} if cover else {})))
                    return Call("mh_photo_view",
                                [CTX, rec, B("points", In(pts)), B("offsets", In(_offsets(counts))), len(counts), len(pts),
                                 B("albedo", In(albedo)), light, 0.3, H, W, S, 1, _opt("depth0", d0), 64, 32,
                                 B("scratch", Scratch(_lib_().mh_photo_scratch_bytes(len(pts), H, W, S))), Size("scratch"),
                                 B("gray_u8", Out((H, W), np.uint8)), B("cover", Out((H, W), np.int32)) if cover else None,
                                 STREAM], {"gray_u8": check}, before=[_project_call(H, W, name)])

        # ---- capture agreement
        @case("F", "mh_support_accumulate", _id)
        def _(H=_H, W=_W, name=_set):
            import hair_capture_np as hc
            import hair_reproj_np as hr

            rec, counts, pts, vert, valid, d0 = _view(H, W, name)
            o8, c8, m8 = _observed(H, W)
            bounds = hr.bounds_of([10.0, 30.0])
            ref = hr.support(vert, valid, counts, H, W, o8, c8, m8, 40, bounds, radius=1, depth0=d0)
            preset = np.random.default_rng(5).integers(1, 1000, (len(counts), 6)).astype(np.int64)
            return Call("mh_support_accumulate",
                        [CTX, B("vert", In(vert)), B("valid", In(valid)), B("offsets", In(_offsets(counts))), len(counts),
                         len(pts), H, W, 0.25, _opt("depth0", d0), B("zmin", In(ref["zmin"])), B("ori_u8", In(o8)),
                         B("conf_u8", In(c8)), B("mask_u8", In(m8)), 40, hc.code_table(), bounds, 2,
                         B("strand_counts", InOut(preset)), B("view_counts", Out(6, np.int64)), STREAM],
                        {"strand_counts": preset + ref["strand"], "view_counts": ref["view"]})

        @case("F", "mh_support_silhouette", _id)
        def _(H=_H, W=_W, name=_set):
            import hair_capture_np as hc

            rec, counts, pts, vert, valid, d0 = _view(H, W, name)
            zmin = hc.capture(vert, valid, counts, H, W, radius=1, depth0=d0)["zmin"]
            m8 = _observed(H, W)[2]
            pred, obs = np.isfinite(zmin), m8 >= 52
            return Call("mh_support_silhouette", [CTX, B("zmin", In(zmin)), B("mask_u8", In(m8)), H, W,
                                                  B("silhouette", Out(3, np.int64)), STREAM],
                        {"silhouette": i64([(pred & obs).sum(), (pred & ~obs).sum(), (~pred & obs).sum()])})

        @case("F", "mh_support_view", _id, scratch=True)
        def _(H=_H, W=_W, name=_set):
            import hair_capture_np as hc
            import hair_reproj_np as hr

            rec, counts, pts, _, _, d0 = _view(H, W, name)
            o8, c8, m8 = _observed(H, W)
            bounds = hr.bounds_of([10.0, 30.0])
            preset = np.random.default_rng(5).integers(1, 1000, (len(counts), 6)).astype(np.int64)

            def check(outs):
                ref = hr.support(outs["vert"], outs["valid"], counts, H, W, o8, c8, m8, 40, bounds, radius=1, depth0=d0)
                _same(outs, {"strand_counts": preset + ref["strand"], "view_counts": ref["view"], "silhouette": ref["silhouette"]})
            return Call("mh_support_view",
                        [CTX, rec, B("points", In(pts)), B("offsets", In(_offsets(counts))), len(counts), len(pts), H, W, 1, 0.25,
                         _opt("depth0", d0), B("ori_u8", In(o8)), B("conf_u8", In(c8)), B("mask_u8", In(m8)), 40, hc.code_table(),
                         bounds, 2, B("scratch", Scratch(_lib_().mh_support_scratch_bytes(len(pts), H, W))), Size("scratch"),
                         B("strand_counts", InOut(preset)), B("view_counts", Out(6, np.int64)), B("silhouette", Out(3, np.int64)),
                         STREAM], {"silhouette": check}, before=[_project_call(H, W, name)])


# ---- strand metrics
for _set in STRAND_SETS:
    @case("F", "mh_strand_arclen", _set)
    def _(name=_set):
        import hair_metrics_np as hm

        counts, pts = _hair(name)
        step = 0.003
        cum = np.concatenate([hm.cumulative_length(s.astype(np.float64)) for s in hm._strands(counts, pts)])
        return Call("mh_strand_arclen", [CTX, B("points", In(pts)), B("offsets", In(_offsets(counts))), len(counts), step,
                                         B("cum_length", Out(len(pts), np.float64)), B("n_samples", Out(len(counts), np.int64)),
                                         STREAM], {"cum_length": cum, "n_samples": hm.resample(counts, pts, step)[0]})

    @case("F", "mh_strand_resample", _set)
    def _(name=_set):
        import hair_metrics_np as hm

        counts, pts = _hair(name)
        step = 0.003
        cum = np.concatenate([hm.cumulative_length(s.astype(np.float64)) for s in hm._strands(counts, pts)])
        m, out = hm.resample(counts, pts, step)
        return Call("mh_strand_resample", [CTX, B("points", In(pts)), B("offsets", In(_offsets(counts))), B("cum_length", In(cum)),
                                           B("sample_offsets", In(_offsets(m))), len(counts), len(out), step,
                                           B("out_points", Out((len(out), 3), np.float32)), STREAM], {"out_points": out})

    @case("F", "mh_strand_tangents", _set)
    def _(name=_set):
        import hair_metrics_np as hm

        counts, pts = _hair(name)
        pts = pts.copy()
        if len(pts) > 3:
            pts[2] = pts[0]             # coincident neighbours: no direction at point 1
        tan, valid = hm.tangents(counts, pts)
        return Call("mh_strand_tangents", [CTX, B("points", In(pts)), B("offsets", In(_offsets(counts))), len(counts), len(pts),
                                           B("tangents", Out((len(pts), 3), np.float64)), B("valid", Out(len(pts), np.uint8)),
                                           STREAM], {"tangents": tan, "valid": valid})

    @case("F", "mh_strand_match", _set)
    def _(name=_set):
        import hair_metrics_np as hm

        counts, q = _hair(name)
        q_tan, q_valid = hm.tangents(counts, q)
        tc, t = _hair("65")
        t = f32(t + np.float32(0.0007))
        t_tan, t_valid = hm.tangents(tc, t)
        t, t_tan = t[t_valid != 0], t_tan[t_valid != 0]
        r2, cosb = hm.bounds([(0.002, 20.0), (0.004, 45.0)])
        h = np.float32(0.006)                                    # the cell exceeds the largest radius by half of it
        lo = t.min(0)
        dims = i32(np.floor((t.max(0) - lo).astype(np.float64) / float(h)) + 1)
        grid = f32([lo[0], lo[1], lo[2], h])

        def cells(p):
            c = np.clip(np.floor((p - grid[:3]) / grid[3]), 0, dims.astype(np.float32) - 1).astype(np.int64)     # in float32
            return (c[:, 2] * int(dims[1]) + c[:, 1]) * int(dims[0]) + c[:, 0]
        key = cells(t)
        order = np.argsort(key, kind="stable")
        cstart = i32(np.searchsorted(key[order], np.arange(int(np.prod(dims)) + 1)))
        q_order = i32(np.argsort(cells(q), kind="stable"))
        want = hm.match_flags(q, q_tan, q_valid, t, t_tan, np.ones(len(t), np.uint8), r2, cosb)
        return Call("mh_strand_match",
                    [CTX, B("q_points", In(q)), B("q_tangents", In(q_tan)), B("q_valid", In(q_valid)), B("q_order", In(q_order)),
                     len(q), B("t_points_sorted", In(t[order])), B("t_tangents_sorted", In(t_tan[order])), len(t),
                     B("cell_start", In(cstart)), grid, dims, f64(r2), f64(cosb), 2, B("out_flags", Out(len(q), np.uint8)), STREAM],
                    {"out_flags": want})


for _n in (1, 63, 65, 257, 4097):
    @case("F", "mh_flag_counts", "n%d" % _n)
    def _(n=_n):
        rng = np.random.default_rng(n)
        flags, valid = rng.integers(0, 256, n).astype(np.uint8), (rng.random(n) < 0.7).astype(np.uint8) * 3
        want = [int(((flags >> k) & 1).sum()) for k in range(8)] + [int((valid != 0).sum())]
        return Call("mh_flag_counts", [CTX, B("flags", In(flags)), B("valid", In(valid)), n, B("out9", Out(9, np.uint64)), STREAM],
                    {"out9": np.asarray(want, np.uint64)})


# ---- strand volume, volume scores
VS_, BUST_ = 0.0025, (0.001, -0.002, 0.003)


def _volume_case(dims, name):
    """a strand set inside (and leaving) a small grid: voxel-space walks through tests/test_hair_volume_gpu.py's _world"""
    import hair_volume_np as hv
    from test_hair_volume_gpu import _vmin, _world

    counts = np.asarray(STRAND_SETS[name], np.int64)
    rng = np.random.default_rng(sum(dims) + len(counts))
    d = np.array(dims, np.float64)
    st = []
    for c in counts:
        a, b = rng.uniform(-1.0, d), rng.uniform(-1.0, d)
        t = np.linspace(0.0, 1.0, c)[:, None] if c > 1 else np.ones((1, 1))
        st.append(a[None, :] * (1.0 - t) + b[None, :] * t + rng.normal(0.0, 0.2, (c, 3)))
    vmin = _vmin(dims)
    pts = _world(np.concatenate(st, 0), vmin, VS_, BUST_)
    acc, dropped, outside = hv.accumulate(counts, pts, BUST_, vmin, VS_, dims, 2)
    return counts, pts, vmin, acc, dropped, outside


for _dims in F_GRIDS:
    for _set in STRAND_SETS:
        _id = "%dx%dx%d-%s" % (_dims + (_set,))

        @case("F", "mh_strand_volume_accumulate", _id)
        def _(dims=_dims, name=_set):
            counts, pts, vmin, acc, dropped, outside = _volume_case(dims, name)
            nvox = int(np.prod(dims))
            acc8 = np.zeros((nvox, 8), np.int64)
            acc8[:, :7] = acc.reshape(nvox, 7)
            return Call("mh_strand_volume_accumulate",
                        [CTX, B("points", In(pts)), B("offsets", In(_offsets(counts))), len(counts), len(pts), f64(BUST_), f64(vmin),
                         VS_, i32(dims), 2, B("acc", Out((nvox, 8), np.int64)), B("occ", Out(nvox, np.uint8)),
                         B("counters", Out(2, np.int64)), STREAM],
                        {"acc": acc8, "occ": (acc8[:, 0] > 0).astype(np.uint8), "counters": i64([dropped, outside])})

        for _sums in (True, False):
            @case("F", "mh_strand_volume_resolve", _id + ("" if _sums else "-no-sums"))
            def _(dims=_dims, name=_set, sums=_sums):
                import hair_volume_np as hv

                counts, pts, vmin, acc, dropped, outside = _volume_case(dims, name)
                nvox = int(np.prod(dims))
                acc8 = np.zeros((nvox, 8), np.int64)
                acc8[:, :7] = acc.reshape(nvox, 7)
                ref = hv.resolve(acc)
                G = len(ref["voxels"])
                index = i32(np.flatnonzero(acc8[:, 0] > 0))
                exp = {k: ref[k] for k in ("voxels", "ori", "cnt", "coh")}
                exp["refused"] = i32([0])
                if sums:
                    exp["sums"] = ref["sums"]
                return Call("mh_strand_volume_resolve",
                            [CTX, B("acc", In(acc8)), B("index", In(index)), G, i32(dims), B("voxels", Out((G, 3), np.int64)),
                             B("ori", Out((G, 3), np.float32)), B("cnt", Out(G, np.int32)), B("coh", Out(G, np.float64)),
                             B("sums", Out((G, 6), np.int64)) if sums else None, B("refused", Out(1, np.int32)), STREAM], exp)

    for _nv in (1, 3, 65):
        _id = "%dx%dx%d-n%d" % (_dims + (_nv,))

        @case("F", "mh_volume_index", _id)
        def _(dims=_dims, n=_nv):
            from test_hair_volume_gpu import _volume

            v, _ = _volume(dims, 1, min(max(n - 2, 1), int(np.prod(dims)) - 2))      # (with the two corners: n voxels, or all)
            v = v[:n] if n < 3 else v
            key = (v[:, 0] * dims[1] + v[:, 1]) * dims[2] + v[:, 2]
            index = np.full(int(np.prod(dims)), -1, np.int32)
            index[key] = np.arange(len(v))
            return Call("mh_volume_index", [CTX, B("voxels", In(v)), len(v), i32(dims),
                                            B("index", Out(len(index), np.int32)), B("status", Out(2, np.int32)), STREAM],
                        {"index": index, "status": i32([0, 0])})

        @case("F", "mh_volume_match", _id)
        def _(dims=_dims, n=_nv):
            import hair_volume_np as hv
            from monohair_amd import hairvolume
            from test_hair_volume_gpu import PAIRS, _volume

            q, qo = _volume(dims, 1, min(max(n - 2, 1), int(np.prod(dims)) - 2))
            q, qo = (q[:n], qo[:n]) if n < 3 else (q, qo)
            t, to = _volume(dims, 2, 20)
            reach, cos2 = hairvolume.threshold_bounds(PAIRS)
            key = (t[:, 0] * dims[1] + t[:, 1]) * dims[2] + t[:, 2]
            index = np.full(int(np.prod(dims)), -1, np.int32)
            index[key] = np.arange(len(t))
            return Call("mh_volume_match", [CTX, B("q_voxels", In(q)), B("q_ori", In(qo)), len(q), B("t_index", In(index)),
                                            B("t_ori", In(to)), i32(dims), i32(reach), f64(cos2), len(reach),
                                            B("out_flags", Out(len(q), np.uint8)), STREAM],
                        {"out_flags": hv.match_flags(q, qo, t, to, dims, reach, cos2)})


# ---- inner fill
def _fill_lists(dims):
    """disjoint exterior and domain voxel lists of a small grid, exterior directions with the rows that are no source"""
    rng = np.random.default_rng(sum(dims))
    total = int(np.prod(dims))
    keys = rng.permutation(total)
    ek, dk = np.sort(keys[:total // 5]), np.sort(keys[total // 5:total // 5 + total // 2])
    vox = lambda k: np.stack([k // (dims[1] * dims[2]), (k // dims[2]) % dims[1], k % dims[2]], 1).astype(np.int64)   # noqa: E731
    eo = rng.normal(size=(len(ek), 3)).astype(np.float32)
    eo[0], eo[1] = 0.0, np.nan
    return vox(ek), eo, vox(dk)


for _dims in F_GRIDS:
    _id = "%dx%dx%d" % _dims

    @case("F", "mh_inner_votes", _id)
    def _(dims=_dims):
        import hair_fill_np as hf

        p = _pm(False, 3)
        rng = np.random.default_rng(1)
        bust = p.views.depth.copy()
        bust[rng.random(bust.shape) < 0.5] = 255
        vmin, vs = f64([-0.06, -0.1, -0.1]), 0.03
        pts = hf.centres(hf.grid_voxels(dims), vmin, vs)
        want = hf.votes(p.views.cams, p.views.depth, p.views.mask, bust, pts)
        assert (want[:, 0] > 0).any()
        return Call("mh_inner_votes", [CTX, B("bust", In(bust)), vmin, vs, i32(dims),
                                       B("counts", Out((len(pts), 4), np.int32)), STREAM], {"counts": want}, ctx=p.ctx)

    for _ext in (True, False):
        @case("F", "mh_inner_domain", _id + ("" if _ext else "-no-exterior"))
        def _(dims=_dims, ext=_ext):
            import hair_fill_np as hf

            nvox = int(np.prod(dims))
            counts = np.random.default_rng(nvox).integers(0, 4, (nvox, 4)).astype(np.int32)
            ev = _fill_lists(dims)[0]
            index = np.full(nvox, -1, np.int32)
            index[(ev[:, 0] * dims[1] + ev[:, 1]) * dims[2] + ev[:, 2]] = np.arange(len(ev))
            dom = hf.domain(counts, dims, ev if ext else None, max_bad=1)
            flags = np.zeros(nvox, np.uint8)
            flags[(dom[:, 0] * dims[1] + dom[:, 1]) * dims[2] + dom[:, 2]] = 1
            return Call("mh_inner_domain", [CTX, B("counts", In(counts)), B("ext_index", In(index)) if ext else None, i32(dims), 1,
                                            B("flags", Out(nvox, np.uint8)), STREAM], {"flags": flags})

    for _sweeps in (0, 1, 4):
        @case("F", "mh_inner_diffuse", "%s-sweeps%d" % (_id, _sweeps))
        def _(dims=_dims, sweeps=_sweeps):
            import hair_fill_np as hf

            ev, eo, dv = _fill_lists(dims)
            G, D, nvox = len(ev), len(dv), int(np.prod(dims))
            T, known, depth = hf.diffuse(ev, eo, dv, dims, sweeps)
            ext_t, src = hf.source_tensors(eo)
            key = lambda v: (v[:, 0] * dims[1] + v[:, 1]) * dims[2] + v[:, 2]       # noqa: E731
            vmap = np.zeros(nvox, np.int32)
            vmap[key(ev)] = -(np.arange(G) + 1)
            vmap[key(dv)] = np.arange(D) + 1
            return Call("mh_inner_diffuse",
                        [CTX, B("ext_voxels", In(ev)), B("ext_ori", In(eo)), G, B("dom_voxels", In(dv)), D, i32(dims), sweeps,
                         B("map", Out(nvox, np.int32)), B("ext_tensor", Out((G, 6), np.float64)), B("ext_source", Out(G, np.uint8)),
                         B("cell", Out(D, np.int32)), B("tensor", Out((D, 6), np.float64)), B("tensor_b", Out((D, 6), np.float64)),
                         B("known", Out(D, np.uint8)), B("known_b", Out(D, np.uint8)), B("depth", Out(D, np.int32)),
                         B("status", Out(2, np.int32)), STREAM],
                        {"map": vmap, "ext_tensor": ext_t, "ext_source": src.astype(np.uint8), "cell": i32(key(dv)), "tensor": T,
                         "known": known, "depth": depth, "status": i32([0, 0])})

    @case("F", "mh_inner_resolve", _id)
    def _(dims=_dims):
        import hair_fill_np as hf

        ev, eo, dv = _fill_lists(dims)
        T, known, _ = hf.diffuse(ev, eo, dv, dims, 2)
        vmin, vs = f64([-0.32, -0.32, -0.24]), 0.0025
        ori, coh, emit = hf.resolve(T, known, 0.5)
        D = len(dv)
        return Call("mh_inner_resolve", [CTX, B("dom_voxels", In(dv)), D, B("tensor", In(T)), B("known", In(known)), vmin, vs,
                                         i32(dims), 0.5, B("world", Out((D, 3), np.float32)), B("ori", Out((D, 3), np.float32)),
                                         B("coh", Out(D, np.float64)), B("emit", Out(D, np.uint8)), STREAM],
                    {"world": hf.centres(dv, vmin, vs), "ori": ori, "coh": coh, "emit": emit})


# ============================================================================ B. neighbours and medoids
def _unit(rng, shape):
    v = rng.normal(size=shape + (3,))
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(np.float32)


for _G in (1, 3, 65):
    for _K in (1, 3, 100, 513):
        _id = "g%d-k%d" % (_G, _K)

        @case("B", "mh_medoid_dense", _id)
        def _(G=_G, K=_K):
            import oracle

            ori = _unit(np.random.default_rng(G * 1000 + K), (G, K))
            out, idx = oracle.medoid_dense(ori)
            return Call("mh_medoid_dense", [CTX, B("ori", In(ori)), G, K, B("out", Out((G, 3), np.float32)),
                                            B("out_index", Out(G, np.int32)), STREAM], {"out": out, "out_index": idx})

        @case("B", "mh_medoid_indexed", _id)
        def _(G=_G, K=_K):
            import oracle

            rng = np.random.default_rng(G * 1000 + K + 1)
            rows = _unit(rng, (700,))
            index = rng.integers(0, 700, (G, K)).astype(np.int32)
            out, idx = oracle.medoid_dense(rows[index])
            return Call("mh_medoid_indexed", [CTX, B("ori_rows", In(rows)), B("index", In(index)), G, K,
                                              B("out", Out((G, 3), np.float32)), B("out_index", Out(G, np.int32)), STREAM],
                        {"out": out, "out_index": idx})

        @case("B", "mh_medoid_segmented", _id)
        def _(G=_G, K=_K):
            import oracle

            rng = np.random.default_rng(G * 1000 + K + 2)
            sizes = rng.integers(1, K + 1, G)
            sizes[0] = K
            seg = i32(np.concatenate([[0], np.cumsum(sizes)]))
            ori = _unit(rng, (int(seg[-1]),))
            out, idx = oracle.medoid_segmented(ori, seg)
            return Call("mh_medoid_segmented", [CTX, B("ori", In(ori)), B("seg_start", In(seg)), G, int(sizes.max()),
                                                B("out", Out((G, 3), np.float32)), B("out_index", Out(G, np.int32)), STREAM],
                        {"out": out, "out_index": idx})


for _n in (1, 65):
    @case("B", "mh_replace_dissimilar", "n%d" % _n)
    def _(n=_n):
        import oracle

        rng = np.random.default_rng(n)
        center, ori = _unit(rng, (n,)), _unit(rng, (n,))
        ori[::2] = center[::2] + np.float32(0.05) * ori[::2]          # half of the rows stay
        want = ori.copy()
        oracle.replace_dissimilar(center, want, 0.95)
        return Call("mh_replace_dissimilar", [CTX, B("center", In(center)), B("ori", InOut(ori)), 0.95, n, STREAM], {"ori": want})

    for _with in (True, False):
        @case("B", "mh_refine_combine", "n%d%s" % (_n, "" if _with else "-no-ori"))
        def _(n=_n, with_ori=_with):
            import oracle

            rng = np.random.default_rng(n + 9)
            center, ori = _unit(rng, (n,)), _unit(rng, (n,))
            ori[::2] = center[::2] + np.float32(0.05) * ori[::2]
            loss_u = rng.random(n).astype(np.float32)
            loss_u[::5], loss_u[3::7] = -1.0, np.nan
            head, top = (rng.random(n) < 0.5).astype(np.uint8), (rng.random(n) < 0.5).astype(np.uint8)
            upd = np.where((head != 0) & (top == 0), np.float32(-1.0), loss_u)
            exp = {"loss_out": np.where(upd == -1, np.float32(0.5), upd).astype(np.float32)}
            if with_ori:
                exp["ori"] = ori.copy()
                oracle.replace_dissimilar(center, exp["ori"], 0.95)
            return Call("mh_refine_combine", [CTX, B("center", In(center)), B("loss_u", In(loss_u)), B("head_filter", In(head)),
                                              B("head_top", In(top)), 0.95, B("ori", InOut(ori)) if with_ori else None,
                                              B("loss_out", Out(n, np.float32)), n, STREAM], exp)

    for _drop in (None, "out_dist", "out_mask"):
        @case("B", "mh_nearest_distance", "n%d%s" % (_n, "-no-" + _drop if _drop else ""))
        def _(n=_n, drop=_drop):
            from scipy.spatial import KDTree

            import refine_edge_cases as rc

            rng = np.random.default_rng(n + 4)
            pts = rng.uniform(-0.1, 0.1, (n, 3)).astype(np.float32)
            ref = rng.uniform(-0.1, 0.1, (77, 3))
            L = 0.02
            d, _ = KDTree(data=ref).query(pts.astype(np.float64), k=1)
            exp = {"out_dist": f64(d), "out_mask": rc.head_top_rule(d, pts[:, 2], L).astype(np.uint8)}
            outs = [None if k == drop else B(k, Out(n, e.dtype)) for k, e in exp.items()]
            exp.pop(drop, None)
            return Call("mh_nearest_distance", [CTX, B("points", In(pts)), n, B("ref_points", In(ref)), 77, outs[0], 0.04, L,
                                                outs[1], STREAM], exp)

    for _k in (1, 8, 100):
        @case("B", "mh_knn_grid", "q%d-k%d" % (_n, _k))
        def _(Q=_n, k=_k):
            from scipy.spatial import KDTree

            rng = np.random.default_rng(Q + k)
            pts = rng.uniform(0.0, 0.1, (3000, 3)).astype(np.float32)
            grid, dims = f32([0.0, 0.0, 0.0, 0.0125]), i32([8, 8, 8])
            c = np.clip(np.floor((pts - grid[:3]) / grid[3]), 0, dims.astype(np.float32) - 1).astype(np.int64)
            key = (c[:, 2] * 8 + c[:, 1]) * 8 + c[:, 0]
            order = np.argsort(key, kind="stable")
            cstart = i32(np.searchsorted(key[order], np.arange(513)))
            q = rng.uniform(0.02, 0.08, (Q, 3)).astype(np.float32)
            _, want = KDTree(data=pts.astype(np.float64)).query(q.astype(np.float64), k=k)
            return Call("mh_knn_grid", [CTX, grid, dims, B("pts_sorted", In(pts[order])), B("order", In(i32(order))),
                                        B("cell_start", In(cstart)), B("queries", In(q)), 0, Q, k, 1, None, None,
                                        B("out_idx", Out((Q, k), np.int32)), B("status", Out(Q, np.int32)), STREAM],
                        {"out_idx": i32(want).reshape(Q, k), "status": i32(np.zeros(Q))})


# ============================================================================ E. hair stage
_long_cache = {}


def _long():
    """tests/golden/strands_long.npz as tests/test_hairgrow_gpu.py's long_setup builds it: occ [Z,H,W], ori [Z,H,W,3], the
    oracle's volume"""
    import os

    import oracle
    from conftest import GOLDEN

    if not _long_cache:
        z = np.load(os.path.join(GOLDEN, "strands_long.npz"))
        G = tuple(int(g) for g in z["trace_shape"])
        occ = np.zeros(G, np.float32)
        occ[tuple(z["trace_occ_nz"].T.astype(np.int64))] = 1
        ori = np.zeros(G + (3,), np.float32)
        ori[tuple(z["trace_ori_nz"].T.astype(np.int64))] = z["trace_ori_nz_val"]
        occ, ori = f32(occ.transpose(2, 1, 0)), f32(ori.transpose(2, 1, 0, 3))
        _long_cache.update(z=z, occ=occ, ori=ori, vol=oracle.Volume(occ, ori))
    return _long_cache


def _rows(values, first, length, stride):
    """rows of `stride` points of which only [first, first + len) is written"""
    m = np.ma.MaskedArray(np.zeros((len(first), stride, 3), np.float32), True)
    for i, (f, l) in enumerate(zip(first, length)):
        m[i, f:f + l] = values[i, f:f + l]
    return m


@case("E", "mh_volume_pack", "long")
def _():
    g = _long()
    Z, H, W = g["occ"].shape
    return Call("mh_volume_pack", [CTX, B("occ", In(g["occ"])), B("ori", In(g["ori"])), W, H, Z,
                                   B("vox", Out((Z, H, W, 4), np.float32)), STREAM], {"vox": f32(g["vol"].vox)})


for _n in (1, 65, 257):
    @case("E", "mh_trace_seeds", "n%d" % _n)
    def _(n=_n):
        import oracle

        g = _long()
        z, vol = g["z"], g["vol"]
        Z, H, W = g["occ"].shape
        long_ = np.flatnonzero(z["trace_len"] == 513)[:1]               # a walk at both caps: slots 0 and 512 of its row
        sel = np.resize(np.concatenate([long_, np.setdiff1d(np.arange(len(z["trace_seeds"])), long_)]), n)   # (88 seeds, repeated)
        seeds, thr = f32(z["trace_seeds"][sel]), float(z["grow_thr"])
        o_out, o_first, o_ln = oracle.trace_seeds(vol, seeds, thr)
        assert o_ln[0] == 513
        return Call("mh_trace_seeds", [CTX, B("vox", In(f32(vol.vox))), W, H, Z, B("seeds", In(seeds)), n, thr,
                                       B("out", Out((n, 513, 3), np.float32)), B("first", Out(n, np.int32)),
                                       B("len", Out(n, np.int32)), STREAM],
                    {"out": _rows(o_out, o_first, o_ln, 513), "first": i32(o_first), "len": i32(o_ln)})

    @case("E", "mh_trace_scalp", "n%d" % _n)
    def _(n=_n):
        import oracle

        g = _long()
        z, vol = g["z"], g["vol"]
        Z, H, W = g["occ"].shape
        first = np.concatenate([np.flatnonzero(z["scalp_len"] == 257)[:1], np.flatnonzero(z["scalp_len"] == 0)[:1]])
        sel = np.resize(np.concatenate([first, np.setdiff1d(np.arange(len(z["scalp_len"])), first)]), n)     # (repeated to n)
        sp, sn, thr = f32(z["scalp_points"][sel]), f32(z["scalp_normals"][sel]), float(z["grow_thr"])
        o_sp, o_sl = oracle.trace_scalp(vol, sp, sn, thr)
        # a walk that is rejected (len 0) leaves the points it took in its row: exactly 26, the seed and 25 steps (it is rejected
        # when it is still inside the head after 25 steps); the oracle does not return them, so they are held to be the same
        # for both fills
        free = np.zeros((n, 257, 3), bool)
        free[o_sl == 0, :26] = True
        return Call("mh_trace_scalp", [CTX, B("vox", In(f32(vol.vox))), W, H, Z, B("seeds", In(sp)), B("normals", In(sn)), n, thr,
                                       B("out", Out((n, 257, 3), np.float32)), B("len", Out(n, np.int32)), STREAM],
                    {"out": Partial(_rows(o_sp, np.zeros(n, np.int64), o_sl, 257), free, same=True), "len": i32(o_sl)})

    for _first in (True, False):
        @case("E", "mh_strands_compact", "n%d%s" % (_n, "" if _first else "-no-first"))
        def _(n=_n, with_first=_first):
            rng = np.random.default_rng(n)
            stride = 33
            rows = rng.normal(size=(n, stride, 3)).astype(np.float32)
            first = rng.integers(0, 10, n).astype(np.int32) if with_first else np.zeros(n, np.int32)
            ln = rng.integers(0, stride - 10, n).astype(np.int32)
            offs = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
            want = np.concatenate([rows[i, first[i]:first[i] + ln[i]] for i in range(n)] + [np.zeros((0, 3), np.float32)])
            total = max(int(offs[-1]), 1)
            return Call("mh_strands_compact", [CTX, B("rows", In(rows)), B("first", In(first)) if with_first else None,
                                               B("len", In(ln)), B("offsets", In(offs[:n])), n, stride,
                                               B("packed", Out((total, 3), np.float32)), STREAM],
                        {"packed": head(want, total)})


def _mesh(n):
    from test_mesh_sample_gpu import BUST, np_sample, random_mesh

    rng = np.random.default_rng(200 + n)
    v, f, vn = random_mesh(rng, 60, 41, zero_area_at=(17,))
    u = rng.random((n, 2))
    u[0] = [0.0, np.nextafter(1.0, 0.0)]
    return v, i32(f), vn, u, f64(BUST), np_sample(v, vn, f, u, f64(BUST))


@case("E", "mh_tri_area64", "nf41")
def _():
    v, f, vn, u, bust, (area, bounds, tri, p, q) = _mesh(65)
    return Call("mh_tri_area64", [CTX, B("vertices", In(v)), len(v), B("faces", In(f)), len(f),
                                  B("area", Out(len(f), np.float64)), STREAM], {"area": area})


for _n in (1, 65, 257):
    for _tri in (True, False):
        @case("E", "mh_mesh_sample", "n%d%s" % (_n, "" if _tri else "-no-triangle"))
        def _(n=_n, with_tri=_tri):
            v, f, vn, u, bust, (area, bounds, tri, p, q) = _mesh(n)
            exp = {"out_points": p, "out_normals": q}
            if with_tri:
                exp["out_triangle"] = i32(tri)
            return Call("mh_mesh_sample", [CTX, B("vertices", In(v)), B("normals", In(vn)), len(v), B("faces", In(f)), len(f),
                                           B("bounds", In(i64(bounds))), B("uniforms", In(u)), n, bust,
                                           B("out_points", Out((n, 3), np.float32)), B("out_normals", Out((n, 3), np.float32)),
                                           B("out_triangle", Out(n, np.int32)) if with_tri else None, STREAM], exp)


_diffuse_cache = {}


def _diffuse(n):
    """tests/test_scalp_diffusion_gpu.py's small volume with n samples (a seed at which some walk is accepted) and the
    restatement's every intermediate"""
    import scalp_diffusion_np as rs
    from test_scalp_diffusion_gpu import small_volume

    if n not in _diffuse_cache:
        for seed in range(n, n + 40):
            pts, nrm, ori, occ = small_volume(seed, n)
            ro, rc, det = rs.diffusion_scalp(pts, nrm, ori, occ)
            if (det["status"] == rs.ACCEPTED).any():
                break
        _diffuse_cache[n] = (pts, nrm, ori, occ, ro, rc, det)
    return _diffuse_cache[n]


def _diffuse_rows(n):
    pts, nrm, ori, occ, ro, rc, det = _diffuse(n)
    Z, H, W = occ.shape[1:]
    rows = np.where(det["status"] == 0, det["step"].astype(np.int64) + 1, 0)
    offs = i64(np.concatenate([[0], np.cumsum(rows)]))
    vox = det["voxel"]
    keys = np.where((vox >= 0).all(1), (vox[:, 2] * H + vox[:, 1]) * W + vox[:, 0], W * H * Z).astype(np.uint64)
    return offs, int(offs[-1]), keys


for _n in (1, 65, 257):
    @case("E", "mh_diffuse_walk", "n%d" % _n)
    def _(n=_n):
        pts, nrm, ori, occ, ro, rc, det = _diffuse(n)
        Z, H, W = occ.shape[1:]
        return Call("mh_diffuse_walk", [CTX, B("occ", In(occ[0])), B("ori", In(ori)), W, H, Z, B("points", In(pts)),
                                        B("normals", In(nrm)), n, B("status", Out(n, np.int32)), B("steps", Out(n, np.int32)),
                                        B("end_points", Out((n, 3), np.float32)), B("first_normals", Out((n, 3), np.float32)),
                                        B("last_normals", Out((n, 3), np.float32)), STREAM],
                    {"status": det["status"], "steps": det["step"], "end_points": det["end_point"],
                     "first_normals": det["first_normal"], "last_normals": det["last_normal"]})

    @case("E", "mh_diffuse_arc", "n%d" % _n)
    def _(n=_n):
        pts, nrm, ori, occ, ro, rc, det = _diffuse(n)
        Z, H, W = occ.shape[1:]
        offs, R, keys = _diffuse_rows(n)
        return Call("mh_diffuse_arc", [CTX, B("points", In(pts)), B("end_points", In(det["end_point"])),
                                       B("first_normals", In(det["first_normal"])), B("last_normals", In(det["last_normal"])),
                                       B("steps", In(det["step"])), B("row_offsets", In(offs)), n, R, W, H, Z,
                                       B("sample", Out((R, 3), np.float64)), B("tangent", Out((R, 3), np.float64)),
                                       B("unit", Out((R, 3), np.float64)), B("voxel", Out((R, 3), np.int32)),
                                       B("keys", Out(R, np.uint64)), STREAM],
                    {"sample": det["total_sample"], "tangent": det["total_normal"], "unit": det["total_normal_unit"],
                     "voxel": i32(det["voxel"]), "keys": keys})

    @case("E", "mh_diffuse_splat", "n%d" % _n)
    def _(n=_n):
        pts, nrm, ori, occ, ro, rc, det = _diffuse(n)
        Z, H, W = occ.shape[1:]
        offs, R, keys = _diffuse_rows(n)
        order = np.argsort(keys, kind="stable")
        sk = keys[order]
        starts = np.flatnonzero(np.concatenate([[True], sk[1:] != sk[:-1]]))
        seg = np.full(R + 1, -1, np.int32)              # capacity R + 1, G + 1 entries in use
        seg[:len(starts) + 1] = np.concatenate([starts, [R]])
        heads = np.zeros(R, np.uint64)
        heads[:len(starts)] = sk[starts]
        meta = i32([len(starts), np.diff(np.concatenate([starts, [R]])).max()])
        # the whole volumes go in and come back: a voxel no row touches keeps its bytes
        return Call("mh_diffuse_splat", [CTX, B("seg_start", In(seg)), B("head_keys", In(heads)), B("meta", In(meta)),
                                         B("order", In(i32(order))), B("unit", In(det["total_normal_unit"])), R, W, H, Z,
                                         B("occ", InOut(occ[0])), B("ori", InOut(ori)), STREAM], {"occ": rc[0], "ori": ro})


# ---- segment connection (HairGrowing.find_connect_info), against the restatement of tests/test_hair_connect_gpu.py
CONNECT_THR, CONNECT_DOT = 0.005, 0.7
_connect_cache = {}


def _connect(n):
    """n segments of the seeded sweep of tests/test_hair_connect_gpu.py (short ones, long arcs with the partners laid along
    their ends), their end grid as HairGrowing._end_tables bins it, and the restatement's lists, joins and chains"""
    from monohair_amd.hairgrow import grid_dims
    from test_hair_connect_gpu import _np_lists, _rs_chain, _rs_table, _stats, _sweep_segments

    if n in _connect_cache:
        return _connect_cache[n]
    if "segs" not in _connect_cache:
        _connect_cache["segs"] = _sweep_segments(np.random.default_rng(2024), 0)
    allsegs = _connect_cache["segs"]
    segs = {1: allsegs[300:301], 65: allsegs[280:345], 257: allsegs[150:407]}[n]
    assert len(segs) == n
    pts = f64(np.concatenate(segs))
    offs = _offsets([len(s) for s in segs])
    ends = np.concatenate([pts[offs[:-1]], pts[offs[1:] - 1]], 0)             # roots, then tips
    lo = ends.min(0)
    h, dims = grid_dims(ends.max(0) - lo, CONNECT_THR, 1.0001, 2 * n)
    cells = np.floor((ends - lo) / h).astype(np.int32)
    lin = (cells[:, 2].astype(np.int64) * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
    ncell = dims[0] * dims[1] * dims[2]
    trees = []
    for t in range(2):          # 0: the roots' tree, 1: the tips'
        l = lin[t * n:(t + 1) * n]
        cstart = np.zeros(ncell + 1, np.int32)
        np.cumsum(np.bincount(l, minlength=ncell), out=cstart[1:])
        trees.append(dict(order=i32(np.argsort(l, kind="stable")), cstart=cstart, ends=f64(ends[t * n:(t + 1) * n]),
                          cells=i32(cells[t * n:(t + 1) * n])))
    lists = _np_lists(segs, CONNECT_THR)
    table = _rs_table(segs, lists, CONNECT_DOT, _stats())
    chains = [_rs_chain(segs, table, i) for i in range(n)]
    _connect_cache[n] = dict(segs=segs, pts=pts, offs=offs, dims=dims, trees=trees, lists=lists, table=table, chains=chains)
    return _connect_cache[n]


def _list_arrays(rows):
    """the [N,50] tables of one end list: index, distance, count (the rest of a row is not read)"""
    n = len(rows)
    idx, dist, cnt = np.full((n, 50), -1, np.int32), np.full((n, 50), np.inf), np.zeros(n, np.int32)
    for i, (c, d) in enumerate(rows):
        idx[i, :len(c)], dist[i, :len(c)], cnt[i] = c, d, len(c)
    return idx, dist, cnt


for _n in (1, 65, 257):
    for _k, (_qe, _te) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        @case("E", "mh_end_knn64", "n%d-%s-%s" % (_n, ("roots", "tips")[_qe], ("roots", "tips")[_te]))
        def _(n=_n, k=_k, qe=_qe, te=_te):
            c = _connect(n)
            q, t = c["trees"][qe], c["trees"][te]
            idx, dist, cnt = _list_arrays(c["lists"][k])
            used = np.arange(50)[None, :] < cnt[:, None]
            # (the header does not say what a row holds behind its count: compared with nothing)
            return Call("mh_end_knn64", [CTX, B("q", In(q["ends"])), B("qcell", In(q["cells"])), n, B("data", In(t["ends"])),
                                         B("order", In(t["order"])), B("cstart", In(t["cstart"])), c["dims"][0], c["dims"][1],
                                         c["dims"][2], CONNECT_THR, 1, B("out_idx", Out((n, 50), np.int32)),
                                         B("out_dist", Out((n, 50), np.float64)), B("out_cnt", Out(n, np.int32)), STREAM],
                        {"out_idx": Partial(np.ma.MaskedArray(idx, ~used), ~used),
                         "out_dist": Partial(np.ma.MaskedArray(dist, ~used), ~used), "out_cnt": cnt})

    @case("E", "mh_connect_candidates", "n%d" % _n)
    def _(n=_n):
        c = _connect(n)
        extra = {}
        for k in range(4):
            idx, dist, cnt = _list_arrays(c["lists"][k])
            extra.update({"idx%d" % k: In(idx), "dist%d" % k: In(dist), "cnt%d" % k: In(cnt)})
        call = Call("mh_connect_candidates", [CTX, B("pts", In(c["pts"])), B("offsets", In(c["offs"])), n,
                                              PtrArray(["idx%d" % k for k in range(4)]), PtrArray(["dist%d" % k for k in range(4)]),
                                              PtrArray(["cnt%d" % k for k in range(4)]), CONNECT_DOT,
                                              B("best", Out(2 * n, np.int32)), B("best_type", Out(2 * n, np.int32)), STREAM],
                    {"best": i32(c["table"][..., 0].reshape(-1)), "best_type": i32(c["table"][..., 1].reshape(-1))})
        call.extra = extra
        return call

    def _chain_count(n):
        c = _connect(n)
        return Call("mh_chain_count", [CTX, B("offsets", In(c["offs"])), n, B("best", In(i32(c["table"][..., 0].reshape(-1)))),
                                       B("best_type", In(i32(c["table"][..., 1].reshape(-1)))), B("total", Out(n, np.int64)),
                                       B("root_len", Out(n, np.int64)), STREAM], {"total": i64([len(s) for s in c["chains"]])})

    @case("E", "mh_chain_count", "n%d" % _n)
    def _(n=_n):
        return _chain_count(n)

    @case("E", "mh_chain_emit", "n%d" % _n)
    def _(n=_n):
        c = _connect(n)
        total = i64([len(s) for s in c["chains"]])
        out = f64(np.concatenate(c["chains"]))
        # root_len comes from mh_chain_count on the same arena (the restatement builds a chain in one piece)
        return Call("mh_chain_emit", [CTX, B("pts", In(c["pts"])), B("offsets", In(c["offs"])), n,
                                      B("best", In(i32(c["table"][..., 0].reshape(-1)))),
                                      B("best_type", In(i32(c["table"][..., 1].reshape(-1)))), B("root_len", Out(n, np.int64)),
                                      B("out_offsets", In(_offsets(total)[:n])), B("out", Out(out.shape, np.float64)), STREAM],
                    {"out": out, "total": total}, before=[_chain_count(n)])


for _n in (1, 65):
    @case("E", "mh_occ_check", "n%d" % _n)
    def _(n=_n):
        from test_hair_connect_gpu import _rs_occupancy, _stats

        c = _connect(n)
        occ = (np.random.default_rng(n).random((192, 256, 256)) < 0.85).astype(np.float32)
        chains = [s.copy() for s in c["chains"]]
        chains[-1] = chains[-1] + np.array([0.4, 0.0, 0.0])        # leaves the 256-voxel box: status 2
        want = []
        for s in chains:          # attempt 0 of the restatement's loop: accepted at once, outside the box, or rejected
            st = _stats()
            np.random.seed(0)
            got, ok = _rs_occupancy(s, occ, st)
            idx = np.rint((s * np.array([1.0, -1.0, -1.0]) - np.array([-0.32, -0.32, -0.24], np.float32).astype(np.float64))
                          / 0.0025).astype(np.int64)
            outside = idx[:, 2].max() >= 192 or (idx[:, 1] >= 256).any() or (idx[:, 0] >= 256).any()
            want.append(2 if outside else (1 if ok and st["retried_ok"] == 0 else 0))
        assert 2 in want and (n == 1 or (0 in want and 1 in want))
        vmin = np.array([-0.32, -0.32, -0.24], np.float32).astype(np.float64)
        return Call("mh_occ_check", [CTX, B("pts", In(f64(np.concatenate(chains)))), B("offsets", In(_offsets([len(s) for s in chains]))),
                                     n, B("occ", In(occ)), ctypes.c_longlong(1), 256, 256, 192, float(vmin[0]), float(vmin[1]),
                                     float(vmin[2]), 0.0025, B("status", Out(n, np.int32)), STREAM], {"status": i32(want)})


@case("E", "mh_smooth_strands", "1-2-3-65-points")
def _():
    from test_hair_connect_gpu import _np_smooth

    rng = np.random.default_rng(8)
    lens, lap, pos = [1, 2, 3, 65, 1], 4.0, 2.0
    strands = [np.cumsum(rng.normal(0, 0.002, (L, 3)), 0).astype(np.float32) for L in lens]
    rhs = f64(np.concatenate([s * np.float32(pos) for s in strands]))        # b = strand * pos in the strand's own dtype
    offs = _offsets(lens)

    def check(outs):
        got = outs["pts"]
        for i, s in enumerate(strands):
            g = got[offs[i]:offs[i + 1]]
            if len(s) < 2:          # a strand of one point is left untouched
                assert g.tobytes() == rhs[offs[i]:offs[i + 1]].tobytes(), i
                continue
            # as tests/test_hair_connect_gpu.py: within 1 float32 ulp of scipy's solveh_banded
            ref = _np_smooth(s.astype(np.float64), lap, pos).astype(np.float32)
            ulp = np.abs(g.astype(np.float32).view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64))
            assert ulp.max() <= 1, (i, int(ulp.max()))
    return Call("mh_smooth_strands", [CTX, B("pts", InOut(rhs)), B("offsets", In(offs)), len(lens), lap, pos,
                                      B("work", Scratch(3 * len(rhs) * 8)), STREAM], {"pts": check})


# ============================================================================ G. exchange (one rank, the real collective library)
def _comm():
    from monohair_amd import dist as mdist

    return mdist.rccl_comm("cuda:0")


for _mode in (0, 1):
    @case("G", "mh_volume_reduce", "one-rank-mode%d" % _mode)
    def _(mode=_mode):
        ctx, comm = _comm()
        X, Y, Z, C = 5, 3, 7, 4
        vol = np.random.default_rng(mode).random((X, Y, Z, C)).astype(np.float32)
        return Call("mh_volume_reduce", [CTX, comm, 0, 1, 0, B("volume", InOut(vol)), X, Y, Z, C, i32([0, X]), mode, STREAM],
                    {"volume": vol}, ctx=ctx)           # one rank owns everything: the volume is unchanged


@case("G", "mh_volume_gather", "one-rank")
def _():
    ctx, comm = _comm()
    X, Y, Z, C = 5, 3, 7, 4
    slab = np.random.default_rng(3).random((X, Y, Z, C)).astype(np.float32)
    return Call("mh_volume_gather", [CTX, comm, 0, 1, 0, B("slab", In(slab)), B("volume", Out((X, Y, Z, C), np.float32)), X, Y, Z,
                                     C, i32([0, X]), STREAM], {"volume": slab}, ctx=ctx)


# ---- scalp attachment: ONE pass of connect_to_scalp against rs_pass of tests/test_hair_scalp_host.py
SCALP_THR_DIST, SCALP_THR_DOT, SCALP_RATIO = 1.25, 0.675, 0.1        # the fourth pass's thresholds: joins and flips happen
_scalp_cache = {}


def _scalp(which):
    """the seeded strands of tests/test_hair_scalp_gpu.py ("sweep": all of them; "one": the rooted ones and one floating
    strand), the inputs of a pass as HairGrowing._scalp_core / _scalp_grid build them, and the state after rs_pass"""
    import collections
    import os

    from scipy.spatial import KDTree

    from conftest import GOLDEN
    from monohair_amd.hairgrow import grid_dims
    from test_hair_scalp_gpu import _sweep_strands
    from test_hair_scalp_host import ball_by_rank, load_volume, rs_pass

    if which in _scalp_cache:
        return _scalp_cache[which]
    if "vox" not in _scalp_cache:
        _scalp_cache["vox"] = load_volume(np.load(os.path.join(GOLDEN, "hair_connect.npz")))[2]
        _scalp_cache["vox_dev"] = Outside(_scalp_cache["vox"])
    vox = _scalp_cache["vox"]
    strands, num_root = _sweep_strands(np.random.default_rng(77))
    if which == "one":
        strands = strands[:num_root] + strands[num_root + 5:num_root + 6]
    strands = [np.ascontiguousarray(x, np.float32) for x in strands]
    n = len(strands)
    pts, offs = f32(np.concatenate(strands)), _offsets([len(x) for x in strands])
    active = i32(np.arange(num_root, n))
    core = f32(np.concatenate(strands[:num_root]))
    sid = i32(np.repeat(np.arange(num_root), [len(x) for x in strands[:num_root]]))
    rank = np.empty(len(core), np.int32)
    rank[KDTree(core).indices] = np.arange(len(core), dtype=np.int32)
    lo, hi = core.min(0), core.max(0)
    h, dims = grid_dims((hi - lo).astype(np.float64), SCALP_THR_DIST, 1.01, len(core))
    grid, dims = f32([lo[0], lo[1], lo[2], h]), i32(dims)
    c = np.clip(np.floor((core - grid[:3]) / grid[3]), 0, dims.astype(np.float32) - 1).astype(np.int64)       # in float32
    key = (c[:, 2] * int(dims[1]) + c[:, 1]) * int(dims[0]) + c[:, 0]
    order = np.argsort(key, kind="stable")
    cstart = i32(np.searchsorted(key[order], np.arange(int(np.prod(dims)) + 1)))
    counts = i64([len(ball_by_rank(core.astype(np.float64), rank, strands[a][0], SCALP_THR_DIST)) for a in active])
    # the pass, restated
    state = dict(strands=[x.copy() for x in strands], root=np.arange(n) < num_root, out=np.zeros(n, bool),
                 out_ratio=np.zeros(n), flips=np.zeros(n, np.int32), choice=np.full((n, 2), -1, np.int32),
                 sims=np.zeros(n, np.float32))
    stats = collections.defaultdict(int)
    new_root = rs_pass(state["strands"], state["root"], state["out"], state["out_ratio"], state["flips"], state["choice"],
                       state["sims"], vox, SCALP_THR_DIST, SCALP_THR_DOT, SCALP_RATIO, stats)
    for k in ("nearest_ties", "loss_ties", "similar_near_0.3", "mean_near_5", "dist_near_thr"):
        assert stats[k] == 0, k                       # no exact tie, no decision within rounding of its threshold
    _scalp_cache[which] = dict(n=n, num_root=num_root, pts=pts, offs=offs, active=active, core=core, sid=sid, rank=rank,
                               grid=grid, dims=dims, order=i32(order), cstart=cstart, counts=counts, state=state,
                               new_root=new_root, new_out=int(state["out"].sum()), vox=_scalp_cache["vox_dev"],
                               vox_shape=vox.shape)
    return _scalp_cache[which]


for _which in ("sweep", "one"):
    @case("E", "mh_scalp_ball_count", _which)
    def _(which=_which):
        d = _scalp(which)
        assert which == "one" or (d["counts"] > 64).any()
        return Call("mh_scalp_ball_count",
                    [CTX, B("pts", In(d["pts"])), B("offsets", In(d["offs"])), B("active", In(d["active"])), len(d["active"]),
                     B("core", In(d["core"])), len(d["core"]), B("order", In(d["order"])), B("cell_start", In(d["cstart"])),
                     d["grid"], d["dims"], SCALP_THR_DIST, B("count", Out(len(d["active"]), np.int64)), STREAM],
                    {"count": d["counts"]})

    @case("E", "mh_scalp_choose", _which)
    def _(which=_which):
        d = _scalp(which)
        n, st = d["n"], d["state"]
        joined = st["choice"][:, 0] >= 0
        assert which == "one" or (joined.any() and st["flips"].any())

        def check(outs):
            assert np.array_equal(outs["flip"], st["flips"].astype(np.uint8))
            assert np.array_equal(outs["best_strand"], st["choice"][:, 0])
            assert np.array_equal(outs["best_index"][joined], st["choice"][joined, 1])      # (read where a strand is joined)
            rooted = np.arange(n) < d["num_root"]              # the caller's presets of the strands that are not active stay
            assert (outs["best_index"][rooted] == 0).all()
        boffs = _offsets(d["counts"])
        return Call("mh_scalp_choose",
                    [CTX, B("pts", In(d["pts"])), B("offsets", In(d["offs"])), B("active", In(d["active"])), len(d["active"]),
                     B("core", In(d["core"])), B("core_strand", In(d["sid"])), B("core_rank", In(d["rank"])), len(d["core"]),
                     B("order", In(d["order"])), B("cell_start", In(d["cstart"])), d["grid"], d["dims"], SCALP_THR_DIST,
                     SCALP_THR_DOT, B("out_ratio", In(np.zeros(n))), B("ball_offsets", In(boffs)),
                     B("ball_scratch", Scratch(8 * max(int(boffs[-1]), 1))), B("flip", InOut(np.zeros(n, np.uint8))),
                     B("best_strand", InOut(np.full(n, -1, np.int32))), B("best_index", InOut(np.zeros(n, np.int32))), STREAM],
                    {"flip": check})

    @case("E", "mh_scalp_emit", _which)
    def _(which=_which):
        from test_hair_scalp_host import similar_close

        d = _scalp(which)
        n, st = d["n"], d["state"]
        joined = st["choice"][:, 0] >= 0
        bidx = i32(np.where(joined, st["choice"][:, 1], 0))
        new = f32(np.concatenate(st["strands"]))
        noffs = _offsets([len(x) for x in st["strands"]])
        assert np.array_equal(np.diff(noffs), np.diff(d["offs"]) + np.where(joined, bidx.astype(np.int64) + 1, 0))
        flags0 = (np.arange(n) < d["num_root"]).astype(np.uint8)
        Z, H, W = d["vox_shape"][:3]

        def check(outs):
            assert similar_close(outs["similar"][joined], st["sims"][joined])      # as tests/test_hair_scalp_gpu.py holds it
            assert (outs["similar"][~joined] == 0).all()
        return Call("mh_scalp_emit",
                    [CTX, B("pts", In(d["pts"])), B("offsets", In(d["offs"])), n, B("flip", In(st["flips"].astype(np.uint8))),
                     B("best_strand", In(i32(st["choice"][:, 0]))), B("best_index", In(bidx)), B("new_offsets", In(noffs)),
                     d["vox"], W, H, Z, SCALP_RATIO, B("new_pts", Out(new.shape, np.float32)), B("flags", InOut(flags0)),
                     B("out_ratio", InOut(np.zeros(n))), B("similar", InOut(np.zeros(n, np.float32))),
                     B("counters", InOut(i32([5, 6, 7]))), STREAM],
                    {"new_pts": new, "flags": (st["root"].astype(np.uint8) | (st["out"].astype(np.uint8) << 1)),
                     "out_ratio": f64(st["out_ratio"]), "similar": check,
                     "counters": i32([5 + d["new_root"], 6 + d["new_out"], 7])})
