"""class PMVO -- the host-side mirror of the reference's `PMVO.py::class PMVO` (lines 13-529) on top of
the HIP library (include/mh_pmvo.h).  Same constructor, same methods, same return shapes/dtypes; every
method is one or two C-ABI calls on torch-owned device buffers.  There is no CPU path in here: without a
GPU and libmhpmvo.so construction fails loudly.

State set by Compute_Visible_and_Ori (as in the reference, PMVO.py:369-376): self.visible [V,N],
self.Ori [V,N,2], self.Conf [V,N], self.mask [V,N], self.Ori_patch [V,N,P,2], self.Conf_patch [V,N,P].
"""
import collections
import ctypes
import warnings
import os

import numpy as np
import torch

from . import _lib
from .camera import CAM_STRIDE, camera_records
from .timing import stage


def depth_offsets(num_sample=90):
    """The depth offsets of sample_next_3d_pos (PMVO.py:274-278): three torch.arange pieces, concatenated,
    cut to num_sample.  Built with the same CPU torch calls, so the values are the reference's bits."""
    s1 = torch.arange(-0.005, -0.001, 0.004 / (num_sample / 4))
    s2 = torch.arange(-0.001, 0.001, 0.002 / (num_sample / 2))
    s3 = torch.arange(0.001, 0.005, 0.004 / (num_sample / 4))
    return torch.cat([s1, s2, s3], 0)[:num_sample].numpy().astype(np.float32)


class PMVO:
    NUM_SAMPLE = 90          # PMVO.py:263
    RANKS = range(0, 20, 2)  # PMVO.py:50

    def __init__(self, camera, depths, Ori, Conf, masks, device="cuda:0", image_size=[1120, 1992], patch_size=5,
                 visible_threshold=1, conf_threshold=0.4):
        """camera: dict view -> Camera (insertion order = view order); depths[k] [H,W,3], Ori[k] [H,W,2],
        Conf[k] [H,W], masks[k] [H,W,3] numpy arrays (reference PMVO.py:14-28)."""
        self._init_common(device, image_size, patch_size, visible_threshold, conf_threshold)
        self.camera_dict = camera
        self.camera_key = list(camera.keys())
        self.camera = [camera[k] for k in self.camera_key]
        recs = camera_records(camera)
        H, W = int(image_size[0]), int(image_size[1])
        self._alloc(len(self.camera_key), H, W)
        st = _lib.stream_ptr()
        for i, k in enumerate(self.camera_key):
            d = torch.from_numpy(np.ascontiguousarray(np.asarray(depths[k]))).to(self.device).type(torch.float)
            o = torch.from_numpy(np.ascontiguousarray(np.asarray(Ori[k]))).to(self.device).type(torch.float)
            c = torch.from_numpy(np.ascontiguousarray(np.asarray(Conf[k]))).to(self.device).type(torch.float)
            m = torch.from_numpy(np.ascontiguousarray(np.asarray(masks[k]))).to(self.device).type(torch.float)
            assert d.shape[:2] == (H, W) and o.shape == (H, W, 2) and c.shape == (H, W) and m.shape[:2] == (H, W), \
                "map shapes do not match image_size=[H,W]"
            ds = d.shape[2] if d.dim() == 3 else 1
            ms = m.shape[2] if m.dim() == 3 else 1
            self._set_view(i, recs[i], d, ds, o, c, m, ms, st)
        torch.cuda.synchronize(self.device)

    @classmethod
    def from_planes(cls, cam_records, depth, ori, conf, mask, device="cuda:0", patch_size=5, visible_threshold=1,
                    conf_threshold=0.4, camera=None):
        """Device-resident compact planes: depth/conf/mask [V,H,W], ori [V,H,W,2] float32 tensors on `device`
        (what an on-GPU producer such as the Gabor stage hands over) + [V,48] camera records."""
        self = cls.__new__(cls)
        V, H, W = depth.shape
        self._init_common(device, [H, W], patch_size, visible_threshold, conf_threshold)
        self.camera_dict = camera
        self.camera_key = list(camera.keys()) if camera is not None else ["view_%03d" % i for i in range(V)]
        self.camera = list(camera.values()) if camera is not None else None
        recs = np.ascontiguousarray(cam_records, dtype=np.float32)
        assert recs.shape == (V, CAM_STRIDE)
        self._alloc(V, H, W)
        st = _lib.stream_ptr()
        for i in range(V):
            self._set_view(i, recs[i], depth[i].contiguous(), 1, ori[i].contiguous(), conf[i].contiguous(),
                           mask[i].contiguous(), 1, st)
        torch.cuda.synchronize(self.device)
        return self

    @classmethod
    def from_u8(cls, camera, depths, ori_u8, conf_u8, mask_u8, device="cuda:0", image_size=None, patch_size=5,
                visible_threshold=1, conf_threshold=0.4, lut=None, records=None):
        """The constructor for maps kept as their 8-bit pixel codes (pmvo_utils.load_maps_u8 or a maps pack):
        dicts view -> uint8 [H,W] for orientation / confidence / mask (or [V,H,W] arrays in view order), depth
        float32 [H,W] or [H,W,3]; numpy arrays or torch tensors (device tensors are used in place).  Decoded on the GPU through the 256-entry table of the loaders
        (pmvo_utils.map_code_lut), so the resident records equal those of PMVO(camera, <decoded float maps>).  The two codes of
        a pixel (orientation, confidence) stay resident as well, 2 B per pixel: the fused front end of forward() gathers a
        patch tap as those 2 bytes instead of a 16-byte record (option "tap_codes", default on; same results)."""
        from .pmvo_utils import map_code_lut

        self = cls.__new__(cls)
        keys = list(camera.keys())

        def get(maps, i):
            return maps[keys[i]] if isinstance(maps, dict) else maps[i]

        H, W = (int(image_size[0]), int(image_size[1])) if image_size is not None else get(ori_u8, 0).shape[:2]
        self._init_common(device, [H, W], patch_size, visible_threshold, conf_threshold)
        self.camera_dict = camera
        self.camera_key = keys
        self.camera = [camera[k] for k in keys]
        recs = camera_records(camera) if records is None else records      # (records: [V,48] override, parity tests)
        lut = np.ascontiguousarray(map_code_lut() if lut is None else lut, dtype=np.float32)
        assert lut.shape == (256, 4)
        self._alloc(len(keys), H, W)
        st = _lib.stream_ptr()
        def up(x, dtype=None):      # read-only memory maps are fine here: the tensor is only the source of a copy
            if torch.is_tensor(x):  # already on a device (Gabor stage / depth rasteriser output): no host round trip
                x = x.to(self.device)
                return (x if dtype is None else x.to(torch.float32)).contiguous()
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(self.device)

        for i in range(len(keys)):
            d = up(get(depths, i), np.float32)
            planes = [up(get(m, i)) for m in (ori_u8, conf_u8, mask_u8)]
            assert d.shape[:2] == (H, W) and all(p.dtype == torch.uint8 and p.shape == (H, W) for p in planes), \
                "map shapes/dtypes do not match image_size=[H,W] / uint8"
            rec = np.ascontiguousarray(recs[i], dtype=np.float32)
            _lib.check(self._L.mh_ctx_set_view_u8(self._ctx, i, rec.ctypes.data_as(ctypes.c_void_p), _lib.ptr(d),
                                                  d.shape[2] if d.dim() == 3 else 1, _lib.ptr(planes[0]),
                                                  _lib.ptr(planes[1]), _lib.ptr(planes[2]),
                                                  lut.ctypes.data_as(ctypes.c_void_p), st), "mh_ctx_set_view_u8")
            torch.cuda.current_stream().synchronize()      # d / planes are read asynchronously by the pack kernel
        return self

    # ------------------------------------------------------------------ plumbing
    def _init_common(self, device, image_size, patch_size, visible_threshold, conf_threshold):
        if not torch.cuda.is_available():
            raise _lib.MhError("monohair_amd.PMVO needs a ROCm GPU: the hot path has no CPU fallback")
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.MhError("monohair_amd.PMVO runs on HIP devices only (got %r)" % (device,))
        torch.cuda.set_device(self.device)
        self.image_size = [int(image_size[0]), int(image_size[1])]
        self.patch_size = int(patch_size)
        # taps run over range(-(size//2), size//2+1) in both directions (PMVO.py:494-495): an even size s gives the same
        # (s+1) x (s+1) window as s+1; the kernels are instantiated for the odd side
        self._side = 2 * (self.patch_size // 2) + 1
        self.visible_threshold = visible_threshold
        self.conf_threshold = conf_threshold
        self._stage = {}            # pinned upload rings of _upload_points, per launch stream
        self._scratch_need = {}     # N -> bytes of the search scratch (constant per context)
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._L.mh_ctx_create(self.device.index or 0, ctypes.byref(h)), "mh_ctx_create")
        self._ctx = h
        self.set_num_sample(self.NUM_SAMPLE)
        self._scratch = None
        self.bust_tree = self.scalp_tree = self.scalp_max = None
        self.base_view_override = None

    def set_num_sample(self, num_sample):
        """The sample count of forward()'s search (the reference's default argument of sample_next_3d_pos, PMVO.py:263) on
        this object: NUM_SAMPLE and the context's depth offsets.  The search takes up to 256 samples and, with the len(RANKS)
        base-view ranks, up to 1024 (rank, sample) items (include/mh_pmvo.h)."""
        offs = depth_offsets(int(num_sample))
        _lib.check(self._L.mh_ctx_set_depth_offsets(self._ctx, offs.ctypes.data_as(ctypes.c_void_p), len(offs)),
                   "mh_ctx_set_depth_offsets")
        self.NUM_SAMPLE = len(offs)

    def _alloc(self, V, H, W):
        self.num_view = V
        _lib.check(self._L.mh_ctx_alloc_views(self._ctx, V, H, W), "mh_ctx_alloc_views")

    def _set_view(self, i, rec, d, ds, o, c, m, ms, st):
        rec = np.ascontiguousarray(rec, dtype=np.float32)
        _lib.check(self._L.mh_ctx_set_view(self._ctx, i, rec.ctypes.data_as(ctypes.c_void_p), _lib.ptr(d), ds,
                                           _lib.ptr(o), _lib.ptr(c), _lib.ptr(m), ms, st), "mh_ctx_set_view")
        # the pack kernel reads d/o/c/m asynchronously: keep them alive until it has run
        torch.cuda.current_stream().synchronize()

    def __del__(self):
        # an object dropped with uploads in flight must not release its pinned slabs under them (see _upload_points)
        try:
            for ring in getattr(self, "_stage", {}).values():
                self._drain_ring(ring)
            stg = getattr(self, "_stage_all", None)
            if stg is not None and stg[1] is not None:
                stg[1].synchronize()
            for ent in getattr(self, "_stage_named", {}).values():
                ent[1].synchronize()
        except Exception:
            pass
        try:
            if getattr(self, "_ctx", None):
                self._L.mh_ctx_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    LAB_OPTIONS = ("search_variant", "search_body", "tap_plane", "tap_codes", "taps_tile", "filter_rows")

    def set_option(self, key, value):
        """A supported option of the context (include/mh_pmvo.h: reproject_rule, reproject_fma_min_cols, sum_block, topk_order,
        gabor_variant, tap_plane_max_mb, line_rule, raster_subpixel_bits).  The lab switches of include/mh_pmvo_lab.h (A/B
        forms and cross-check kernels: LAB_OPTIONS) are routed to mh_ctx_set_lab_option so that tests and bench.py keep one call."""
        if key in self.LAB_OPTIONS:
            return self.set_lab_option(key, value)
        _lib.check(self._L.mh_ctx_set_option(self._ctx, key.encode(), int(value)), "mh_ctx_set_option")

    def set_lab_option(self, key, value):
        _lib.check(self._L.mh_ctx_set_lab_option(self._ctx, key.encode(), int(value)), "mh_ctx_set_lab_option")

    def set_head(self, bust_tree, scalp_tree, scalp_max):
        """The reference reads these from module globals (PMVO.py:99-106, 814-820)."""
        self.bust_tree, self.scalp_tree, self.scalp_max = bust_tree, scalp_tree, scalp_max

    def _dev_points(self, points):
        """[N,3] points -> float32 on the device.  numpy input is cast on the host first, as the reference does
        (`torch.from_numpy(points).type(torch.float).to(device)`, PMVO.py:40): same rounding, half the H2D bytes and no
        cast kernel on the stream."""
        if isinstance(points, np.ndarray):
            return self._upload_points(points)
        return points.to(self.device).type(torch.float).contiguous()

    def upload_all_points(self, points, head=0, after_head=None):
        """One asynchronous upload of a whole [M,3] host array (float32 cast on the host, PMVO.py:40) through one pinned
        staging buffer kept on the object; the drivers then hand device slices to forward().
        head > 0: rows [0, head) are converted and copied first, `after_head(dev)` is called (the driver launches the first
        chunks there), then the rest is converted and copied -- the host-side conversion of a large float64 array (1 ms per
        300 k points) then runs while the GPU already works.  Returns (device tensor, float32 host view of the staged rows --
        valid until the next call)."""
        m = int(points.shape[0])
        if m == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=self.device), np.zeros((0, 3), np.float32)
        stg = getattr(self, "_stage_all", None)
        if stg is not None and stg[1] is not None:
            stg[1].synchronize()
        if stg is None or stg[0].shape[0] < m:
            stg = self._stage_all = [torch.empty((m, 3), dtype=torch.float32, pin_memory=True), torch.cuda.Event()]
        host = stg[0].numpy()[:m]
        dev = torch.empty((m, 3), dtype=torch.float32, device=self.device)
        cs = torch.cuda.current_stream(self.device)
        head = min(max(int(head), 0), m) if after_head is not None else 0
        for part, (lo, hi) in enumerate(((0, head), (head, m))):
            if hi > lo:
                np.copyto(host[lo:hi], points[lo:hi], casting="same_kind")
                _lib.check(self._L.mh_upload_async(self._ctx, stg[0].data_ptr() + lo * 12, dev.data_ptr() + lo * 12,
                                                   (hi - lo) * 12, cs.cuda_stream), "mh_upload_async")
            if part == 0 and after_head is not None:
                after_head(dev)
        stg[1].record(cs)
        return dev, host

    def _upload_points(self, points, stream=None):
        """Host numpy [N,3] -> float32 device tensor through a ring of PINNED staging slots per launch stream and
        an asynchronous copy.  `tensor.to(device)` from pageable memory blocks the host for ~0.2 ms per call (staging +
        wait) -- as long as a whole iteration takes on 8-bit maps, which made the loop of `optimize` host-bound there.
        The float64 -> float32 cast happens in the copy into the staging buffer (numpy's rounding = the reference's
        `.type(torch.float)`, PMVO.py:40)."""
        n = int(points.shape[0])
        if n == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=self.device)
        cs = torch.cuda.current_stream(self.device) if stream is None else stream
        ring = self._stage.get(cs.cuda_stream)
        if ring is None or ring["cap"] < n:
            # ONE pinned slab of 32 slots per launch stream (3 MB), allocated on the stream's first call (a ring that grew
            # slot by slot paid a pinned allocation -- milliseconds, and it drains the device -- up to 32 times per stream
            # during the first few hundred iterations of a loop)
            # The copies go through mh_upload_pinned, which torch's host caching allocator does not track: before the old slab
            # is dropped (its pinned block could be handed out again at once), every copy still queued out of it must be over.
            self._drain_ring(ring)
            cap = max(n, 8192)
            slab = torch.empty((self._STAGE_SLOTS, cap, 3), dtype=torch.float32, pin_memory=True)
            ring = self._stage[cs.cuda_stream] = {"cap": cap, "slab": slab, "np": slab.numpy(), "i": 0,
                                                  "ptr": slab.data_ptr(), "ev": [None] * self._STAGE_SLOTS}
        # slots are used in ring order (copies of one stream complete in order); a slot whose copy is still pending means the
        # host is 32 iterations ahead of a GPU-bound loop: only then does it wait
        k = ring["i"] % self._STAGE_SLOTS
        ring["i"] += 1
        ev = ring["ev"][k]
        if ev is None:
            ev = ring["ev"][k] = torch.cuda.Event()
        elif not ev.query():
            ev.synchronize()
        np.copyto(ring["np"][k, :n], points, casting="same_kind")
        dev = torch.empty((n, 3), dtype=torch.float32, device=self.device)
        # (not `dev.copy_(pinned, non_blocking=True)`: that also records an allocator-tracking event per call -- 70 -> 55 us of
        # host time per forward())
        _lib.check(self._L.mh_upload_pinned(self._ctx, ring["ptr"] + k * ring["cap"] * 12, dev.data_ptr(), n * 12,
                                            cs.cuda_stream), "mh_upload_pinned")
        ev.record(cs)
        return dev

    _STAGE_SLOTS = 32

    @staticmethod
    def _drain_ring(ring):
        """wait for every asynchronous copy that still reads from a staging ring's pinned slab"""
        for ev in (ring or {}).get("ev", ()):
            if ev is not None:
                ev.synchronize()

    # ------------------------------------------------------------------ reference methods
    def Compute_Visible_and_Ori(self, points):
        """PMVO.py:346-376 -> one mh_project_gather launch."""
        points = self._dev_points(points)
        V, N, P = self.num_view, points.shape[0], self._side ** 2
        f = dict(dtype=torch.float32, device=self.device)
        self.visible = torch.empty((V, N), **f)
        self.Ori = torch.empty((V, N, 2), **f)
        self.Conf = torch.empty((V, N), **f)
        self.mask = torch.empty((V, N), **f)
        self._Ori_patch = torch.empty((V, N, P, 2), **f)
        self._Conf_patch = torch.empty((V, N, P), **f)
        self._pixf = torch.empty((V, N, 2), **f)
        self._points = points
        _lib.check(self._L.mh_project_gather(self._ctx, _lib.ptr(points), N, self._side, _lib.ptr(self.visible),
                                             _lib.ptr(self.Ori), _lib.ptr(self.Conf), _lib.ptr(self.mask),
                                             _lib.ptr(self._Ori_patch), _lib.ptr(self._Conf_patch),
                                             _lib.ptr(self._pixf), _lib.stream_ptr()), "mh_project_gather")

    def _materialise_patches(self):
        """forward() does not write the [V,N,P,..] patch tensors (its fused front end builds the search's tap
        lists straight from the maps); they are produced on first access so the attribute surface of the
        reference (PMVO.py:374-376) is kept."""
        if getattr(self, "_Ori_patch", None) is None and getattr(self, "_points", None) is not None:
            self.Compute_Visible_and_Ori(self._points)

    @property
    def Ori_patch(self):
        self._materialise_patches()
        return self._Ori_patch

    @property
    def Conf_patch(self):
        self._materialise_patches()
        return self._Conf_patch

    def _topk32(self, stp=None):
        V, N = self.visible.shape
        idx = torch.empty((20, N), dtype=torch.int32, device=self.device)
        val = torch.empty((20, N), dtype=torch.float32, device=self.device)
        _lib.check(self._L.mh_topk_views(self._ctx, _lib.ptr(self.visible), _lib.ptr(self.Conf), N, _lib.ptr(idx),
                                         _lib.ptr(val), _lib.stream_ptr() if stp is None else stp), "mh_topk_views")
        return idx, val

    def Find_max_conf_from_visible_view(self):
        """PMVO.py:339-343 -> (base_view_index [20,N] int64, base_view_conf [20,N])."""
        idx, val = self._topk32()
        return idx.long(), val

    # ------------------------------------------------------------------ the reference's intermediate methods
    # (PMVO.forward above is fused and does not call them; same names, arguments and returns as PMVO.py)
    def _view_index(self, view):
        """camera key / Camera object / integer -> index of the resident view"""
        if isinstance(view, (int, np.integer)):
            return int(view)
        if isinstance(view, str):
            return self.camera_key.index(view)
        for i, c in enumerate(self.camera or []):
            if c is view:
                return i
        name = getattr(view, "id", None)
        if name in self.camera_key:
            return self.camera_key.index(name)
        raise _lib.MhError("unknown view %r" % (view,))

    def project_points(self, points, camera, image_size=None):
        """PMVO.py:378-397 -> (uv [N,2] long as (row, col), z' = -z/2 [N], out-of-image flags [N]).  `camera`: one of
        the resident cameras (object, key or index); image_size must be the resident one."""
        pts = self._dev_points(points)
        N = pts.shape[0]
        if image_size is not None and [int(image_size[0]), int(image_size[1])] != self.image_size:
            raise _lib.MhError("project_points: image_size differs from the resident maps")
        rc = torch.empty((N, 2), dtype=torch.int32, device=self.device)
        zp = torch.empty((N,), dtype=torch.float32, device=self.device)
        oob = torch.empty((N,), dtype=torch.bool, device=self.device)
        _lib.check(self._L.mh_project_points(self._ctx, self._view_index(camera), _lib.ptr(pts), N, _lib.ptr(rc),
                                             _lib.ptr(zp), _lib.ptr(oob), None, _lib.stream_ptr()), "mh_project_points")
        return rc.long(), zp, oob

    def _gather(self, uv, view, size=1, want_mask=False):
        uv = torch.as_tensor(uv).to(self.device).long().contiguous()
        size = 2 * (int(size) // 2) + 1          # range(-(size // 2), size // 2 + 1): an even size is the next odd window
        N, P = uv.shape[0], size * size
        rec = torch.empty((N, P, 4), dtype=torch.float32, device=self.device)
        mask = torch.empty((N, P), dtype=torch.float32, device=self.device) if want_mask else None
        _lib.check(self._L.mh_gather_pixels(self._ctx, self._view_index(view), _lib.ptr(uv), N, size, _lib.ptr(rec),
                                            _lib.ptr(mask), _lib.stream_ptr()), "mh_gather_pixels")
        return rec, mask

    def get_depth(self, uv, view):
        """PMVO.py:482-485"""
        return self._gather(uv, view)[0][:, 0, 3]

    def get_ori(self, uv, view):
        """PMVO.py:487-489"""
        return self._gather(uv, view)[0][:, 0, 0:2]

    def get_conf(self, uv, view):
        """PMVO.py:517-519 (raw, unclamped)"""
        return self._gather(uv, view)[0][:, 0, 2]

    def get_mask(self, uv, view):
        """PMVO.py:521-523"""
        return self._gather(uv, view, want_mask=True)[1][:, 0]

    def get_ori_patch(self, uv, view, size=1):
        """PMVO.py:491-502 -> [N, side*side, 2], side = 2 * (size // 2) + 1"""
        return self._gather(uv, view, size)[0][..., 0:2].contiguous()

    def get_c_patch(self, uv, view, size=1):
        """PMVO.py:504-515 -> [N, side*side], side = 2 * (size // 2) + 1"""
        return self._gather(uv, view, size)[0][..., 2].contiguous()

    def compute_visible(self, depth, z):
        """PMVO.py:525-529 (z is already -z_cam/2*255)"""
        depth = torch.as_tensor(depth).to(self.device).float().contiguous()
        z = torch.as_tensor(z).to(self.device).float().contiguous().expand_as(depth).contiguous()
        out = torch.empty_like(depth)
        _lib.check(self._L.mh_compute_visible(self._ctx, _lib.ptr(depth), _lib.ptr(z), depth.numel(), _lib.ptr(out),
                                              _lib.stream_ptr()), "mh_compute_visible")
        return out

    def compute_weight(self, visible, Conf, mask):
        """PMVO.py:211-215: (visible != -1) * Conf; the mask `where` of the reference is an identity"""
        return torch.where(visible == -1, torch.zeros_like(visible), torch.ones_like(visible)) * Conf

    def sample_next_3d_pos(self, points, base_view_index, num_sample=90):
        """PMVO.py:263-335 -> (sample_points [N,num_sample,3], surface_points [N,3]); needs Compute_Visible_and_Ori
        on the same points.  (The reference's surface-point assignment at :333-334 writes into a temporary, so
        surface_points is a copy of points there too.)"""
        pts = self._dev_points(points)
        N = pts.shape[0]
        if getattr(self, "Ori", None) is None or self.Ori.shape[1] != N:
            raise _lib.MhError("sample_next_3d_pos: call Compute_Visible_and_Ori(points) first")
        base = torch.as_tensor(base_view_index).to(self.device).to(torch.int32).contiguous()
        offs = torch.from_numpy(depth_offsets(num_sample)).to(self.device)
        out = torch.empty((N, offs.shape[0], 3), dtype=torch.float32, device=self.device)
        _lib.check(self._L.mh_sample_next(self._ctx, _lib.ptr(pts), _lib.ptr(base), _lib.ptr(self.Ori), _lib.ptr(offs), N,
                                          offs.shape[0], _lib.ptr(out), _lib.stream_ptr()), "mh_sample_next")
        return out, pts.clone()

    def compute_reproject_ori(self, points, sample_next_points):
        """PMVO.py:219-241 -> [V, N, num_sample, 2]"""
        pts = self._dev_points(points)
        smp = torch.as_tensor(sample_next_points).to(self.device).float().contiguous()
        N, S = smp.shape[0], smp.shape[1]
        D = torch.empty((self.num_view, N, S, 2), dtype=torch.float32, device=self.device)
        _lib.check(self._L.mh_reproject_ori(self._ctx, _lib.ptr(pts), _lib.ptr(smp), N, S, _lib.ptr(D),
                                            _lib.stream_ptr()), "mh_reproject_ori")
        return D

    def compute_points_prj_ori(self, points, next_points):
        """PMVO.py:243-260 -> [V, N, 2]"""
        nxt = torch.as_tensor(next_points).to(self.device).float()
        return self.compute_reproject_ori(points, nxt[:, None, :])[:, :, 0, :].contiguous()

    def compute_prj_loss(self, Prj_Ori_2D, Ori=None, weight=None):
        """PMVO.py:151-209 -> (min_loss [N], min_index [N] long, high_conf_index [N] bool) on the patches of the last
        Compute_Visible_and_Ori (the reference ignores its `Ori` and `weight` arguments too)."""
        D = torch.as_tensor(Prj_Ori_2D).to(self.device).float().contiguous()
        V, N, S, _ = D.shape
        P = self._side ** 2
        loss = torch.empty((N,), dtype=torch.float32, device=self.device)
        idx = torch.empty((N,), dtype=torch.int64, device=self.device)
        hc = torch.empty((N,), dtype=torch.bool, device=self.device)
        _lib.check(self._L.mh_prj_loss(self._ctx, _lib.ptr(D), _lib.ptr(self.Ori_patch), _lib.ptr(self.Conf_patch),
                                       _lib.ptr(self.visible), V, N, S, P, float(self.conf_threshold), _lib.ptr(loss),
                                       _lib.ptr(idx), _lib.ptr(hc), None, _lib.stream_ptr()), "mh_prj_loss")
        return loss, idx, hc

    def side_streams(self, n=3):
        """n HIP streams owned by this object (created once; the per-stream search scratch is keyed by them)."""
        if len(getattr(self, "_side_streams", [])) < n:
            self._side_streams = [torch.cuda.Stream(device=self.device) for _ in range(n)]
        return self._side_streams[:n]

    def aux_stream(self, name, priority=None):
        """A named HIP stream owned by this object, created on first use (the drivers' copy / side / prefetch streams)."""
        d = self.__dict__.setdefault("_aux_streams", {})
        if name not in d:
            d[name] = (torch.cuda.Stream(device=self.device) if priority is None
                       else torch.cuda.Stream(device=self.device, priority=int(priority)))
        return d[name]

    _TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8}

    def stage_fill(self, key, arr, dtype=np.float32):
        """First half of stage_upload, safe to run on a worker thread (one key per thread): convert / copy `arr` into the
        pinned staging buffer of `key` (waiting for the previous copy out of it).  -> handle for stage_issue."""
        a = np.asarray(arr)
        dt = np.dtype(dtype)
        nbytes = a.size * dt.itemsize
        if nbytes == 0:
            return (None, a.shape, dt, 0)
        pool = self.__dict__.setdefault("_stage_named", {})
        ent = pool.get(key)
        if ent is not None:
            ent[1].synchronize()          # the previous copy out of this buffer
        if ent is None or ent[0].numel() < nbytes:
            ent = pool[key] = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
        host = ent[0].numpy()[:nbytes].view(dt).reshape(a.shape)
        np.copyto(host, a, casting="same_kind")
        return (ent, a.shape, dt, nbytes)

    def stage_issue(self, handle):
        """Second half: the asynchronous copy of a filled staging buffer on the current stream -> fresh device tensor."""
        ent, shape, dt, nbytes = handle
        dev = torch.empty(shape, dtype=self._TORCH_OF[dt], device=self.device)
        if nbytes == 0:
            return dev
        cs = torch.cuda.current_stream(self.device)
        _lib.check(self._L.mh_upload_pinned(self._ctx, ent[0].data_ptr(), dev.data_ptr(), nbytes, cs.cuda_stream),
                   "mh_upload_pinned")
        ent[1].record(cs)
        return dev

    def stage_upload(self, key, arr, dtype=np.float32):
        """Host array -> fresh device tensor of `dtype` through a pinned staging buffer kept per `key`: one conversion /
        copy on the host (numpy's rounding for float64 -> float32 = the reference's `.type(torch.float)`, PMVO.py:40), one
        asynchronous copy on the current stream.  `tensor.to(device)` from pageable memory blocks the host for the whole
        transfer; the drivers upload a pass's arrays while the GPU works."""
        return self.stage_issue(self.stage_fill(key, arr, dtype))

    def start_refine_prefetch(self, pts_dev, sub_num=5000, k=100):
        """What refine() needs of the POINTS alone (PMVO.py:605-612 the 100 nearest neighbours of every point; :96-137 the
        head-filter votes and the scalp test) is prepared on a stream of its own while optimize()'s iterations run: see
        RefinePrefetch.  Called by optimize() once its launches are queued; refine() adopts the result if it is handed
        the same points (compared on the device, bit for bit)."""
        if os.environ.get("MH_REFINE_PREFETCH", "1") == "0":
            self._prefetch = None
            return None
        self._prefetch = RefinePrefetch(self, pts_dev, sub_num, k)
        return self._prefetch

    def take_refine_prefetch(self, pts_dev, sub_num, k):
        """The prefetch of start_refine_prefetch if it was made for exactly these points and thresholds, else None."""
        pf, self._prefetch = getattr(self, "_prefetch", None), None
        if pf is None:
            return None
        return pf.adopt(pts_dev, sub_num, k)

    def _get_scratch(self, N, key=None):
        """Tap-list scratch of the search, one buffer per launch stream (chunks of `optimize` are independent and
        may be in flight on different streams)."""
        need = self._scratch_need.get(N)
        if need is None:
            need = self._scratch_need[N] = int(self._L.mh_search_scratch_bytes(self._ctx, N, self._side))
        if key is None:
            key = torch.cuda.current_stream().cuda_stream
        if self._scratch is None:
            self._scratch = {}
        buf = self._scratch.get(key)
        if buf is None or buf.numel() < need:
            buf = torch.empty(need, dtype=torch.uint8, device=self.device)
            self._scratch[key] = buf
        return buf, need

    def search_work(self, N, base_val=None):
        """What the last forward() on the current stream executed: (list lengths [V,N] int64, usable ranks [N] or None).
        The preparation kernels leave the per-(view, point) tap-list lengths in the scratch (0 = the view does not see
        the point); with base_val [20,N] the number of base-view ranks the search evaluated per point (rank 0 always,
        later ranks up to the last one with base_view_conf > 0, PMVO.py:64)."""
        buf, _ = self._get_scratch(N)
        off = int(self._L.mh_search_counts_offset(self._ctx, N, self._side))
        cnt = buf[off:off + self.num_view * N].view(self.num_view, N).to(torch.int64)
        nvalid = None
        if base_val is not None:
            pos = base_val[list(self.RANKS)] > 0                      # [len(RANKS), N]
            last = (pos * torch.arange(1, pos.shape[0] + 1, device=pos.device)[:, None]).amax(0)
            nvalid = torch.clamp(last, min=1)
        return cnt, nvalid

    def forward(self, points, base_view=None, extras=False, fused=True, out=None):
        """PMVO.py:39-78.  points: numpy [N,3].  Returns (points, line_ori [N,3], min_loss [N],
        high_conf [N] bool) on the device.  base_view=(idx [20,N], val [20,N]) injects a base-view ranking
        (parity tests: torch.topk's tie order is unspecified).  fused=False runs Compute_Visible_and_Ori and
        the tap preparation as separate kernels through the materialised patch tensors (same results).
        out=(line_ori [N,3] float32, min_loss [N] float32, high_conf [N] bool): contiguous device tensors the search
        writes into (the driver `optimize` passes slices of one result buffer: no per-chunk concatenation)."""
        ranks = list(self.RANKS)          # (the class's, or a set installed on this object)
        step = ranks[1] - ranks[0] if len(ranks) > 1 else 1
        assert ranks == list(range(0, step * len(ranks), step)), "RANKS must be 0, step, 2 * step, ... (mh_forward's nrank, rank_step)"
        f = dict(dtype=torch.float32, device=self.device)
        cs = torch.cuda.current_stream(self.device)          # looked up once: ~8 us of Python per call
        stp = ctypes.c_void_p(cs.cuda_stream)
        d_ = torch.Tensor.data_ptr          # raw addresses: ctypes converts ints to void* without a wrapper object each
        if fused:
            points = self._upload_points(points, cs) if isinstance(points, np.ndarray) else self._dev_points(points)
            V, N = self.num_view, points.shape[0]
            self.visible = torch.empty((V, N), **f)
            self.Ori = torch.empty((V, N, 2), **f)
            self.Conf = torch.empty((V, N), **f)
            self.mask = torch.empty((V, N), **f)
            self._Ori_patch = self._Conf_patch = self._pixf = None
            self._points = points
            scratch, need = self._get_scratch(N, cs.cuda_stream)
        else:
            self.Compute_Visible_and_Ori(points)
            points = self._points
            N = points.shape[0]
            scratch, need = self._get_scratch(N, cs.cuda_stream)
        if out is not None:
            line_ori, min_loss, hc = out
            assert line_ori.shape == (N, 3) and min_loss.shape == (N,) and hc.shape == (N,) and hc.dtype == torch.bool
            assert line_ori.is_contiguous() and min_loss.is_contiguous() and hc.is_contiguous() and line_ori.is_cuda
        else:
            line_ori = torch.empty((N, 3), **f)
            min_loss = torch.empty((N,), **f)
            hc = torch.empty((N,), dtype=torch.bool, device=self.device)      # the kernel writes 0/1 bytes
        bs = torch.empty((N, 3), **f) if extras else None
        br = torch.empty((N,), dtype=torch.int32, device=self.device) if extras else None
        bi = torch.empty((N,), dtype=torch.int32, device=self.device) if extras else None
        if fused and base_view is None:
            # the whole iteration in one call: projection / visibility / tap lists, base-view ranking, loss search
            bidx32 = torch.empty((20, N), dtype=torch.int32, device=self.device)
            bval = torch.empty((20, N), **f)
            if N:
                _lib.check(self._L.mh_forward(
                    self._ctx, d_(points), N, self._side, float(self.conf_threshold), len(ranks), step,
                    d_(self.visible), d_(self.Ori), d_(self.Conf), d_(self.mask), d_(scratch), need, d_(bidx32), d_(bval),
                    d_(line_ori), d_(min_loss), d_(hc), _lib.ptr(bs), _lib.ptr(br), _lib.ptr(bi), stp), "mh_forward")
        else:
            if fused:
                _lib.check(self._L.mh_forward_prepare(self._ctx, _lib.ptr(points), N, self._side,
                                                      float(self.conf_threshold), _lib.ptr(self.visible),
                                                      _lib.ptr(self.Ori), _lib.ptr(self.Conf), _lib.ptr(self.mask),
                                                      _lib.ptr(scratch), need, stp), "mh_forward_prepare")
            if base_view is None:
                bidx32, bval = self._topk32(stp)       # int32 end to end: no int64 round trip on the hot path
            else:
                bidx32 = torch.as_tensor(base_view[0]).to(self.device).to(torch.int32).contiguous()
                bval = torch.as_tensor(base_view[1]).to(self.device).type(torch.float).contiguous()
            if fused:
                _lib.check(self._L.mh_search_prepared(
                    self._ctx, _lib.ptr(points), N, self._side, float(self.conf_threshold), len(ranks),
                    step, _lib.ptr(self.Ori), _lib.ptr(bidx32), _lib.ptr(bval), _lib.ptr(scratch),
                    _lib.ptr(line_ori), _lib.ptr(min_loss), _lib.ptr(hc), _lib.ptr(bs), _lib.ptr(br), _lib.ptr(bi),
                    stp), "mh_search_prepared")
            else:
                _lib.check(self._L.mh_search_forward(
                    self._ctx, _lib.ptr(points), N, self._side, float(self.conf_threshold), len(ranks),
                    step, _lib.ptr(self.visible), _lib.ptr(self.Ori), _lib.ptr(self._pixf),
                    _lib.ptr(self._Ori_patch), _lib.ptr(self._Conf_patch), _lib.ptr(bidx32), _lib.ptr(bval),
                    _lib.ptr(scratch), need, _lib.ptr(line_ori), _lib.ptr(min_loss), _lib.ptr(hc), _lib.ptr(bs),
                    _lib.ptr(br), _lib.ptr(bi), stp), "mh_search_forward")
        out = (points, line_ori, min_loss, hc)
        if extras:
            return out + (dict(best_sample=bs, best_rank=br, best_s=bi, base_idx=bidx32.long(), base_val=bval),)
        return out

    __call__ = forward

    def prj_loss_of(self, points, ori):
        """compute_reproject_ori + compute_prj_loss for next = points + ori*0.005/4 (PMVO.py:86-90) on the
        state of the last Compute_Visible_and_Ori: (loss [N], high_conf [N] bool)."""
        N = points.shape[0]
        ori = ori.to(self.device).type(torch.float).contiguous()
        loss = torch.empty((N,), dtype=torch.float32, device=self.device)
        hc = torch.empty((N,), dtype=torch.uint8, device=self.device)
        _lib.check(self._L.mh_refine_loss(self._ctx, _lib.ptr(points), _lib.ptr(ori), 0.005, 4.0, N,
                                          self._side, float(self.conf_threshold), _lib.ptr(self.visible),
                                          _lib.ptr(self.Ori_patch), _lib.ptr(self.Conf_patch), _lib.ptr(loss),
                                          _lib.ptr(hc), _lib.stream_ptr()), "mh_refine_loss")
        return loss, hc.bool()

    def refine(self, points, ori, head_top=None):
        """PMVO.py:81-93: loss of a given direction; -1 where filter_head_points fires.  head_top: optional
        precomputed host part of filter_head_points (head_top_mask) so that the call does not synchronise."""
        self.Compute_Visible_and_Ori(points)
        points = self._points
        filter_index = self.filter_head_points(points, self.visible_threshold, head_top=head_top)
        loss, _ = self.prj_loss_of(points, ori)
        return torch.where(filter_index, torch.full_like(loss, -1.0), loss)

    def head_top_mask_device(self, points_dev):
        """The scalp half of filter_head_points (PMVO.py:98-107) for float32 points on the device: within 4 cm of the
        scalp and more than 1 cm below its top -> uint8 (0/1) tensor on the device.  The reference asks a scipy KDTree for the
        nearest scalp vertex (float64); here the distance to the nearest vertex is found exhaustively on the GPU in
        float64 (mh_nearest_distance: the same sum of squares and one sqrt), so the 4 cm decision is scipy's."""
        if self.scalp_tree is None:
            raise _lib.MhError("filter_head_points needs set_head(bust_tree, scalp_tree, scalp_max)")
        if getattr(self, "_scalp_dev", None) is None or self._scalp_dev[0] is not self.scalp_tree:
            ref = np.ascontiguousarray(np.asarray(self.scalp_tree.data, dtype=np.float64).reshape(-1, 3))
            self._scalp_dev = (self.scalp_tree, torch.from_numpy(ref).to(self.device))
        ref = self._scalp_dev[1]
        pts = points_dev if (points_dev.dtype == torch.float32 and points_dev.is_contiguous()) else \
            points_dev.to(self.device).type(torch.float).contiguous()
        N = pts.shape[0]
        mask = torch.empty((N,), dtype=torch.uint8, device=self.device)
        # (the height test in float64, as numpy evaluates `float32 array < float64 scalar` where the goldens were made)
        _lib.check(self._L.mh_nearest_distance(self._ctx, _lib.ptr(pts), N, _lib.ptr(ref), ref.shape[0], None, 0.04,
                                               float(self.scalp_max[2] - 0.01), _lib.ptr(mask), _lib.stream_ptr()),
                   "mh_nearest_distance")
        return mask

    def head_top_mask(self, points_numpy):
        """numpy in / numpy out form of head_top_mask_device (float32 points, as the reference passes them)."""
        pts = np.ascontiguousarray(np.asarray(points_numpy, dtype=np.float32).reshape(-1, 3))
        return self.head_top_mask_device(torch.from_numpy(pts).to(self.device)).cpu().numpy().astype(bool)

    def replace_dissimilar(self, center, ori, threshold=0.95):
        """ori[n] <- center[n] where |cos(center, ori)| < threshold, in place on the device (PMVO.py:631-636)."""
        N = ori.shape[0]
        _lib.check(self._L.mh_replace_dissimilar(self._ctx, _lib.ptr(center), _lib.ptr(ori), float(threshold), N,
                                                 _lib.stream_ptr()), "mh_replace_dissimilar")

    def _votes(self, points, want, visible_threshold=None, raw=False):
        """mask / visibility votes of mh_filter_points for the requested outputs; raw=True returns the kernel's uint8 0/1
        arrays instead of bool tensors.  (The points of one call are one batch of the reference: its sums over views add the
        trailing len mod 32 points of a batch in another order, include/mh_pmvo.h.)"""
        points = self._dev_points(points)
        N = points.shape[0]
        bufs = [torch.empty((N,), dtype=torch.uint8, device=self.device) if w else None for w in want]
        vt = self.visible_threshold if visible_threshold is None else visible_threshold
        _lib.check(self._L.mh_filter_points(self._ctx, _lib.ptr(points), N, self._side,
                                            float(self.conf_threshold), float(vt), _lib.ptr(bufs[0]),
                                            _lib.ptr(bufs[1]), _lib.ptr(bufs[2]), _lib.ptr(bufs[3]), 0, 0, 0,
                                            _lib.stream_ptr()), "mh_filter_points")
        if raw:
            return points, bufs
        return points, [None if b is None else b.bool() for b in bufs]

    def filter_points(self, points):
        """PMVO.py:402-459 -> (surface_index, surface_points, filter_index)."""
        points, (surf, filt, _, _) = self._votes(points, (True, True, False, False))
        return surf, points[surf], filt

    def compute_unvisible_points(self, points):
        """PMVO.py:461-480."""
        _, (_, _, unv, _) = self._votes(points, (False, False, True, False))
        return unv

    def filter_head_points(self, points, visible_threshold, head_top=None):
        """PMVO.py:96-144: mask vote on the GPU; the scalp KDTree query (scipy, float64) stays on the host exactly
        as in the reference (the bust query's result is unused there, :99).  head_top: optional precomputed
        head_top_mask of the same points (bool tensor on the device)."""
        pts, (_, _, _, head) = self._votes(points, (False, False, False, True), visible_threshold)
        if head_top is None:
            head_top = self.head_top_mask_device(pts)
        return torch.logical_and(head, ~head_top.bool())


class RefinePrefetch:
    """The point-only inputs of refine()'s smoothing loop, prepared while optimize() runs (single rank).

    refine's neighbour table `KDTree(points).query(points, 100)` (PMVO.py:605-612), the head-filter votes of every point
    (:110-137, per 5000-point chunk) and the scalp test (:98-107) depend on the points alone, and the points exist before
    optimize() starts.  A helper thread builds the grid, runs the self-query (with its host-side retries) and the two
    vote kernels on a low-priority stream of its own; the search kernels of optimize() keep the GPU, these fill what they
    leave.  refine() adopts the result only if the points it is handed equal these bit for bit (mh_buffers_differ on the
    device) and the thresholds are the ones used here; otherwise it computes everything itself as before."""

    def __init__(self, pmvo, pts_dev, sub_num, k):
        import threading

        self.pmvo, self.pts_dev, self.sub_num, self.k = pmvo, pts_dev, int(sub_num), int(k)
        self.n = int(pts_dev.shape[0])
        self.conf_threshold, self.visible_threshold = float(pmvo.conf_threshold), float(pmvo.visible_threshold)
        self.scalp_tree = pmvo.scalp_tree
        self.error = None
        self.grid = self.index_all = self.head_all = self.head_top_all = None
        prio = os.environ.get("MH_PREFETCH_PRIORITY", "low")
        rng = (0, 0)
        try:
            rng = torch.cuda.Stream.priority_range()        # (least, greatest), e.g. (0, -1)
        except Exception:
            pass
        self.stream = pmvo.aux_stream("prefetch_" + prio, priority=(rng[0] if prio == "low" else 0))
        self.ready = torch.cuda.Event()
        self.ready.record(torch.cuda.current_stream(pmvo.device))      # pts_dev's upload is queued on the caller's stream
        self.done = torch.cuda.Event()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        from .pmvo_utils import GridKNN

        pm = self.pmvo
        try:
            with torch.cuda.device(pm.device), torch.cuda.stream(self.stream):
                self.stream.wait_event(self.ready)
                if self.n:
                    self.grid = GridKNN(self.pts_dev, k_hint=self.k, device=pm.device)
                    self.index_all = self.grid.query(self.pts_dev, self.k, int32=True, self_query=True).contiguous()
                    self.head_all = torch.empty((self.n,), dtype=torch.uint8, device=pm.device)
                    # (rows in the cell order of the grid the neighbour search just built: 64 spatial neighbours per wave)
                    _lib.check(pm._L.mh_filter_points_ordered(pm._ctx, _lib.ptr(self.pts_dev), self.n, pm._side,
                                                              self.conf_threshold, self.visible_threshold, None, None, None,
                                                              _lib.ptr(self.head_all), self.sub_num, 0, self.n,
                                                              _lib.ptr(self.grid.cell_order()), _lib.stream_ptr()),
                               "mh_filter_points_ordered")
                    if self.scalp_tree is not None:
                        self.head_top_all = pm.head_top_mask_device(self.pts_dev)
                self.done.record(self.stream)
        except BaseException as e:          # refine() then prepares these itself
            self.error = e

    def adopt(self, pts_dev, sub_num, k):
        """-> self (results valid on the CURRENT stream) or None.  Joins the helper thread."""
        self.thread.join()
        pm = self.pmvo
        if (self.error is not None or self.n != int(pts_dev.shape[0]) or self.n == 0 or self.sub_num != int(sub_num)
                or self.k != int(k) or self.conf_threshold != float(pm.conf_threshold)
                or self.visible_threshold != float(pm.visible_threshold) or self.scalp_tree is not pm.scalp_tree
                or self.head_top_all is None):
            return None
        cur = torch.cuda.current_stream(pm.device)
        cur.wait_event(self.done)
        flag = torch.empty(1, dtype=torch.int32, device=pm.device)
        _lib.check(pm._L.mh_buffers_differ(pm._ctx, _lib.ptr(pts_dev), _lib.ptr(self.pts_dev), self.n * 12, _lib.ptr(flag),
                                           _lib.stream_ptr()), "mh_buffers_differ")
        if int(flag.cpu().numpy()[0]) != 0:
            return None
        for t in (self.index_all, self.head_all, self.head_top_all):
            t.record_stream(cur)              # allocated on the prefetch stream, used on this one from now on
        self.grid.record_stream(cur)
        return self


# =====================================================================================================
# Drivers -- mirrors of the module-level functions of the reference's PMVO.py (:535-764).  Chunking, file
# names and dtypes are the reference's (they are its checkpoint/resume mechanism); with torch.distributed
# initialised the independent chunks are dealt round-robin to the ranks (monohair_amd.dist).
# =====================================================================================================
def _filter_single(points, pmvo, step, num_sub_p):
    """filter_negative_points on one rank: the candidates go up in a few large blocks (the float64 -> float32 conversion of
    block k+1 runs on the host while the GPU votes on block k), one vote launch per block -- the kernel is told where its
    points sit in the reference's N//30-sized pieces (PMVO.py:540-552; include/mh_pmvo.h: batch / row0 / total) -- and the
    surface points are compacted on the device (`covered[surface].astype(float32)` = the selected rows of the float32
    copy the votes were computed on).  -> (flags [total,2] uint8 numpy, surface_points float32 [S,3] numpy, pinned)."""
    from .pmvo_utils import spatial_order

    dev = pmvo.device
    L, ctx = pmvo._L, pmvo._ctx
    total = min(int(points.shape[0]), step * num_sub_p)
    per = max(1, -(-step // 4)) * num_sub_p                      # four blocks, cut at piece boundaries
    bounds = [(lo, min(lo + per, total)) for lo in range(0, total, per)]
    surf = torch.empty((total,), dtype=torch.uint8, device=dev)
    filt = torch.empty((total,), dtype=torch.uint8, device=dev)
    out = torch.empty((total, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros((len(bounds) + 1,), dtype=torch.int32, device=dev)
    scratch = torch.empty(int(L.mh_select_scratch_bytes(per)), dtype=torch.uint8, device=dev)
    st = _lib.stream_ptr()
    off = lambda t, row, width=1: ctypes.c_void_p(t.data_ptr() + row * width * t.element_size())   # noqa: E731
    for k, (lo, hi) in enumerate(bounds):
        # (the conversions of the four blocks on four worker threads side by side: 3.9-4.1 ms for the stage instead of 3.2 --
        # thread wake-ups and the GIL cost more than the 0.25 ms conversions they overlap; measured, dropped)
        blk = pmvo.stage_upload("filter%d" % k, points[lo:hi])
        # (the rows of a block are taken cell by cell -- 64 spatial neighbours per wave -- not in the candidates' raster order)
        order = spatial_order(blk)
        _lib.check(L.mh_filter_points_ordered(ctx, _lib.ptr(blk), hi - lo, pmvo._side, float(pmvo.conf_threshold),
                                              float(pmvo.visible_threshold), off(surf, lo), off(filt, lo), None, None,
                                              num_sub_p, lo, total, _lib.ptr(order), st), "mh_filter_points_ordered")
        _lib.check(L.mh_select_rows(ctx, off(surf, lo), None, 0, hi - lo, _lib.ptr(blk), None, _lib.ptr(out), None, None,
                                    off(cnt, k), off(cnt, k + 1), _lib.ptr(scratch), scratch.numel(), st), "mh_select_rows")
    flags = torch.empty((2, total), dtype=torch.uint8, pin_memory=True)
    hcnt = torch.empty((1,), dtype=torch.int32, pin_memory=True)
    flags[0].copy_(surf, non_blocking=True)
    flags[1].copy_(filt, non_blocking=True)
    hcnt.copy_(cnt[len(bounds):], non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    S = int(hcnt[0])
    pts = torch.empty((S, 3), dtype=torch.float32, pin_memory=True)
    pts.copy_(out[:S], non_blocking=True)
    torch.cuda.current_stream(dev).synchronize()
    return flags.numpy(), pts.numpy()


def filter_negative_points(points, pmvo, args, step=30):
    """PMVO.py:535-557: surface / shell classification of the raw candidates, in N//30-sized pieces."""
    from . import dist as mdist

    if points.shape[0] % step != 0:
        step = step + 1
    num_sub_p = points.shape[0] // 30
    if mdist.world() == 1 and num_sub_p > 0 and isinstance(points, np.ndarray) and os.environ.get("MH_FILTER_BLOCKS", "1") != "0":
        flags, surface_points = _filter_single(points, pmvo, step, num_sub_p)
        surface_indexs, filter_indexs = flags[0].astype(bool), flags[1].astype(bool)
        print("surface_num:", surface_points.shape[:])
        print("num filter_unvisible:", np.sum(filter_indexs))
        return surface_indexs, surface_points, filter_indexs
    pieces = [points[i * num_sub_p:(i + 1) * num_sub_p] for i in range(step)]

    def work(sub):
        # the two vote arrays as the kernel writes them (uint8); the numpy piece is cast to float32 on the host like every
        # other entry point (PMVO.py:40), the gathered surface points of filter_points are not needed here
        _, (s, f, _, _) = pmvo._votes(sub, (True, True, False, False), raw=True)
        return torch.stack([s, f], 1)

    flags = mdist.map_chunks(pieces, work, pmvo.device, empty=lambda: torch.empty((0, 2), dtype=torch.uint8,
                                                                               device=pmvo.device))
    flags = torch.cat(flags, 0).cpu().numpy().astype(bool)
    surface_indexs, filter_indexs = flags[:, 0], flags[:, 1]
    covered = points[:flags.shape[0]]
    surface_points = covered[surface_indexs].astype(np.float32)   # the reference returns the fp32 copies
    print("surface_num:", surface_points.shape[:])
    print("num filter_unvisible:", np.sum(filter_indexs))
    return surface_indexs, surface_points, filter_indexs


def _start_mat_prefault(pmvo, args, points):
    """Ori3D.mat / Occ3D.mat of refine() are created and their pages made resident by a background thread (SparseMatWriter:
    26 ms of page faults at the headline size).  With refine's device-resident pass the whole of refine takes less than
    that, so the thread starts HERE, while optimize()'s iterations run: every surface point is a candidate voxel.  refine()
    adopts the writer when it is asked for the same directory and the default grid; a writer that is not adopted removes
    its temporary files when it is dropped."""
    from . import dist as mdist
    from . import pmvo_utils as U

    old = getattr(pmvo, "_mat_early", None)
    pmvo._mat_early = None
    if old is not None:
        old[1].abort()
    path = getattr(args, "save_path", "") or ""
    if mdist.rank() != 0 or not os.path.isdir(path) or os.environ.get("MH_MAT_EARLY", "1") == "0" or not len(points):
        return
    pmvo._mat_early = (path, U.SparseMatWriter(path, U.GRID_RESOLUTION, points, U.VOXEL_MIN, U.VOXEL_SIZE))


def _optimize_single(pts_np, pmvo, args):
    """optimize() on one rank.  The chunks rotate over three HIP streams (consecutive chunks are independent: the tail of
    one chunk's search kernel -- workgroups of points that see many views -- overlaps the front end and the head of the
    next chunks); every chunk's search writes straight into its slice of three device buffers.  The result files are
    STREAMED: a copy stream brings the rows of each group of eight finished chunks to pinned host arrays while later
    chunks compute, and the host appends them to optimize/*.npy (np.save's bytes, NpyRowWriter) -- when the last search
    ends, one group is left to copy and write.  While the GPU iterates, what refine() needs of the points alone is
    prepared on a low-priority stream (PMVO.start_refine_prefetch)."""
    from concurrent.futures import ThreadPoolExecutor

    from .pmvo_utils import NpyRowWriter

    num_sub_p = 5000
    M = int(pts_np.shape[0])
    step = M // num_sub_p + 1
    dev = pmvo.device
    streams = pmvo.side_streams(3)     # kept on the object: their tap-list scratch (1.2 GB each) is reused
    main = torch.cuda.current_stream(dev)
    cp = pmvo.aux_stream("copy")
    o_all = torch.empty((M, 3), dtype=torch.float32, device=dev)
    l_all = torch.empty((M,), dtype=torch.float32, device=dev)
    h_all = torch.empty((M,), dtype=torch.bool, device=dev)
    # the arrays the caller gets: pinned, filled group by group (torch's host allocator recycles the blocks)
    ho = torch.empty((M, 3), dtype=torch.float32, pin_memory=True)
    hl = torch.empty((M,), dtype=torch.float32, pin_memory=True)
    hh = torch.empty((M,), dtype=torch.bool, pin_memory=True)
    done = {}                          # chunk -> event on its stream

    def launch(dev_all, lo_chunk, hi_chunk):
        for st in streams:
            st.wait_stream(main)      # the copy of these rows (and whatever produced the maps) has been enqueued on `main`
        for i in range(lo_chunk, hi_chunk):
            a, b = i * num_sub_p, min((i + 1) * num_sub_p, M)
            if b <= a:
                continue
            st = streams[i % len(streams)]
            with torch.cuda.stream(st):
                pmvo.forward(dev_all[a:b], out=(o_all[a:b], l_all[a:b], h_all[a:b]))
                done[i] = torch.cuda.Event()
                done[i].record(st)

    nhead = len(streams)               # chunks launched before the rest of the points is converted and copied
    # the candidate points go to the device ONCE (3.4 MB at the headline size); a chunk is a slice of that tensor
    dev_all, staged = pmvo.upload_all_points(pts_np, head=nhead * num_sub_p, after_head=lambda d: launch(d, 0, nhead))
    # (the prefetch's helper thread starts BEFORE the bulk of the forwards is queued: its first launches then sit early in the
    # hardware queues and its host-side synchronisations pass while the GPU iterates -- 52.0-52.4 ms per pass against 52.4-53.6
    # when it was started behind them)
    pmvo.start_refine_prefetch(dev_all, num_sub_p, 100)
    launch(dev_all, nhead, step)
    _start_mat_prefault(pmvo, args, pts_np)
    # select_p.npy is the float32 copy of the input (PMVO.py:40,575): written while the GPU works
    select_points = pts_np if (pts_np.dtype == np.float32 and pts_np.flags.c_contiguous) else staged.copy()
    os.makedirs(args.save_root, exist_ok=True)
    pool = ThreadPoolExecutor(1)
    early = pool.submit(np.save, args.save_root + "/select_p.npy", select_points)
    # groups of finished chunks -> pinned host rows -> files
    files = (NpyRowWriter(args.save_root + "/select_o.npy", (M, 3), np.float32),
             NpyRowWriter(args.save_root + "/min_loss.npy", (M,), np.float32),
             NpyRowWriter(args.save_root + "/high_conf_index.npy", (M,), np.bool_))
    chunks = sorted(done)
    GROUP = 8
    groups = []
    with torch.cuda.stream(cp):
        for g0 in range(0, len(chunks), GROUP):
            grp = chunks[g0:g0 + GROUP]
            for i in grp[-len(streams):]:                 # the last chunk of the group on each stream
                cp.wait_event(done[i])
            a, b = grp[0] * num_sub_p, min((grp[-1] + 1) * num_sub_p, M)
            ho[a:b].copy_(o_all[a:b], non_blocking=True)
            hl[a:b].copy_(l_all[a:b], non_blocking=True)
            hh[a:b].copy_(h_all[a:b], non_blocking=True)
            ev = torch.cuda.Event()
            ev.record(cp)
            groups.append((a, b, ev))
    select_ori, min_loss, high_conf_index = ho.numpy(), hl.numpy(), hh.numpy()
    for a, b, ev in groups:
        ev.synchronize()
        files[0].write(select_ori[a:b])
        files[1].write(min_loss[a:b])
        files[2].write(high_conf_index[a:b])
    for f in files:
        f.close()
    for st in streams:                 # (all their work is over: the last group's copy waited for it)
        main.wait_stream(st)
    main.wait_stream(cp)
    early.result()
    pool.shutdown()
    return select_points, select_ori, min_loss, high_conf_index


def optimize(points, pmvo, args):
    """PMVO.py:565-595: forward() over chunks of 5000 points, results to optimize/*.npy.
    Returns (select_points, select_ori, min_loss, high_conf_index) -- the arrays the reference loads back from the files
    (PMVO.py:868-870); on one rank they live in pinned host memory."""
    from . import dist as mdist

    num_sub_p = 5000
    step = points.shape[0] // num_sub_p + 1
    pts_np = points if isinstance(points, np.ndarray) else torch.as_tensor(points).detach().cpu().numpy()
    if mdist.world() == 1:
        out = _optimize_single(pts_np, pmvo, args)
        assert len(out[2]) == len(out[0])
        return out
    from concurrent.futures import ThreadPoolExecutor

    pool = ThreadPoolExecutor(4)
    streams = pmvo.side_streams(3)
    counter = [0]
    main = torch.cuda.current_stream()

    def join():                        # results are read on the main stream: join the side streams first
        for st in streams:
            main.wait_stream(st)

    # ONE float64 -> float32 conversion (numpy's rounding = the reference's `.type(torch.float)`, PMVO.py:40), in the pinned
    # staging buffer: the result is both what is uploaded and select_p.npy (PMVO.py:575)
    dev_all, select_points = pmvo.upload_all_points(pts_np)
    select_points = select_points.copy()
    early = None
    if mdist.rank() == 0:
        os.makedirs(args.save_root, exist_ok=True)
        early = pool.submit(np.save, args.save_root + "/select_p.npy", select_points)
    for st in streams:
        st.wait_stream(main)
    chunks = [dev_all[i * num_sub_p:(i + 1) * num_sub_p] for i in range(step)]

    def work(sub):
        st = streams[counter[0] % len(streams)]
        counter[0] += 1
        with torch.cuda.stream(st):
            _, o, l, h = pmvo.forward(sub)
            # (the points forward() returns are the float32 copy of its input: they do not travel back)
            out = torch.cat([o, l[:, None], h[:, None].to(torch.float32)], 1)
        out.record_stream(main)
        return out

    res = mdist.map_chunks(chunks, work, pmvo.device,
                           empty=lambda: torch.empty((0, 5), dtype=torch.float32, device=pmvo.device), after=join)
    res = torch.cat(res, 0).cpu().numpy()
    select_ori, min_loss = res[:, 0:3], res[:, 3]
    high_conf_index = res[:, 4] > 0.5
    assert len(min_loss) == len(select_points)
    if mdist.rank() == 0:
        jobs = (("select_o", select_ori), ("min_loss", min_loss), ("high_conf_index", high_conf_index))
        # the files are written side by side (numpy releases the GIL in write)
        list(pool.map(lambda j: np.save(args.save_root + "/%s.npy" % j[0], np.ascontiguousarray(j[1])), jobs))
        early.result()
    pool.shutdown()
    mdist.barrier()
    return select_points, select_ori, min_loss, high_conf_index


# ---- refine (PMVO.py:602-764)
REFINE_CHUNK = 5000                      # points per smoothing chunk (PMVO.py:602) and per batch of the sums over views
REFINE_K = 100                           # neighbours of a medoid (PMVO.py:605,660)
REPLACE_COS = 0.95                       # a direction less similar than this to its medoid is replaced (PMVO.py:625-640)
LOSS_STEP, LOSS_RANGE = 0.005, 4.0       # the depth step / range of the loss of a medoid direction (PMVO.py:619-623)


def _row(t, row, width=1):
    """Pointer to row `row` of a contiguous tensor with `width` elements per row."""
    return ctypes.c_void_p(t.data_ptr() + row * width * t.element_size())


def _stream_ptr(stream):
    return ctypes.c_void_p(stream.cuda_stream)


def _chunk_slices(n_all, chunk, ranks, rank):
    """(lo, hi, s, a, b) for every smoothing chunk: the chunk is rows [lo, hi) and `rank` of `ranks` owns [a, b), slice
    `rank` of width s = ceil((hi-lo)/ranks).  `step = n_all // chunk + 1` (PMVO.py:603): when n_all is a multiple of
    `chunk` there is a trailing chunk of no points.  A point's new orientation depends on the orientations as they were
    when its chunk started (PMVO.py:614,640), so the slices of a chunk are independent."""
    out = []
    for i in range(n_all // chunk + 1):
        lo, hi = i * chunk, min((i + 1) * chunk, n_all)
        s = -(-(hi - lo) // ranks)
        out.append((lo, hi, s, min(lo + rank * s, hi), min(lo + (rank + 1) * s, hi)))
    return out


def _row_offsets(slices):
    """row_of[i]: the first row of chunk i in a table that holds one row per owned point (prefix sums of b - a)."""
    return np.concatenate([[0], np.cumsum([b - a for _, _, _, a, b in slices])]).astype(np.int64).tolist()


def _loss_groups(step):
    """The chunk indices after which a loss launch of _smooth_chain closes: groups of 2, 4, 8, 8, ... chunks (short groups
    first, so that the side stream starts early) and a last one that ends with the last chunk."""
    closes, nxt, grp = [], 2, 2
    for i in range(step):
        if i + 1 == nxt or i == step - 1:
            closes.append(i)
            grp = min(grp * 2, 8)
            nxt = i + 1 + grp
    return closes


class _Writer:
    """np.save in the background while the caller goes on.  Every save() call is a batch of (path, array[, event to wait for
    first]) jobs that one thread of its own writes in order and then ends, so an error elsewhere leaves nothing waiting.  The
    first exception is kept, jobs that start after it are dropped, and join() re-raises it on the caller (once).
    enabled=False (not rank 0): nothing is written."""

    def __init__(self, enabled=True):
        self.enabled, self.threads, self.error = enabled, [], None

    def save(self, *jobs):
        if self.enabled:
            import threading

            self.threads.append(threading.Thread(target=self._run, args=(jobs,)))
            self.threads[-1].start()

    def _run(self, jobs):
        for path, array, *after in jobs:
            if self.error is None:
                try:
                    if after and after[0] is not None:
                        after[0].synchronize()           # (the copy that fills a pinned array)
                    np.save(path, array)
                except BaseException as e:
                    self.error = self.error or e

    def join(self):
        while self.threads:
            self.threads.pop().join()
        err, self.error = self.error, None
        if err is not None:
            raise err


def _knn(data_points, query_points, k, device, mode="device", int32=False, self_query=False, keep_grid=None):
    """The `KDTree(data).query(queries, k)` of refine (PMVO.py:605,612,660,671) -> index [Q,k] int64 tensor on `device`.
    mode "device": exact grid k-NN kernel (csrc/knn.hip, scipy's result and order); "host": scipy on all cores.
    scipy returns index n for missing neighbours when k > n (the reference would raise on ori[index]); k is clamped.
    keep_grid: a list that receives the GridKNN object (device mode), so that a later query of a subset can reuse it."""
    k = min(k, data_points.shape[0])
    if mode == "device":
        from .pmvo_utils import GridKNN

        g = GridKNN(data_points, k_hint=k, device=device)
        if keep_grid is not None:
            keep_grid.append(g)
        return g.query(query_points, k, int32=int32, self_query=self_query)
    from scipy.spatial import KDTree

    _, index = KDTree(data=data_points).query(query_points, k, workers=-1)
    index = np.asarray(index).reshape(len(query_points), k)
    return torch.from_numpy(index.astype(np.int32) if int32 else index).to(device)


def _smooth_chain(pmvo, pts_dev, ori_dev, loss_dev, index_all, head_all, head_top_all, main, side):
    """The smoothing loop of one rank (PMVO.py:602-643), in place in ori_dev / loss_dev.  Only the ORIENTATIONS chain from
    chunk to chunk (chunk k+1's medoids read what chunk k replaced, PMVO.py:614,640): medoid -> replacement rule, two small
    launches per chunk on `main`.  The loss of a chunk's medoid directions (PMVO.py:619-623) feeds nothing in later chunks
    and runs beside the chain on `side`, in the groups of _loss_groups as soon as their medoids exist (the batch arguments
    place every point in its 5000-point chunk of the reference's sums, include/mh_pmvo.h: mh_refine_loss_maps); one launch
    writes every loss at the end.  head_all: the head-filter votes of all points, queued on `side` by the caller.  Same
    kernels on the same values as the four-launches-per-chunk form (_smooth_sharded; tests compare the two bit for bit)."""
    L, ctx, device = pmvo._L, pmvo._ctx, pmvo.device
    n_all, K = int(pts_dev.shape[0]), int(index_all.shape[1])
    st, st2 = _stream_ptr(main), _stream_ptr(side)
    centers = torch.empty((n_all, 3), dtype=torch.float32, device=device)
    loss_all = torch.empty((n_all,), dtype=torch.float32, device=device)
    closes, g0 = _loss_groups(n_all // REFINE_CHUNK + 1), 0
    for i, (lo, hi, _, _, _) in enumerate(_chunk_slices(n_all, REFINE_CHUNK, 1, 0)):
        if hi > lo:
            _lib.check(L.mh_medoid_indexed(ctx, _lib.ptr(ori_dev), _row(index_all, lo, K), hi - lo, K, _row(centers, lo, 3),
                                           None, st), "mh_medoid_indexed")
            _lib.check(L.mh_replace_dissimilar(ctx, _row(centers, lo, 3), _row(ori_dev, lo, 3), REPLACE_COS, hi - lo, st),
                       "mh_replace_dissimilar")
        if i in closes and hi > g0:
            ev = torch.cuda.Event()
            ev.record(main)
            side.wait_event(ev)
            _lib.check(L.mh_refine_loss_maps(ctx, _row(pts_dev, g0, 3), _row(centers, g0, 3), LOSS_STEP, LOSS_RANGE, hi - g0,
                                             pmvo._side, float(pmvo.conf_threshold), _row(loss_all, g0), None, REFINE_CHUNK,
                                             g0, n_all, st2), "mh_refine_loss_maps")
            g0 = hi
    main.wait_stream(side)
    _lib.check(L.mh_refine_combine(ctx, _lib.ptr(centers), _lib.ptr(loss_all), _lib.ptr(head_all), _lib.ptr(head_top_all),
                                   REPLACE_COS, None, _lib.ptr(loss_dev), n_all, st), "mh_refine_combine")


def _smooth_sharded(pmvo, pts_dev, ori_dev, loss_dev, index_all, head_top_all, slices, ranks):
    """The smoothing loop with four launches per chunk and no tensor operation: medoid over the neighbour rows, the loss of
    that direction straight from the maps, the head-filter votes, and the tail (-1 / replacement / 0.5) in place.  With
    several ranks every rank runs its slice of a chunk (index_all holds the rows of the owned points only), then one in-place
    all_gather per array makes every rank's copy complete again: the arrays a rank holds at the start of a chunk are the
    single-rank ones, bit for bit."""
    from . import dist as mdist

    L, ctx, st, device = pmvo._L, pmvo._ctx, _lib.stream_ptr(), pmvo.device
    n_all, K = int(pts_dev.shape[0]), int(index_all.shape[1])
    center = torch.empty((REFINE_CHUNK, 3), dtype=torch.float32, device=device)
    loss_u = torch.empty((REFINE_CHUNK,), dtype=torch.float32, device=device)
    head = torch.empty((REFINE_CHUNK,), dtype=torch.uint8, device=device)
    row_of = _row_offsets(slices)
    for i, (lo, hi, s, a, b) in enumerate(slices):
        n = b - a
        if hi <= lo:
            continue
        if n > 0:
            _lib.check(L.mh_medoid_indexed(ctx, _lib.ptr(ori_dev), _row(index_all, row_of[i], K), n, K, _lib.ptr(center), None,
                                           st), "mh_medoid_indexed")
            _lib.check(L.mh_refine_loss_maps(ctx, _row(pts_dev, a, 3), _lib.ptr(center), LOSS_STEP, LOSS_RANGE, n, pmvo._side,
                                             float(pmvo.conf_threshold), _lib.ptr(loss_u), None, REFINE_CHUNK, a, n_all, st),
                       "mh_refine_loss_maps")
            _lib.check(L.mh_filter_points(ctx, _row(pts_dev, a, 3), n, pmvo._side, float(pmvo.conf_threshold),
                                          float(pmvo.visible_threshold), None, None, None, _lib.ptr(head), REFINE_CHUNK, a,
                                          n_all, st), "mh_filter_points")
            _lib.check(L.mh_refine_combine(ctx, _lib.ptr(center), _lib.ptr(loss_u), _lib.ptr(head), _row(head_top_all, a),
                                           REPLACE_COS, _row(ori_dev, a, 3), _row(loss_dev, a), n, st), "mh_refine_combine")
        if ranks > 1:
            mdist.all_gather_rows_inplace(ori_dev, lo, s)
            mdist.all_gather_rows_inplace(loss_dev, lo, s)


def _save_smoothed(writer, args, points, new_ori, new_loss, after=None):
    """The three files of PMVO.py:645-648, written in the background while the shell stage runs.  The reference reads them
    back right away (:650-652): the arrays in memory are what np.load would return."""
    if writer.enabled:
        os.makedirs(args.output_path + "/refine", exist_ok=True)
    root = args.output_path + "/refine/"
    writer.save((root + "select_p.npy", points), (root + "select_o.npy", new_ori, after), (root + "min_loss.npy", new_loss, after))


# What the steps of _refine_device share: the caller's stream, the side and copy streams; the number of points and of shell
# points; the points, orientations and losses on the device; optimize()'s prefetch (or None); the shell points as float32 and
# as the queries of their neighbour search, their head-filter votes and scalp test (None without shell points).
_DeviceState = collections.namedtuple("_DeviceState", "main side cp n_all F pts ori loss pf fb fq hd ht")


def _device_inputs(points, ori, loss, pmvo, filter_unvisible_points, args):
    """Uploads through pinned staging, the adoption of optimize()'s prefetch, and -- first thing on the side stream -- the
    head-filter votes and the scalp test of the shell points, which need the shell points only.  -> _DeviceState."""
    device = pmvo.device
    main, side = torch.cuda.current_stream(device), pmvo.aux_stream("refine_side")
    fu = np.ascontiguousarray(filter_unvisible_points) if filter_unvisible_points is not None else np.zeros((0, 3), np.float32)
    F = int(len(fu))
    with stage("refine: uploads + prefetch adoption", device):
        pts = pmvo.stage_upload("refine_p", np.asarray(points).reshape(-1, 3))
        ori_dev = pmvo.stage_upload("refine_o", np.asarray(ori).reshape(-1, 3))
        loss_dev = pmvo.stage_upload("refine_l", np.asarray(loss).reshape(-1))
        pf = pmvo.take_refine_prefetch(pts, REFINE_CHUNK, REFINE_K)
        # (what ran: tests, bench)
        pmvo.last_refine = {"device_pass": True, "prefetch_adopted": pf is not None, "shell_stage": "device"}
    fb = fq = hd = ht = None
    side.wait_stream(main)
    if F:
        with torch.cuda.stream(side):
            fb = pmvo.stage_upload("refine_fb", fu.reshape(-1, 3))                    # float32 (votes, scalp test, files)
            fq = pmvo.stage_upload("refine_fq", fu.reshape(-1, 3), np.float64) if fu.dtype == np.float64 else fb
            hd = torch.empty((F,), dtype=torch.uint8, device=device)
            _lib.check(pmvo._L.mh_filter_points(pmvo._ctx, _lib.ptr(fb), F, pmvo._side, float(pmvo.conf_threshold),
                                                float(args.PMVO.visible_threshold), None, None, None, _lib.ptr(hd),
                                                REFINE_CHUNK, 0, F, _lib.stream_ptr()), "mh_filter_points")
            ht = pmvo.head_top_mask_device(fb)
    return _DeviceState(main, side, pmvo.aux_stream("copy"), int(points.shape[0]), F, pts, ori_dev, loss_dev, pf, fb, fq, hd, ht)


def _device_neighbours(pmvo, d):
    """What the smoothing loop needs of the points alone -- optimize()'s prefetch, or made here -> (the spatial index of all
    points, the neighbour table, the head-filter votes (queued on the side stream), the scalp test)."""
    from . import pmvo_utils as U

    device, n_all = pmvo.device, d.n_all
    if d.pf is not None:
        return d.pf.grid, d.pf.index_all, d.pf.head_all, d.pf.head_top_all
    with stage("refine: knn (surface)", device):
        grid = U.GridKNN(d.pts, k_hint=REFINE_K, device=device)
        index_all = grid.query(d.pts, min(REFINE_K, n_all), int32=True, self_query=True).contiguous()
    with stage("refine: head-top mask", device):
        head_top_all = pmvo.head_top_mask_device(d.pts)
    head_all = torch.empty((n_all,), dtype=torch.uint8, device=device)
    d.side.wait_stream(d.main)
    with torch.cuda.stream(d.side):
        _lib.check(pmvo._L.mh_filter_points_ordered(pmvo._ctx, _lib.ptr(d.pts), n_all, pmvo._side, float(pmvo.conf_threshold),
                                                    float(pmvo.visible_threshold), None, None, None, _lib.ptr(head_all),
                                                    REFINE_CHUNK, 0, n_all, _lib.ptr(grid.cell_order()),
                                                    _lib.stream_ptr()), "mh_filter_points_ordered")
    return grid, index_all, head_all, head_top_all


def _start_result_copy(d):
    """The smoothed arrays travel to pinned host memory on the copy stream while the shell stage runs.
    -> (orientations, losses, event that ends the copy)."""
    ev_loop = torch.cuda.Event()
    ev_loop.record(d.main)
    ho = torch.empty((d.n_all, 3), dtype=torch.float32, pin_memory=True)
    hl = torch.empty((d.n_all,), dtype=torch.float32, pin_memory=True)
    ev_res = torch.cuda.Event()
    with torch.cuda.stream(d.cp):
        d.cp.wait_event(ev_loop)
        ho.copy_(d.ori, non_blocking=True)
        hl.copy_(d.loss, non_blocking=True)
        ev_res.record(d.cp)
    return ho.numpy(), hl.numpy(), ev_res


def _shell_device(pmvo, d, grid, threshold):
    """Loss threshold, shell points, concatenation (PMVO.py:651-693): flags and stable compactions, the host reads two
    counters.  -> (points [cap,3], orientations [cap,3], kept points, kept points + kept shell points), or None when the
    host-driven stage has to run: fewer kept points than neighbours (the reference then asks for that many)."""
    L, ctx, device, st, n_all, F = pmvo._L, pmvo._ctx, pmvo.device, _stream_ptr(d.main), d.n_all, d.F
    valid = torch.empty((n_all,), dtype=torch.uint8, device=device)
    _lib.check(L.mh_flag_less(ctx, _lib.ptr(d.loss), float(threshold), n_all, _lib.ptr(valid), st), "mh_flag_less")
    sel_p = torch.empty((n_all + F, 3), dtype=torch.float32, device=device)
    sel_o = torch.empty((n_all + F, 3), dtype=torch.float32, device=device)
    cnt = torch.zeros((2,), dtype=torch.int32, device=device)
    scratch = torch.empty(int(L.mh_select_scratch_bytes(max(n_all, F))), dtype=torch.uint8, device=device)
    _lib.check(L.mh_select_rows(ctx, _lib.ptr(valid), None, 0, n_all, _lib.ptr(d.pts), _lib.ptr(d.ori), _lib.ptr(sel_p),
                                _lib.ptr(sel_o), None, None, _row(cnt, 0), _lib.ptr(scratch), scratch.numel(), st),
               "mh_select_rows")
    hcnt = torch.empty((2,), dtype=torch.int32, pin_memory=True)
    hcnt[:1].copy_(cnt[:1], non_blocking=True)
    d.main.synchronize()                 # (1) the number of points the threshold keeps
    n_valid = int(hcnt[0])
    if not (F and n_valid):              # (no shell stage without kept points or without shell points, PMVO.py:658)
        d.main.wait_stream(d.side)
        return sel_p, sel_o, n_valid, n_valid
    if n_valid < min(REFINE_K, n_all):
        pmvo.last_refine["shell_stage"] = "host (fewer kept points than neighbours)"
        return None
    # KDTree(select_points).query(fu, 100) on the grid of ALL points with the kept ones flagged valid: the indices come back
    # in terms of `points` (order-preserving compaction: same (distance, index) order), so the medoid reads the full
    # orientation array (PMVO.py:660-672)
    idx, status = grid.query_nosync(d.fq, REFINE_K, valid_dev=valid)
    cen = torch.empty((F, 3), dtype=torch.float32, device=device)

    def shell_rows(first):
        """medoids of the table -> the shell rows that are kept = not filter_head_points = not (head votes and not under
        the scalp top) (PMVO.py:674-686), behind the kept points; a synchronisation brings their number (and, the first
        time, which queries the grid could not finish)."""
        _lib.check(L.mh_medoid_indexed(ctx, _lib.ptr(d.ori), _lib.ptr(idx), F, int(idx.shape[1]), _lib.ptr(cen), None, st),
                   "mh_medoid_indexed")
        if first:
            d.main.wait_stream(d.side)
        _lib.check(L.mh_select_rows(ctx, _lib.ptr(d.hd), _lib.ptr(d.ht), 1, F, _lib.ptr(d.fb), _lib.ptr(cen), _lib.ptr(sel_p),
                                    _lib.ptr(sel_o), None, _row(cnt, 0), _row(cnt, 1), _lib.ptr(scratch), scratch.numel(), st),
                   "mh_select_rows")
        if first:
            hst.copy_(status, non_blocking=True)
        hcnt[1:].copy_(cnt[1:], non_blocking=True)
        d.main.synchronize()

    hst = torch.empty((F,), dtype=torch.int32, pin_memory=True)
    shell_rows(True)                      # (2) kept shell rows; queries the grid could not finish at its first cell size
    if bool(hst.numpy().any()):
        # some shell points need another cell size (kept points sparser than the grid was laid out for): GridKNN's own
        # retries fix those rows of the table in place, then the medoids and the selection of the shell rows once more
        pmvo.last_refine["shell_stage"] = "device (%d queries retried on another cell size)" % int((hst.numpy() != 0).sum())
        grid.finish_nosync(d.fq, REFINE_K, idx, hst.numpy(), valid_dev=valid)
        shell_rows(False)
    return sel_p, sel_o, n_valid, int(hcnt[1])


def _fit_device(pmvo, d, sel, voxel_min, voxel_size, grid_resolution):
    """The kept shell rows travel to pinned host memory on the copy stream while the voxel fit (PMVO.py:695-726) runs on
    the concatenation.  -> (voxels, their orientations, shell points, shell orientations)."""
    from . import pmvo_utils as U

    sel_p, sel_o, n_valid, n_sel = sel
    hp = torch.empty((n_sel - n_valid, 3), dtype=torch.float32, pin_memory=True)
    hq = torch.empty((n_sel - n_valid, 3), dtype=torch.float32, pin_memory=True)
    ev_shell = torch.cuda.Event()
    with torch.cuda.stream(d.cp):
        d.cp.wait_stream(d.main)
        hp.copy_(sel_p[n_valid:n_sel], non_blocking=True)
        hq.copy_(sel_o[n_valid:n_sel], non_blocking=True)
        ev_shell.record(d.cp)
    with stage("refine: voxel fit + reduce", pmvo.device):
        vox, vori = U.voxel_fit_device(sel_p, sel_o, n_sel, pmvo.device, voxel_min, voxel_size, grid_resolution)
    ev_shell.synchronize()
    return vox, vori, hp.numpy(), hq.numpy()


def _refine_device(points, ori, loss, pmvo, filter_unvisible_points, args, threshold, voxel_min, voxel_size,
                   grid_resolution, writer):
    """The smoothing loop, the loss threshold, the shell points and the voxel fit of refine() (PMVO.py:602-726) on one rank
    with every array resident on the device from the first launch to the last: between the stages the host reads four
    counters, nothing else -- the `np.where` / `ori[index]` / `np.concatenate` steps of the reference are stable
    compactions on the device (mh_flag_less, mh_select_rows, mh_segment_heads), the neighbour table / head votes / scalp
    test of the points come from optimize()'s prefetch when it was made for these points, and the refine/*.npy files are
    written by `writer` from pinned copies while the shell stage and the fit run.  Same kernels on the same values in the
    same order as the host-driven form (_smooth_host; tests pin both to the reference's multi-chunk run).

    The smoothed result is stored into the caller's `ori` and `loss`.  -> (grid of all points, fit); fit = (voxels, their
    orientations, shell points, shell orientations), or None when the shell stage has to take the host path."""
    d = _device_inputs(points, ori, loss, pmvo, filter_unvisible_points, args)
    grid, index_all, head_all, head_top_all = _device_neighbours(pmvo, d)
    with stage("refine: smoothing loop", pmvo.device):
        _smooth_chain(pmvo, d.pts, d.ori, d.loss, index_all, head_all, head_top_all, d.main, d.side)
        new_ori, new_loss, ev_res = _start_result_copy(d)
        _save_smoothed(writer, args, points, new_ori, new_loss, after=ev_res)
    with stage("refine: shell points", pmvo.device):
        sel = _shell_device(pmvo, d, grid, threshold)
    fit = None if sel is None else _fit_device(pmvo, d, sel, voxel_min, voxel_size, grid_resolution)
    ev_res.synchronize()
    ori[:] = new_ori                     # in place, like the reference's chunk write-backs (PMVO.py:640-642)
    loss[:] = new_loss
    return grid, fit


def _adopt_mat_writer(pmvo, args, candidates, is_root, voxel_min, voxel_size, grid_resolution):
    """Ori3D.mat / Occ3D.mat are created NOW and their pages made resident in the background (every point that can end up in
    the volume is known: the surface points and the shell candidates); the occupied elements are stored at the end.  The
    writer optimize() started while its iterations ran is adopted if it is for this directory and grid, else aborted."""
    from . import pmvo_utils as U

    save_path = getattr(args, "save_path", "") or ""
    early, pmvo._mat_early = getattr(pmvo, "_mat_early", None), None
    if early is not None:
        if (is_root and early[0] == save_path and voxel_size == U.VOXEL_SIZE and np.array_equal(voxel_min, U.VOXEL_MIN)
                and np.array_equal(grid_resolution, U.GRID_RESOLUTION)):
            return early[1]
        early[1].abort()
    if not (is_root and os.path.isdir(save_path)):
        return None
    cands = [np.asarray(p_)[:, :3] for p_ in candidates if p_ is not None and len(p_)]
    return U.SparseMatWriter(args.save_path, grid_resolution, np.concatenate(cands, 0) if cands else None, voxel_min,
                             voxel_size)


def _device_pass_selected(points, args):
    """Device k-NN: the whole of PMVO.py:602-726 runs device-resident (_refine_device) -- on one rank, and on EVERY rank of
    a multi-rank run that does not shard refine (the default: no communication, rank 0 writes the files).
    MH_REFINE_DEVICE=0, MH_REFINE_SHARD=1, args.knn = "host" or MH_REFINE_CHAIN=0 take the host-driven forms (_smooth_host;
    tests pin all of them to the reference)."""
    from . import dist as mdist

    return ((mdist.world() == 1 or not mdist.refine_sharded()) and len(points) > 0
            and getattr(args, "knn", "device") == "device" and os.environ.get("MH_REFINE_DEVICE", "1") != "0"
            and os.environ.get("MH_REFINE_CHAIN", "1") != "0")


def _smooth_host(points, ori, loss, pmvo, args, writer, grid_all):
    """The host-driven forms of the smoothing loop, in place in `ori` and `loss`.  Neighbour indices and the head-top mask
    depend on the points only: ONE query for all chunks, then the sequentially dependent loop (chunk k+1 reads the
    orientations chunk k wrote, PMVO.py:614,640) runs on the device, stream-ordered, without a host round trip per chunk:
    _smooth_chain on one rank; _smooth_sharded with MH_REFINE_CHAIN=0, or with several ranks (mdist.refine_sharded), each of
    which queries the neighbours of the rows it owns only.  grid_all receives the spatial index of all points."""
    from . import dist as mdist

    device, n_all, knn = pmvo.device, points.shape[0], getattr(args, "knn", "device")
    R, rk = (mdist.world(), mdist.rank()) if mdist.refine_sharded() else (1, 0)
    slices = _chunk_slices(n_all, REFINE_CHUNK, R, rk)
    with stage("refine: knn (surface)", device):
        if R == 1:
            index_all = _knn(points, points, REFINE_K, device, knn, int32=True, self_query=True, keep_grid=grid_all)
        else:
            qidx = np.concatenate([np.arange(a, b) for _, _, _, a, b in slices])
            index_all = _knn(points, points[qidx], REFINE_K, device, knn, int32=True, keep_grid=grid_all)
        index_all = index_all.contiguous()
    with stage("refine: smoothing loop", device):
        pts_dev = torch.from_numpy(np.ascontiguousarray(points, dtype=np.float32)).to(device)
        with stage("refine: head-top mask", device):      # scalp half of filter_head_points, once for all chunks
            head_top_all = pmvo.head_top_mask_device(pts_dev)
        if R > 1:
            slack = R * (-(-REFINE_CHUNK // R))            # rows the in-place exchange may touch past the last chunk
            ori_dev = torch.zeros((n_all + slack, 3), dtype=torch.float32, device=device)
            loss_dev = torch.zeros((n_all + slack,), dtype=torch.float32, device=device)
            ori_dev[:n_all] = torch.from_numpy(ori).to(device).type(torch.float)
            loss_dev[:n_all] = torch.from_numpy(loss).to(device).type(torch.float)
        else:       # (one rank: no tensor operation beyond the upload -- first uses of torch kernels cost a one-shot run ~40 ms)
            ori_dev = torch.from_numpy(ori).to(device).type(torch.float).contiguous()
            loss_dev = torch.from_numpy(loss).to(device).type(torch.float).contiguous()
        if R == 1 and os.environ.get("MH_REFINE_CHAIN", "1") != "0":
            main, side = torch.cuda.current_stream(device), pmvo.side_streams(1)[0]
            head_all = torch.empty((n_all,), dtype=torch.uint8, device=device)
            side.wait_stream(main)
            _lib.check(pmvo._L.mh_filter_points(pmvo._ctx, _lib.ptr(pts_dev), n_all, pmvo._side, float(pmvo.conf_threshold),
                                                float(pmvo.visible_threshold), None, None, None, _lib.ptr(head_all),
                                                REFINE_CHUNK, 0, n_all, _stream_ptr(side)), "mh_filter_points")
            _smooth_chain(pmvo, pts_dev, ori_dev, loss_dev, index_all, head_all, head_top_all, main, side)
        else:
            _smooth_sharded(pmvo, pts_dev, ori_dev, loss_dev, index_all, head_top_all, slices, R)
        ori[:] = ori_dev[:n_all].cpu().numpy()
        loss[:] = loss_dev[:n_all].cpu().numpy()
    _save_smoothed(writer, args, points, ori, loss)        # (not written again before the join)


def _shell_block(pmvo, args, src, fb, row0, n_shell):
    """rows row0.. of the n_shell shell points -> device tensors (medoid orientation of the 100 nearest kept points [n,3],
    head-filter votes [n], head-top mask [n]).  The points are independent: one medoid launch and one vote launch for all of
    them (the reference's 5000-point chunks bound its memory -- and place a point in a batch of its sums over views, which
    the vote kernel is told: PMVO.py:662-672).  src = (orientations on the device, grid of all points, flags of the kept
    ones) or (orientations of the kept points on the device, None, the kept points): where the neighbours are searched."""
    device = pmvo.device
    ori_dev, grid, kept = src
    with stage("refine: knn (shell)", device):
        if grid is not None:
            idx = grid.query(fb, REFINE_K, int32=True, valid=kept).contiguous()
        else:
            idx = _knn(kept, fb, REFINE_K, device, getattr(args, "knn", "device"), int32=True).contiguous()
    fb_dev = torch.from_numpy(fb.astype(np.float32)).to(device).contiguous()
    F, K = idx.shape
    cen = torch.empty((F, 3), dtype=torch.float32, device=device)
    hd = torch.empty((F,), dtype=torch.uint8, device=device)
    _lib.check(pmvo._L.mh_medoid_indexed(pmvo._ctx, _lib.ptr(ori_dev), _lib.ptr(idx), F, K, _lib.ptr(cen), None,
                                         _lib.stream_ptr()), "mh_medoid_indexed")
    _lib.check(pmvo._L.mh_filter_points(pmvo._ctx, _lib.ptr(fb_dev), F, pmvo._side, float(pmvo.conf_threshold),
                                        float(args.PMVO.visible_threshold), None, None, None, _lib.ptr(hd), REFINE_CHUNK, row0,
                                        n_shell, _lib.stream_ptr()), "mh_filter_points")
    return cen, hd, pmvo.head_top_mask_device(fb_dev)


def _shell_packed(pmvo, args, src, cuts, fb, k):
    """_shell_block of rank k's rows as one tensor [n,4]: the medoid, and 1.0 where the point is not filter_head_points."""
    cen, hd, ht = _shell_block(pmvo, args, src, fb, cuts[k], cuts[-1])
    out = torch.empty((cen.shape[0], 4), dtype=torch.float32, device=pmvo.device)
    out[:, :3] = cen
    out[:, 3] = (~(hd.bool() & ~ht.bool())).to(torch.float32)
    return out


def _shell_sharded(pmvo, args, src, fu):
    """Block k of the shell points belongs to rank k; one all_gather of the results -> (medoids, kept mask) on the host."""
    import functools

    from . import dist as mdist

    W_ = mdist.world()
    cuts = [(len(fu) * k) // W_ for k in range(W_ + 1)]
    res = torch.cat(mdist.map_chunks([fu[cuts[k]:cuts[k + 1]] for k in range(W_)],
                                     functools.partial(_shell_packed, pmvo, args, src, cuts), pmvo.device,
                                     empty=lambda: torch.empty((0, 4), dtype=torch.float32, device=pmvo.device),
                                     with_index=True), 0).cpu().numpy()
    return res[:, :3], res[:, 3] > 0.5


def _shell_host(points, ori, index, filter_unvisible_points, pmvo, args, grid_all):
    """Orientation of the occluded shell points from their 100 nearest points among the kept ones, points[index]
    (PMVO.py:662-686) -> (shell points that are not filter_head_points, their orientations), float32 host arrays."""
    from . import dist as mdist

    if not (len(index) and len(filter_unvisible_points)):
        return np.zeros((0, 3), np.float32), np.zeros((0, 3), np.float32)
    fu = np.ascontiguousarray(filter_unvisible_points)
    if grid_all and grid_all[0].M == len(points):
        # KDTree(select_points).query(fu) on the grid that already exists for all points: the points kept by the loss
        # threshold are flagged valid, the indices come back in terms of `points` (order-preserving compaction: same
        # (distance, index) order), so the medoid reads the full orientation array
        valid = np.zeros(len(points), np.uint8)
        valid[index] = 1
        ori_rows, grid, kept = ori, grid_all[0], valid
    else:
        ori_rows, grid, kept = ori[index], None, points[index]
    src = (torch.from_numpy(np.ascontiguousarray(ori_rows, dtype=np.float32)).to(pmvo.device), grid, kept)
    if mdist.refine_sharded():
        centres, keep = _shell_sharded(pmvo, args, src, fu)
    else:
        # one rank: the three results go to the host as they are (no tensor operation: in a one-shot process every first
        # use of a torch kernel costs tens of milliseconds of code-object loading)
        cen, hd, ht = _shell_block(pmvo, args, src, fu, 0, len(fu))
        keep = ~np.logical_and(hd.cpu().numpy().astype(bool), ~ht.cpu().numpy().astype(bool))     # not filter_head_points
        centres = cen.cpu().numpy()
    return fu.astype(np.float32)[keep], np.ascontiguousarray(centres[keep])


def _fit_host(select_points, select_ori, device, voxel_min, voxel_size, grid_resolution):
    """Voxel fit (PMVO.py:695-726): every rank fits a disjoint slab of voxels and one reduce assembles the volume -- or,
    with several ranks and refine not sharded, every rank holds every point and fits the whole volume itself (no exchange,
    rank 0 writes).  The volume stays a list of occupied voxels."""
    from . import dist as mdist
    from . import pmvo_utils as U

    with stage("refine: voxel fit + reduce", device):
        if mdist.world() > 1 and not mdist.refine_sharded():
            res = U.voxel_fit(select_points, select_ori, device, voxel_min, voxel_size, grid_resolution, dense=False)
            return res["voxels"].cpu().numpy(), res["ori"].cpu().numpy()
        return mdist.voxel_fit_reduced(select_points, select_ori, device, voxel_min, voxel_size, grid_resolution, sparse=True)


def _finish_volume(vox, vori, pmvo, args, infer_inner, mat_writer, writer, is_root, voxel_min, voxel_size, grid_resolution):
    """The network's orientation merged in for points seen in <= 2 views (PMVO.py:733-751), Ori3D.mat / Occ3D.mat, and the
    end of every background write.  -> the voxel list that was written."""
    from . import dist as mdist
    from . import pmvo_utils as U

    if is_root and infer_inner:
        coarse_data = np.load(args.data.root + "/ours/raw.npy")
        unvisible_index = pmvo.compute_unvisible_points(
            torch.from_numpy(coarse_data[:, :3].astype(np.float32)).to(pmvo.device)).cpu().numpy()
        vox, vori, un_visible_points, unvisible_ori = U.merge_inner_points(vox, vori, coarse_data, unvisible_index,
                                                                           voxel_min, voxel_size, grid_resolution)
        np.save(os.path.join(args.save_path, "coarse.npy"), un_visible_points)
        np.save(os.path.join(args.save_path, "coarse_ori.npy"), unvisible_ori)
    if is_root:
        with stage("refine: Ori3D/Occ3D.mat", pmvo.device):
            if mat_writer is not None:
                mat_writer.finish(vox, vori)
            else:
                U.save_ori_occ_mat_sparse(args.save_path, grid_resolution, vox, vori)
    writer.join()
    mdist.barrier()
    return vox, vori


def refine(points, ori, loss, pmvo, filter_unvisible_points, args, infer_inner=True, threshold=0.001,
           genrate_ori_only=False, voxel_min=None, voxel_size=None, grid_resolution=None, return_dense=True):
    """PMVO.py:602-764: KNN-medoid smoothing (sequentially dependent 5000-point chunks, in place), threshold,
    orientations for the occluded shell points, voxel fit, Ori3D.mat / Occ3D.mat.
    Returns the dense (occ [X,Y,Z], ori [X,Y,Z,3]) float64 arrays of the reference (it returns nothing itself);
    return_dense=False skips building them (PMVO.py's command line does: the files are written from the voxel list).
    voxel_min/voxel_size/grid_resolution default to the reference's hard-coded 256x256x192 @ 2.5 mm grid.
    args.knn = "host" switches the neighbour queries back to scipy's KDTree (default: the device kernel)."""
    from . import dist as mdist
    from . import pmvo_utils as U

    voxel_min = U.VOXEL_MIN if voxel_min is None else np.asarray(voxel_min, dtype=np.float64)
    voxel_size = U.VOXEL_SIZE if voxel_size is None else voxel_size
    grid_resolution = U.GRID_RESOLUTION if grid_resolution is None else np.asarray(grid_resolution).astype(np.int32)
    volume = (voxel_min, voxel_size, grid_resolution)
    is_root = mdist.rank() == 0          # (several ranks: all compute, rank 0 writes)
    mat_writer = _adopt_mat_writer(pmvo, args, (points, filter_unvisible_points), is_root, *volume)
    writer = _Writer(enabled=is_root)    # refine/*.npy, written while the stages below run; over before refine() returns
    pmvo.last_refine = {"device_pass": False, "prefetch_adopted": False, "shell_stage": "host"}
    grid_all, fit = [], None             # (the spatial index of ALL points, which the host shell stage reuses)
    if genrate_ori_only:
        points, ori, loss = (np.load(args.output_path + "/refine/%s.npy" % n) for n in ("select_p", "select_o", "min_loss"))
    else:
        print("filter nosiy points...")
        if _device_pass_selected(points, args):
            grid, fit = _refine_device(points, ori, loss, pmvo, filter_unvisible_points, args, threshold, *volume, writer)
            grid_all.append(grid)
        else:
            _smooth_host(points, ori, loss, pmvo, args, writer, grid_all)
    print("compute points orientation near the surface... ")
    if fit is None:
        index = np.where(loss < threshold)[0]
        with stage("refine: shell points", pmvo.device):
            shell_points, shell_ori = _shell_host(points, ori, index, filter_unvisible_points, pmvo, args, grid_all)
        vox, vori = _fit_host(np.concatenate([points[index], shell_points], 0), np.concatenate([ori[index], shell_ori], 0),
                              pmvo.device, *volume)
    else:
        vox, vori, shell_points, shell_ori = fit
    writer.save((args.output_path + "/refine/filter_unvisible.npy", shell_points),
                (args.output_path + "/refine/filter_unvisible_ori.npy", shell_ori))
    vox, vori = _finish_volume(vox, vori, pmvo, args, infer_inner, mat_writer, writer, is_root, *volume)
    return U.dense_from_sparse(grid_resolution, vox, vori) if return_dense else None
