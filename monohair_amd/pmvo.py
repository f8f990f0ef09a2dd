"""class PMVO -- the host-side mirror of the reference's `PMVO.py::class PMVO` (lines 13-529) on top of
the HIP library (include/mh_pmvo.h).  Same constructor, same methods, same return shapes/dtypes; every
method is one or two C-ABI calls on torch-owned device buffers.  There is no CPU path in here: without a
GPU and libmhpmvo.so construction fails loudly.

State set by Compute_Visible_and_Ori (as in the reference, PMVO.py:369-376): self.visible [V,N],
self.Ori [V,N,2], self.Conf [V,N], self.mask [V,N], self.Ori_patch [V,N,P,2], self.Conf_patch [V,N,P].

The drivers that run it over a capture live in optimize.py (filter_negative_points, optimize) and refine.py (refine); the
reference keeps class and drivers in one module, so their names resolve here as well.
"""
import ctypes
import os
import warnings

import numpy as np
import torch

from . import _lib
from .camera import CAM_STRIDE, camera_records
from .optimize import RefinePrefetch, filter_negative_points, optimize  # noqa: F401
from .pmvo_utils import map_code_lut
from .refine import refine  # noqa: F401
from .refine import _Writer, _chunk_slices, _loss_groups, _row_offsets  # noqa: F401  (where a test module looked for them before the split)
from .transfer import Transfer


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
            _lib.check(self._L.mh_ctx_set_view_u8(self._ctx, i, _lib.host_ptr(rec), _lib.ptr(d),
                                                  d.shape[2] if d.dim() == 3 else 1, _lib.ptr(planes[0]),
                                                  _lib.ptr(planes[1]), _lib.ptr(planes[2]),
                                                  _lib.host_ptr(lut), st), "mh_ctx_set_view_u8")
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
        self._scratch_need = {}     # N -> bytes of the search scratch (constant per context)
        self._L = _lib.lib()
        h = ctypes.c_void_p()
        _lib.check(self._L.mh_ctx_create(self.device.index or 0, ctypes.byref(h)), "mh_ctx_create")
        self._ctx = h
        self.transfer = Transfer(h, self.device)      # pinned staging buffers, their events, this object's streams
        self.set_num_sample(self.NUM_SAMPLE)
        self._scratch = None
        self.bust_tree = self.scalp_tree = self.scalp_max = None
        self.base_view_override = None

    def set_num_sample(self, num_sample):
        """The sample count of forward()'s search (the reference's default argument of sample_next_3d_pos, PMVO.py:263) on
        this object: NUM_SAMPLE and the context's depth offsets.  The search takes up to 256 samples and, with the len(RANKS)
        base-view ranks, up to 1024 (rank, sample) items (include/mh_pmvo.h)."""
        offs = depth_offsets(int(num_sample))
        _lib.check(self._L.mh_ctx_set_depth_offsets(self._ctx, _lib.host_ptr(offs), len(offs)),
                   "mh_ctx_set_depth_offsets")
        self.NUM_SAMPLE = len(offs)

    def _alloc(self, V, H, W):
        self.num_view = V
        _lib.check(self._L.mh_ctx_alloc_views(self._ctx, V, H, W), "mh_ctx_alloc_views")

    def _set_view(self, i, rec, d, ds, o, c, m, ms, st):
        rec = np.ascontiguousarray(rec, dtype=np.float32)
        _lib.check(self._L.mh_ctx_set_view(self._ctx, i, _lib.host_ptr(rec), _lib.ptr(d), ds,
                                           _lib.ptr(o), _lib.ptr(c), _lib.ptr(m), ms, st), "mh_ctx_set_view")
        # the pack kernel reads d/o/c/m asynchronously: keep them alive until it has run
        torch.cuda.current_stream().synchronize()

    def __del__(self):
        # an object dropped with uploads in flight must not release its pinned buffers under them (transfer.py)
        try:
            self.transfer.drain()
        except Exception:
            pass
        try:
            if getattr(self, "_ctx", None):
                self._L.mh_ctx_destroy(self._ctx)
                self._ctx = None
        except Exception:
            pass

    LAB_OPTIONS = ("search_variant", "search_body", "tap_plane", "tap_codes", "taps_tile", "filter_rows", "carve_early_exit")

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
            return self.transfer.upload_ring(points)
        return points.to(self.device).type(torch.float).contiguous()

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
        return [self.transfer.stream("side%d" % i) for i in range(n)]

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
            points = self.transfer.upload_ring(points, cs) if isinstance(points, np.ndarray) else self._dev_points(points)
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
