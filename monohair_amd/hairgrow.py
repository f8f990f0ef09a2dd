"""Strand tracing on the fitted orientation/occupancy volume -- host-side mirror of the tracing half of the
reference's `HairGrow.py::class HairGrowing` (__init__ :41-55, trace :59-149, traceFromScalp :154-223,
GenerateGuideStrandFromScalp :226-265, randomlyGenerateSegments :269-299, VoxelToWorld :816-824), the immediate
consumer of Ori3D.mat / Occ3D.mat, and the segment connection that follows it
(find_connect_info :434-590 with connect_segments :303-420, the connect_segments stage of __main__ :925-952), and the
scalp attachment that ends the pipeline (connect_to_scalp :606-812, WorldToVoxel :826-835, the connect_scalp stage of
__main__ :954-976, csrc/hairscalp.hip), and the scalp samples the whole stage starts from (__main__ :880-897,
csrc/meshsample.hip), and the scalp-diffused volumes the stage reads when `scalp_diffusion` is set (diffusion_scalp of
Utils/PMVO_utils.py:467-593, csrc/hairdiffuse.hip).

All seeds are traced in parallel by the HIP kernels of csrc/hairgrow.hip; the sequential `flag` gate only decides
which finished traces are kept and is replayed afterwards (mh_strands_accept).  The jitter of every trace() call
comes from torch's CPU generator in the order the reference draws it, so a seeded run reproduces the reference's
CPU path bit for bit."""
import ctypes
import os
import types

import numpy as np
import torch

from . import _lib
from ._lib import host_ptr
from .pmvo_utils import (VOXEL_SIZE, get_ground_truth_3D_occ, get_ground_truth_3D_ori, load_strand,
                         points_to_voxel, read_obj_normals, save_hair_strands, save_volume_mat_sparse, voxel_to_points)
from .strand_smooth import pack_strands, smooth_strands, split_strands, strand_offsets

_KNN_K = 50                                                      # k of the reference's end queries
_VMIN64 = np.array([-0.32, -0.32, -0.24], np.float32).astype(np.float64)   # points_to_voxel's float32 voxel_min
_TYPES = ("root", "tip")
_OUTSIDE = "%s indexes outside the occupancy volume (the reference's torch indexing raises IndexError here)"


def _td(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def grid_dims(extent, radius, slack, n):
    """(h, dims) of a uniform grid over n points spanning `extent` (float64 [3], from the grid's origin): cells of radius *
    slack, so that everything within the radius of a point lies in the 27 cells around its own, doubled while there would
    be more than max(4n, 2^20) of them."""
    h = radius * slack
    while True:
        dims = np.floor(extent / h).astype(np.int64) + 1
        if int(np.prod(dims)) <= max(4 * n, 1 << 20):
            return h, [int(d) for d in dims]
        h *= 2.0


def _occ_eval_host(ss, occ_h):
    """One attempt of the occupancy test (HairGrow.py:517-528) on the host: 1 accepted, 0 rejected, 2 outside the
    reference's fixed box; raises where torch's indexing would."""
    p = ss.copy()
    p[:, 1:] *= -1
    idx = np.rint((p - _VMIN64) / VOXEL_SIZE).astype(np.int64)
    if idx[:, 2].max() >= 192 or (idx[:, 1] >= 256).any() or (idx[:, 0] >= 256).any():
        return 2
    Z, H, W = occ_h.shape
    if (idx < -np.array([W, H, Z])).any() or (idx >= np.array([W, H, Z])).any():
        raise _lib.MhError(_OUTSIDE % "find_connect_info: a strand")
    v = occ_h[idx[:, 2], idx[:, 1], idx[:, 0]]
    return 1 if np.float32(v.sum(dtype=np.float32)) / np.float32(v.shape[0]) > np.float32(0.8) else 0


class HairGrowing:
    def __init__(self, occ_path, ori_path, device="cuda:0", image_size=[1120, 1992], occ=None, ori=None):
        """occ_path/ori_path: Occ3D.mat / Ori3D.mat as PMVO writes them; or pass the readers' arrays directly
        (occ [Z,Y,X,1], ori [Z,Y,X,3])."""
        if not torch.cuda.is_available():
            raise _lib.MhError("HairGrowing needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device(device)
        self.image_size = image_size
        occ = get_ground_truth_3D_occ(occ_path) if occ is None else np.asarray(occ, np.float32)
        ori = get_ground_truth_3D_ori(ori_path) if ori is None else np.asarray(ori, np.float32)
        occ_t = torch.from_numpy(np.ascontiguousarray(occ[..., 0])).to(self.device).float()          # [Z,H,W]
        ori_t = torch.from_numpy(np.ascontiguousarray(ori)).to(self.device).float()                  # [Z,H,W,3]
        self.Z, self.H, self.W = occ_t.shape
        self._ctx = _lib.bare_ctx(self.device)
        self._vox = torch.empty((self.Z, self.H, self.W, 4), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mh_volume_pack(self._ctx, _lib.ptr(occ_t), _lib.ptr(ori_t), self.W, self.H, self.Z,
                                                 _lib.ptr(self._vox), _lib.stream_ptr()), "mh_volume_pack")
        # attribute surface of the reference (HairGrow.py:49-55)
        self.occ = self._vox[..., 3][None]                        # [1,Z,H,W]
        self.ori = self._vox[..., :3].permute(3, 0, 1, 2)         # [3,Z,H,W], y/z negated
        self.strands = None

    # ------------------------------------------------------------------ kernels
    def _trace_scalp(self, pts, nrm, thr):
        n = pts.shape[0]
        out = torch.empty((n, 257, 3), dtype=torch.float32, device=self.device)
        ln = torch.empty((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mh_trace_scalp(self._ctx, _lib.ptr(self._vox), self.W, self.H, self.Z, _lib.ptr(pts),
                                                 _lib.ptr(nrm), n, float(thr), _lib.ptr(out), _lib.ptr(ln),
                                                 _lib.stream_ptr()), "mh_trace_scalp")
        return out, ln

    def _trace_seeds(self, seeds, thr):
        n = seeds.shape[0]
        out = torch.empty((n, 513, 3), dtype=torch.float32, device=self.device)
        first = torch.empty((n,), dtype=torch.int32, device=self.device)
        ln = torch.empty((n,), dtype=torch.int32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mh_trace_seeds(self._ctx, _lib.ptr(self._vox), self.W, self.H, self.Z,
                                                 _lib.ptr(seeds), n, float(thr), _lib.ptr(out), _lib.ptr(first),
                                                 _lib.ptr(ln), _lib.stream_ptr()), "mh_trace_seeds")
        return out, first, ln

    def _accept(self, flag, pts, first, ln, seeds, mode):
        """sequential flag gate on the host over finished traces -> list of [L,3] numpy strands.  The fixed-stride rows
        (513 / 257 points per seed, mostly empty: 1.3 GB for 215 k seeds) are packed on the device first
        (mh_strands_compact), so only the points that exist cross PCIe."""
        n, stride = pts.shape[0], pts.shape[1]
        first_h = np.ascontiguousarray(first.cpu().numpy(), dtype=np.int32)
        ln_h = np.ascontiguousarray(ln.cpu().numpy(), dtype=np.int32)
        seeds_h = np.ascontiguousarray(seeds.cpu().numpy(), dtype=np.float32)
        offs_h = strand_offsets(np.maximum(ln_h, 0))
        total = int(offs_h[-1])
        packed = torch.empty((max(total, 1), 3), dtype=torch.float32, device=self.device)
        with torch.cuda.device(self.device):
            _lib.check(_lib.lib().mh_strands_compact(self._ctx, _lib.ptr(pts), _lib.ptr(first.contiguous()),
                                                     _lib.ptr(ln.contiguous()), _lib.ptr(torch.from_numpy(offs_h).to(self.device)),
                                                     n, stride, _lib.ptr(packed), _lib.stream_ptr()), "mh_strands_compact")
        pts_h = np.ascontiguousarray(packed.cpu().numpy())
        assert total < 2 ** 31
        offs32 = offs_h.astype(np.int32)
        acc = np.zeros(n, np.uint8)
        _lib.check(_lib.lib().mh_strands_accept(self.W, self.H, self.Z, host_ptr(flag), host_ptr(pts_h), host_ptr(offs32),
                                                host_ptr(ln_h), 0, host_ptr(seeds_h), n, mode, host_ptr(acc)), "mh_strands_accept")
        return split_strands(pts_h, offs_h, np.flatnonzero(acc))

    def _voxel_rounds(self, flag, thrDot, rounds):
        """`rounds` passes of trace() over the occupied voxels.  The reference shifts its seed tensor IN PLACE on
        every call (HairGrow.py:62-63: += 0.5, += rand*0.5), so the shifts accumulate from round to round."""
        positive = torch.nonzero(self.occ[0], as_tuple=False)
        pos = torch.flip(positive, dims=[1]).type(torch.float)                        # (x,y,z)
        n = pos.shape[0]
        jitter = torch.rand(rounds * n, 3).to(self.device)       # CPU generator, the reference's draw order
        seeds = []
        for r in range(rounds):
            pos = pos + 0.5
            pos = pos + jitter[r * n:(r + 1) * n] * 0.5
            seeds.append(pos)
        seeds = torch.cat(seeds, 0).contiguous()
        out, first, ln = self._trace_seeds(seeds, thrDot)
        return self._accept(flag, out, first, ln, seeds, 0)

    def _to_device_views(self, strands_np):
        if not strands_np:
            return []
        cat = torch.from_numpy(np.concatenate(strands_np, 0)).to(self.device)
        return list(torch.split(cat, [s.shape[0] for s in strands_np]))

    # ------------------------------------------------------------------ reference methods
    def trace(self, seedPos, flag, thrDot, W=None, H=None, Z=None):
        """HairGrow.py:59-149 for ONE seed (the drivers above trace all seeds in one launch instead): shifts seedPos in
        place by 0.5 and by rand*0.5 like the reference, reads `flag` ([Z,H,W] tensor or array) at the seed only, and
        returns the strand [L,3] (L >= 5) or False."""
        seedPos += torch.tensor([0.5, 0.5, 0.5], dtype=torch.float, device=seedPos.device)
        seedPos += torch.rand_like(seedPos) * 0.5
        x, y, z = (min(max(int(v), 0), hi - 1) for v, hi in zip(seedPos.tolist(), (self.W, self.H, self.Z)))
        if float(flag[z, y, x]) >= 3:
            return False
        out, first, ln = self._trace_seeds(seedPos.to(self.device).type(torch.float)[None].contiguous(), thrDot)
        n, f = int(ln[0]), int(first[0])
        return out[0, f:f + n].clone() if n >= 5 else False

    def traceFromScalp(self, seedPos, seedNormal, thrDot, W=None, H=None, Z=None, pointsTree=None):
        """HairGrow.py:154-223 for ONE root: the strand [L,3], or None when it grows into the head."""
        out, ln = self._trace_scalp(seedPos.to(self.device).type(torch.float)[None].contiguous(),
                                    seedNormal.to(self.device).type(torch.float)[None].contiguous(), thrDot)
        n = int(ln[0])
        return out[0, :n].clone() if n > 0 else None

    def GenerateGuideStrandFromScalp(self, scalp_points, scalp_normals, pointsTree=None, thrDot=0.8):
        """HairGrow.py:226-265 -> (strands: list of [L,3] device tensors in voxel space, num_root)."""
        flag = np.zeros((self.Z, self.H, self.W), np.float32)
        sp = scalp_points.to(self.device).type(torch.float).contiguous()
        sn = scalp_normals.to(self.device).type(torch.float).contiguous()
        out, ln = self._trace_scalp(sp, sn, thrDot)
        roots = self._accept(flag, out, torch.zeros_like(ln), ln, sp, 1)
        num_root = len(roots)
        strands = roots + self._voxel_rounds(flag, thrDot, 2)
        self.strands = self._to_device_views(strands)
        return self.strands, num_root

    def randomlyGenerateSegments(self, thrDot=0.8):
        """HairGrow.py:269-299."""
        flag = np.zeros((self.Z, self.H, self.W), np.float32)
        self.strands = self._to_device_views(self._voxel_rounds(flag, thrDot, 3))
        return self.strands

    # ------------------------------------------------------------------ find_connect_info, step by step
    def _end_tables(self, pts, offs, thr):
        """The four KDTree queries of HairGrow.py:440-470, k = 50 within thr: root->roots, root->tips, tip->roots, tip->tips
        as (index [N,50], float64 distance, count) on a float64 grid over all 2N ends, binned on the host."""
        N, dev = len(offs) - 1, self.device
        ends = np.concatenate([pts[offs[:-1]], pts[offs[1:] - 1]], 0)             # roots, then tips
        lo = ends.min(0)
        h, dims = grid_dims(ends.max(0) - lo, thr, 1.0001, 2 * N)
        cells = np.floor((ends - lo) / h).astype(np.int32)
        lin = (cells[:, 2].astype(np.int64) * dims[1] + cells[:, 1]) * dims[0] + cells[:, 0]
        ncell = dims[0] * dims[1] * dims[2]
        ends_d, qcell_d, grids = [], [], []
        for t in range(2):          # 0: the roots' tree, 1: the tips'
            l = lin[t * N:(t + 1) * N]
            cstart = np.zeros(ncell + 1, np.int32)
            np.cumsum(np.bincount(l, minlength=ncell), out=cstart[1:])
            grids.append((_td(np.argsort(l, kind="stable").astype(np.int32), dev), _td(cstart, dev)))
            ends_d.append(_td(ends[t * N:(t + 1) * N], dev))
            qcell_d.append(_td(cells[t * N:(t + 1) * N], dev))
        lists = []
        for qe, te in ((0, 0), (0, 1), (1, 0), (1, 1)):
            idx = torch.empty((N, _KNN_K), dtype=torch.int32, device=dev)
            dist = torch.empty((N, _KNN_K), dtype=torch.float64, device=dev)
            cnt = torch.empty((N,), dtype=torch.int32, device=dev)
            _lib.check(_lib.lib().mh_end_knn64(self._ctx, _lib.ptr(ends_d[qe]), _lib.ptr(qcell_d[qe]), N,
                                               _lib.ptr(ends_d[te]), _lib.ptr(grids[te][0]), _lib.ptr(grids[te][1]),
                                               dims[0], dims[1], dims[2], thr, 1, _lib.ptr(idx), _lib.ptr(dist),
                                               _lib.ptr(cnt), _lib.stream_ptr()), "mh_end_knn64")
            lists.append((idx, dist, cnt))
        return lists

    def _connect_candidates(self, pts_d, offs_d, N, dot_thr):
        """find_best_connect_strands (HairGrow.py:550-590) for both ends of every segment -> best, type ([2N] int32)."""
        arr = lambda k: (ctypes.c_void_p * 4)(*[l[k].data_ptr() for l in self._end_lists])   # noqa: E731
        best = torch.empty((2 * N,), dtype=torch.int32, device=self.device)
        btype = torch.empty((2 * N,), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().mh_connect_candidates(self._ctx, _lib.ptr(pts_d), _lib.ptr(offs_d), N, arr(0), arr(1), arr(2),
                                                    dot_thr, _lib.ptr(best), _lib.ptr(btype), _lib.stream_ptr()),
                   "mh_connect_candidates")
        return best, btype

    def _connect_chains(self, pts_d, offs_d, N, best, btype):
        """connect_segments (HairGrow.py:303-420): every segment grown along its joins -> (points float64, offsets)."""
        L, dev = _lib.lib(), self.device
        total = torch.empty((N,), dtype=torch.int64, device=dev)
        rootlen = torch.empty((N,), dtype=torch.int64, device=dev)
        _lib.check(L.mh_chain_count(self._ctx, _lib.ptr(offs_d), N, _lib.ptr(best), _lib.ptr(btype), _lib.ptr(total),
                                    _lib.ptr(rootlen), _lib.stream_ptr()), "mh_chain_count")
        ooffs = torch.zeros((N + 1,), dtype=torch.int64, device=dev)
        torch.cumsum(total, 0, out=ooffs[1:])
        out = torch.empty((int(ooffs[-1]), 3), dtype=torch.float64, device=dev)
        _lib.check(L.mh_chain_emit(self._ctx, _lib.ptr(pts_d), _lib.ptr(offs_d), N, _lib.ptr(best), _lib.ptr(btype),
                                   _lib.ptr(rootlen), _lib.ptr(ooffs), _lib.ptr(out), _lib.stream_ptr()), "mh_chain_emit")
        return out, ooffs

    def _occ_status(self, out, ooffs, N, occ_v):
        """Attempt 0 of the occupancy test (HairGrow.py:517-528) of every chain on occ_v, a [Z,H,W] view of the volume:
        int32 [N], 1 accepted, 0 rejected, 2 outside the reference's box, 3 an index torch refuses."""
        Z, H, W = occ_v.shape
        status = torch.empty((N,), dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().mh_occ_check(self._ctx, _lib.ptr(out), _lib.ptr(ooffs), N, _lib.ptr(occ_v),
                                           occ_v.stride(-1), W, H, Z, float(_VMIN64[0]), float(_VMIN64[1]),
                                           float(_VMIN64[2]), VOXEL_SIZE, _lib.ptr(status), _lib.stream_ptr()),
                   "mh_occ_check")
        return status

    def _occ_retries(self, chains, status, occ_v):
        """The retry loop of HairGrow.py:514-544 for the chains attempt 0 rejected, on the host in segment order with
        np.random's global generator, exactly as the reference draws -> (strands, number that failed)."""
        occ_h, fail = None, 0
        for i, st in enumerate(status):
            if st == 3:
                raise _lib.MhError(_OUTSIDE % "find_connect_info: a strand")
            if st == 0:
                if occ_h is None:
                    occ_h = occ_v.cpu().numpy()
                for count in range(1, 51):
                    ss = chains[i].copy()
                    ss += np.random.random((3)) * 0.005
                    if count >= 50:
                        break
                    st = _occ_eval_host(ss, occ_h)
                    if st == 1:
                        chains[i] = ss
                    if st != 0:
                        break
            fail += st != 1
        return chains, int(fail)

    def find_connect_info(self, strands, connect_threshold=0.005, connect_dot_threshold=0.7, occ=None):
        """HairGrow.py:434-547: joins the segments (list of float64 [L,3] arrays in world units, L >= 2) into strands and
        returns them.  occ: [1,Z,H,W] occupancy (0/1 values) or None for the solver's own.  The connection table is left
        in self.connect_info (the reference's strands_connect_info: per segment {'root': [j, 'root'|'tip'] or None,
        'tip': ...}), the failure count in self.connect_fail.  Strands that fail the first occupancy test are retried on
        the host in segment order with np.random's global generator, exactly as the reference draws."""
        N = len(strands)
        self.connect_info, self.connect_fail = [], 0
        if N == 0:
            return []
        thr = float(connect_threshold)
        if not (thr > 0 and np.isfinite(thr)):
            raise _lib.MhError("find_connect_info: connect_threshold must be positive and finite")
        pts, offs = pack_strands(strands, np.float64, "find_connect_info", finite=True)
        if occ is None:
            occ_v = self.occ[0]                       # channel 3 of the packed voxels
        else:
            occ_v = torch.as_tensor(occ).to(self.device).float().contiguous()
            occ_v = occ_v.reshape((-1,) + tuple(occ_v.shape[-3:]))[0]
        with torch.cuda.device(self.device):
            pts_d, offs_d = _td(pts, self.device), _td(offs, self.device)
            self._end_lists = self._end_tables(pts, offs, thr)
            best, btype = self._connect_candidates(pts_d, offs_d, N, float(connect_dot_threshold))
            out, ooffs = self._connect_chains(pts_d, offs_d, N, best, btype)
            status = self._occ_status(out, ooffs, N, occ_v).cpu().numpy()
            chains = split_strands(out.cpu().numpy(), ooffs.cpu().numpy())
            best_h, btype_h = best.cpu().numpy().reshape(N, 2), btype.cpu().numpy().reshape(N, 2)
        self.connect_best, self.connect_best_type = best_h, btype_h
        self.connect_info = [{e: (None if best_h[i, k] < 0 else [int(best_h[i, k]), _TYPES[btype_h[i, k]]])
                              for k, e in enumerate(_TYPES)} for i in range(N)]
        new_strands, self.connect_fail = self._occ_retries(chains, status, occ_v)
        return new_strands

    # ------------------------------------------------------------------ connect_to_scalp, step by step
    def _scalp_core(self, s):
        """The core set of a pass (HairGrow.py:620-640): the points of the strands rooted so far, the strand of each, and
        the position of each in KDTree(core).indices -- the order in which query_ball_point returns a ball."""
        from scipy.spatial import KDTree

        n, dev = s.flags.shape[0], self.device
        pid = torch.repeat_interleave(torch.arange(n, device=dev), s.offs[1:] - s.offs[:-1])
        sel = (s.flags[pid] & 1) != 0
        c = types.SimpleNamespace(pts=s.P[sel].contiguous(), sid=pid[sel].to(torch.int32), grid_thr=None)
        core_h = c.pts.cpu().numpy()
        c.M = core_h.shape[0]
        rank_h = np.empty(c.M, np.int32)
        rank_h[KDTree(core_h).indices] = np.arange(c.M, dtype=np.int32)
        c.rank = torch.from_numpy(rank_h).to(dev)
        c.lo, c.hi = core_h.min(0), core_h.max(0)
        c.scratch = torch.empty(int(_lib.lib().mh_grid_scratch_bytes(c.M)), dtype=torch.uint8, device=dev)
        c.order = torch.empty(c.M, dtype=torch.int32, device=dev)
        return c

    def _scalp_grid(self, c, thr_dist):
        """The grid of the core points for balls of radius thr_dist: cells a little larger than the radius (the cell of a
        point is a float32 floor) over the float32 extent."""
        h, dims = grid_dims((c.hi - c.lo).astype(np.float64), thr_dist, 1.01, c.M)
        c.grid = np.array([c.lo[0], c.lo[1], c.lo[2], h], np.float32)
        c.dims = np.array(dims, np.int32)
        c.cstart = torch.empty(int(np.prod(dims)) + 1, dtype=torch.int32, device=self.device)
        _lib.check(_lib.lib().mh_grid_build(self._ctx, host_ptr(c.grid), host_ptr(c.dims), _lib.ptr(c.pts), c.M,
                                            _lib.ptr(c.scratch), c.scratch.numel(), None, _lib.ptr(c.order), _lib.ptr(c.cstart),
                                            None, _lib.stream_ptr()), "mh_grid_build")
        c.grid_thr = thr_dist

    def _scalp_pass(self, s, c, act, thr_dist, thr_dot, out_ratio):
        """One pass of the reference's loop body over the floating strands `act` (the three kernels of
        csrc/hairscalp.hip); flags, out_ratio, similar, flips and choice of `s` are updated in place.
        -> (points, offsets after the joins, newly rooted, newly out, strands torch's indexing would refuse)."""
        L, ctx, dev, st = _lib.lib(), self._ctx, self.device, _lib.stream_ptr()
        n, nact = s.flags.shape[0], int(act.shape[0])
        bcnt = torch.empty(nact, dtype=torch.int64, device=dev)
        _lib.check(L.mh_scalp_ball_count(ctx, _lib.ptr(s.P), _lib.ptr(s.offs), _lib.ptr(act), nact, _lib.ptr(c.pts), c.M,
                                         _lib.ptr(c.order), _lib.ptr(c.cstart), host_ptr(c.grid), host_ptr(c.dims), thr_dist,
                                         _lib.ptr(bcnt), st), "mh_scalp_ball_count")
        boff = torch.zeros(nact + 1, dtype=torch.int64, device=dev)
        torch.cumsum(bcnt, 0, out=boff[1:])
        bscr = torch.empty(max(int(boff[-1]), 1), dtype=torch.int64, device=dev)
        flip = torch.zeros(n, dtype=torch.uint8, device=dev)
        bsid = torch.full((n,), -1, dtype=torch.int32, device=dev)
        bidx = torch.zeros(n, dtype=torch.int32, device=dev)
        _lib.check(L.mh_scalp_choose(ctx, _lib.ptr(s.P), _lib.ptr(s.offs), _lib.ptr(act), nact, _lib.ptr(c.pts),
                                     _lib.ptr(c.sid), _lib.ptr(c.rank), c.M, _lib.ptr(c.order), _lib.ptr(c.cstart),
                                     host_ptr(c.grid), host_ptr(c.dims), thr_dist, thr_dot, _lib.ptr(s.oratio), _lib.ptr(boff),
                                     _lib.ptr(bscr), _lib.ptr(flip), _lib.ptr(bsid), _lib.ptr(bidx), st), "mh_scalp_choose")
        joined = bsid >= 0
        newlen = (s.offs[1:] - s.offs[:-1]) + torch.where(joined, bidx.long() + 1, torch.zeros_like(bidx).long())
        noffs = torch.zeros(n + 1, dtype=torch.int64, device=dev)
        torch.cumsum(newlen, 0, out=noffs[1:])
        Pn = torch.empty((int(noffs[-1]), 3), dtype=torch.float32, device=dev)
        counters = torch.zeros(3, dtype=torch.int32, device=dev)
        _lib.check(L.mh_scalp_emit(ctx, _lib.ptr(s.P), _lib.ptr(s.offs), n, _lib.ptr(flip), _lib.ptr(bsid), _lib.ptr(bidx),
                                   _lib.ptr(noffs), _lib.ptr(self._vox), self.W, self.H, self.Z, float(out_ratio),
                                   _lib.ptr(Pn), _lib.ptr(s.flags), _lib.ptr(s.oratio), _lib.ptr(s.similar),
                                   _lib.ptr(counters), st), "mh_scalp_emit")
        s.flips += flip
        s.choice[joined] = torch.stack([bsid, bidx], 1)[joined]
        return (Pn, noffs) + tuple(int(v) for v in counters.cpu())

    def connect_to_scalp(self, strands, num_root, out_ratio, infer_inner=False):
        """HairGrow.py:606-784: attaches the floating strands (strands[num_root:], float32 [L,3] in voxel units, L >= 2) to
        strands that are rooted, pass after pass, and returns the rooted and the "out" strands in index order.  out_ratio:
        the reference's args.HairGenerate.out_ratio (the occupied fraction a join must exceed).  infer_inner only selects
        the same thresholds again in the reference.  Each pass is three kernels over all floating strands
        (csrc/hairscalp.hip); the host builds ONE scipy KDTree per change of the rooted set, for the order in which
        query_ball_point returns its members, and reads three counters per pass.  Left behind: self.scalp_passes (per
        pass: thr_dist, thr_dot, rooted and out counts after it), self.scalp_root_flag / scalp_out_flag /
        scalp_out_ratio / scalp_flips (times reversed) / scalp_choice ([n,2]: last neighbour and point index joined, -1
        none) / scalp_similar (random_move_strands' orientation score of that join)."""
        pts_h, offs_h = pack_strands(strands, np.float32, "connect_to_scalp", finite=True)
        n, num_root, dev = len(strands), int(num_root), self.device
        if n == 0 or num_root <= 0:
            raise _lib.MhError("connect_to_scalp: no rooted strand (the reference's np.concatenate of an empty core list "
                               "raises here)")
        flags_h = np.zeros(n, np.uint8)
        flags_h[:num_root] = 1
        s = types.SimpleNamespace(P=_td(pts_h, dev), offs=_td(offs_h, dev), flags=_td(flags_h, dev),
                                  oratio=torch.zeros(n, dtype=torch.float64, device=dev),
                                  similar=torch.zeros(n, dtype=torch.float32, device=dev),
                                  flips=torch.zeros(n, dtype=torch.int32, device=dev),
                                  choice=torch.full((n, 2), -1, dtype=torch.int32, device=dev))
        thr_dist, thr_dot, max_thr_dist, max_dot_dist = 0.5, 0.9, 2.0, 0.6
        rooted, out_n, core = num_root, 0, None       # core: rebuilt when the rooted set has changed
        self.scalp_passes = []
        with torch.cuda.device(dev):
            while True:
                act = torch.nonzero(s.flags == 0)[:, 0].to(torch.int32)
                new_root = new_out = 0
                if act.shape[0]:
                    core = core or self._scalp_core(s)
                    if core.grid_thr != thr_dist:
                        self._scalp_grid(core, thr_dist)
                    s.P, s.offs, new_root, new_out, refused = self._scalp_pass(s, core, act, thr_dist, thr_dot, out_ratio)
                    if refused:
                        raise _lib.MhError(_OUTSIDE % "connect_to_scalp: a joined strand")
                    if new_root:
                        core = None
                rooted += new_root
                out_n += new_out
                self.scalp_passes.append((thr_dist, thr_dot, rooted, out_n))
                if not new_root > (n - num_root) // 500:     # too few joined: widen the search, or stop at its widest
                    if thr_dist == max_thr_dist and thr_dot == max_dot_dist:
                        break
                    thr_dist = min(thr_dist + 0.25, max_thr_dist)
                    thr_dot = max(thr_dot - 0.075, max_dot_dist)
            flags_h = s.flags.cpu().numpy()
            self.scalp_out_ratio, self.scalp_similar = s.oratio.cpu().numpy(), s.similar.cpu().numpy()
            self.scalp_flips, self.scalp_choice = s.flips.cpu().numpy(), s.choice.cpu().numpy()
            pts_h, offs_h = s.P.cpu().numpy(), s.offs.cpu().numpy()
        self.scalp_root_flag, self.scalp_out_flag = (flags_h & 1) != 0, (flags_h & 2) != 0
        return split_strands(pts_h, offs_h, np.flatnonzero(flags_h))

    def WorldToVoxel(self, strands, bust_to_origin=None):
        """HairGrow.py:826-835 -> list of float32 [L,3] arrays in voxel units (adds bust_to_origin to the caller's arrays
        in place, like the reference)."""
        out = []
        for ss in strands:
            if bust_to_origin is not None:
                ss += bust_to_origin
            out.append(points_to_voxel(torch.from_numpy(np.asarray(ss)).type(torch.float).clone()).numpy())
        return out

    def VoxelToWorld(self, strands, bust_to_origin=None):
        """HairGrow.py:816-824."""
        out = []
        for ss in strands:
            w = voxel_to_points(ss.clone()).cpu().numpy()
            if bust_to_origin is not None:
                w -= bust_to_origin
            out.append(w)
        return out


def scalp_allocation(area, n):
    """Open3D's stratified allocation of n samples to triangles of the given areas (float64 [nf]): the bounds B [nf] int64,
    B[t] = floor(n * C[t] + 0.5) with C = cumsum(area / area.sum()) and B[nf-1] = n.  Sample i belongs to the first triangle
    t with B[t] > i, so triangle t receives B[t] - B[t-1] samples, in triangle order, whatever the random stream; a
    triangle of zero area receives none."""
    area = np.asarray(area, dtype=np.float64).reshape(-1)
    n = int(n)
    if area.size == 0 or n < 0 or not np.isfinite(area).all() or (area < 0).any() or not area.sum() > 0:
        raise _lib.MhError("scalp_allocation: needs n >= 0 and finite, non-negative areas with a positive sum")
    C = np.cumsum(area / area.sum())
    B = np.minimum(np.floor(n * C + 0.5), float(n)).astype(np.int64)      # (a C[t] that rounding took above 1 must not pass n)
    B[-1] = n
    return B


def sample_scalp(scalp_path, bust_to_origin, number_of_points=60000, seed=0, device="cuda:0", mesh=None, uniforms=None,
                 return_details=False):
    """The scalp samples of HairGrow.py's __main__ (:880-897): number_of_points points of the mesh at scalp_path with
    interpolated vertex normals (Open3D's sample_points_uniformly, use_triangle_normal=False), shifted by bust_to_origin
    and taken to voxel space -> (points_voxel, normals_voxel), float32 [n,3] tensors on `device`, exactly what tracing
    receives.  The reference draws from an unseeded generator; here the uniforms are
    np.random.default_rng(seed).random((n, 2)), so a seed repeats a run.  mesh: (vertices, faces, vertex normals) in place
    of the file; uniforms: float64 [n,2] in [0,1) in place of the seeded draw.  The triangle areas and the samples are
    computed by csrc/meshsample.hip; the allocation in between is scalp_allocation.  return_details: also return
    dict(area [nf] float64, bounds [nf] int64, triangle [n] int32 tensor: the triangle of every sample)."""
    if not torch.cuda.is_available():
        raise _lib.MhError("sample_scalp needs a ROCm GPU (no CPU fallback)")
    v, f, vn = read_obj_normals(scalp_path) if mesh is None else mesh
    v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1, 3)
    vn = np.ascontiguousarray(vn, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(f).reshape(-1, 3)
    n, nv, nf = int(number_of_points), v.shape[0], f.shape[0]
    if nv == 0 or nf == 0 or vn.shape[0] != nv or n < 0 or f.min() < 0 or f.max() >= nv:
        raise _lib.MhError("sample_scalp: needs a mesh with faces, one normal per vertex and face indices inside it")
    u = np.random.default_rng(seed).random((n, 2)) if uniforms is None else np.ascontiguousarray(uniforms, np.float64)
    if u.shape != (n, 2) or not ((u >= 0) & (u < 1)).all():
        raise _lib.MhError("sample_scalp: uniforms must be [n,2] in [0,1)")
    bust = np.ascontiguousarray(np.asarray(bust_to_origin, dtype=np.float64).reshape(3))
    dev, L = torch.device(device), _lib.lib()
    ctx = _lib.bare_ctx(dev)
    v_d, vn_d, f_d = _td(v, dev), _td(vn, dev), _td(f.astype(np.int32), dev)
    area = torch.empty((nf,), dtype=torch.float64, device=dev)
    pts = torch.empty((n, 3), dtype=torch.float32, device=dev)
    nrm = torch.empty((n, 3), dtype=torch.float32, device=dev)
    tri = torch.empty((n,), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        _lib.check(L.mh_tri_area64(ctx, _lib.ptr(v_d), nv, _lib.ptr(f_d), nf, _lib.ptr(area), _lib.stream_ptr()),
                   "mh_tri_area64")
        area_h = area.cpu().numpy()
        B = scalp_allocation(area_h, n)
        B_d, u_d = _td(B, dev), _td(u, dev)
        _lib.check(L.mh_mesh_sample(ctx, _lib.ptr(v_d), _lib.ptr(vn_d), nv, _lib.ptr(f_d), nf, _lib.ptr(B_d), _lib.ptr(u_d),
                                    n, host_ptr(bust), _lib.ptr(pts), _lib.ptr(nrm), _lib.ptr(tri), _lib.stream_ptr()),
                   "mh_mesh_sample")
    if return_details:
        return pts, nrm, dict(area=area_h, bounds=B, triangle=tri)
    return pts, nrm


DIFFUSE_STATUS = ("accepted", "inside hair", "ten steps", "nine restarts", "left the volume")


def diffusion_scalp(points, normals, ori, occ, device="cuda:0", return_details=False):
    """The reference's diffusion_scalp (Utils/PMVO_utils.py:467-593): from every scalp sample a walk along its normal in
    steps of one voxel until it meets hair whose orientation agrees (else the normal is bent towards the orientation found
    and the walk restarts), a cubic Hermite arc from the sample to that voxel, and the arcs' unit tangents averaged into the
    empty voxels they cross.  points / normals [n,3]: world-space samples; ori [3,Z,Y,X], occ [1,Z,Y,X]: the volume in the
    .mat convention (not HairGrowing's flipped copy).  Returns (ori, occ), new float32 tensors of the same shapes on
    `device`.  Everything is computed by csrc/hairdiffuse.hip in the reference's order of operations (float32 walk, float64
    arc, rows added per voxel in row order), bit for bit; there is no CPU fallback.

    return_details: also a dict with status [n] (index into DIFFUSE_STATUS) and step [n] per sample, end_point /
    first_normal / last_normal [n,3], total_sample and total_normal [R,3] float64 (what the reference saves as
    total_sample.npy / total_normal.npy), total_normal_unit [R,3] and voxel [R,3] (x, y, z; int64) per row, and
    left_volume: the number of samples abandoned because their walk left the volume.

    Deliberate differences: a walk whose voxel index leaves [0, dim) is abandoned with its own status and counted (the
    reference raises IndexError there, or wraps around for small negative indices), and a row of an arc outside the volume
    is left out; with no accepted sample the volumes come back unchanged (the reference fails at np.concatenate([])); the
    two .npy files are not written, their contents are in the details."""
    if not torch.cuda.is_available():
        raise _lib.MhError("diffusion_scalp needs a ROCm GPU (no CPU fallback)")
    dev, L = torch.device(device), _lib.lib()
    ctx = _lib.bare_ctx(dev)
    pts = torch.as_tensor(points).to(dev).type(torch.float).reshape(-1, 3).contiguous()
    nrm = torch.as_tensor(normals).to(dev).type(torch.float).reshape(-1, 3).contiguous()
    ori_o = torch.as_tensor(ori).to(dev).type(torch.float).contiguous().clone()
    occ_o = torch.as_tensor(occ).to(dev).type(torch.float).contiguous().clone()
    if occ_o.dim() != 4 or occ_o.shape[0] != 1 or ori_o.shape != (3,) + tuple(occ_o.shape[1:]) or nrm.shape != pts.shape:
        raise _lib.MhError("diffusion_scalp: needs points and normals [n,3], ori [3,Z,Y,X] and occ [1,Z,Y,X]")
    Z, H, W = (int(v) for v in occ_o.shape[1:])
    n = pts.shape[0]
    status = torch.empty((n,), dtype=torch.int32, device=dev)
    step = torch.empty((n,), dtype=torch.int32, device=dev)
    end, first, last = (torch.empty((n, 3), dtype=torch.float32, device=dev) for _ in range(3))
    R = 0
    with torch.cuda.device(dev):
        st = _lib.stream_ptr()
        _lib.check(L.mh_diffuse_walk(ctx, _lib.ptr(occ_o), _lib.ptr(ori_o), W, H, Z, _lib.ptr(pts), _lib.ptr(nrm), n,
                                     _lib.ptr(status), _lib.ptr(step), _lib.ptr(end), _lib.ptr(first), _lib.ptr(last), st),
                   "mh_diffuse_walk")
        offs = torch.zeros((n + 1,), dtype=torch.int64, device=dev)
        if n:
            torch.cumsum(torch.where(status == 0, step.long() + 1, torch.zeros_like(step).long()), 0, out=offs[1:])
            R = int(offs[-1])
        assert R < 2 ** 31
        sample, tangent, unit = (torch.empty((R, 3), dtype=torch.float64, device=dev) for _ in range(3))
        voxel = torch.empty((R, 3), dtype=torch.int32, device=dev)
        if R:
            keys = torch.empty((R,), dtype=torch.int64, device=dev)
            _lib.check(L.mh_diffuse_arc(ctx, _lib.ptr(pts), _lib.ptr(end), _lib.ptr(first), _lib.ptr(last), _lib.ptr(step),
                                        _lib.ptr(offs), n, R, W, H, Z, _lib.ptr(sample), _lib.ptr(tangent), _lib.ptr(unit),
                                        _lib.ptr(voxel), _lib.ptr(keys), st), "mh_diffuse_arc")
            # rows grouped by voxel, in row order within a voxel: the sort is stable
            scratch = torch.empty(int(L.mh_sort_scratch_bytes(R)), dtype=torch.uint8, device=dev)
            skeys = torch.empty_like(keys)
            order = torch.empty((R,), dtype=torch.int32, device=dev)
            _lib.check(L.mh_sort_keys(ctx, _lib.ptr(keys), R, max(1, (W * H * Z).bit_length()), _lib.ptr(scratch),
                                      scratch.numel(), _lib.ptr(skeys), _lib.ptr(order), st), "mh_sort_keys")
            sel = torch.empty(int(L.mh_select_scratch_bytes(R)), dtype=torch.uint8, device=dev)
            seg = torch.empty((R + 1,), dtype=torch.int32, device=dev)
            heads = torch.empty((R,), dtype=torch.int64, device=dev)
            meta = torch.empty((2,), dtype=torch.int32, device=dev)
            _lib.check(L.mh_segment_heads(ctx, _lib.ptr(skeys), R, _lib.ptr(seg), _lib.ptr(heads), _lib.ptr(meta),
                                          _lib.ptr(sel), sel.numel(), st), "mh_segment_heads")
            _lib.check(L.mh_diffuse_splat(ctx, _lib.ptr(seg), _lib.ptr(heads), _lib.ptr(meta), _lib.ptr(order),
                                          _lib.ptr(unit), R, W, H, Z, _lib.ptr(occ_o), _lib.ptr(ori_o), st),
                       "mh_diffuse_splat")
    if not return_details:
        return ori_o, occ_o
    return ori_o, occ_o, dict(status=status, step=step, end_point=end, first_normal=first, last_normal=last,
                              total_sample=sample, total_normal=tangent, total_normal_unit=unit, voxel=voxel.long(),
                              left_volume=int((status == 4).sum()))


def diffuse_scalp(save_path, scalp_points_voxel, scalp_normals_voxel, device="cuda:0", occ_path=None, ori_path=None,
                  return_details=False):
    """The stage that writes the volumes HairGrow.py reads when `scalp_diffusion` is set: Occ3D.mat / Ori3D.mat of
    save_path (or occ_path / ori_path) go through diffusion_scalp with the scalp samples of the run -- scalp_samples.npz's
    float32 voxel-space points taken back to world units by voxel_to_points, the normals un-flipped (y and z negated
    again) -- and come out as Occ3D_diffusion.mat / Ori3D_diffusion.mat in the same directory, in PMVO.py's layout and
    dtype: get_ground_truth_3D_occ / _ori read back exactly the returned arrays.  Returns (ori [3,Z,Y,X], occ [1,Z,Y,X])."""
    occ = get_ground_truth_3D_occ(occ_path or os.path.join(save_path, "Occ3D.mat"))          # [Z,Y,X,1]
    ori = get_ground_truth_3D_ori(ori_path or os.path.join(save_path, "Ori3D.mat"))          # [Z,Y,X,3]
    pts = voxel_to_points(torch.as_tensor(scalp_points_voxel).cpu().type(torch.float).clone())
    nrm = torch.as_tensor(scalp_normals_voxel).cpu().type(torch.float).clone()
    nrm[..., 1:] *= -1
    res = diffusion_scalp(pts, nrm, torch.from_numpy(ori).permute(3, 0, 1, 2), torch.from_numpy(occ).permute(3, 0, 1, 2),
                          device=device, return_details=return_details)
    save_volume_mat_sparse(os.path.join(save_path, "Occ3D_diffusion.mat"), os.path.join(save_path, "Ori3D_diffusion.mat"),
                           res[1][0].cpu().numpy(), res[0].permute(1, 2, 3, 0).cpu().numpy())
    return res


def generate_segments(occ_path, ori_path, scalp_points_voxel, scalp_normals_voxel, save_path, bust_to_origin,
                      grow_threshold=0.8, device="cuda:0", write_smooth=False, occ=None, ori=None, solver=None):
    """The `generate_segments` stage of HairGrow.py's __main__ (:897-920): scalp_segment.hair + num_root.npy, and with
    write_smooth also the Laplacian-smoothed copy scalp_segment_smooth.hair (:914-917).  occ / ori: the readers' arrays
    in place of the two files; solver: a HairGrowing of that volume to use instead of building one.  Returns the unsmoothed
    segments."""
    if solver is None:
        solver = HairGrowing(occ_path, ori_path, device=device, occ=occ, ori=ori)
    strands, num_root = solver.GenerateGuideStrandFromScalp(scalp_points_voxel, scalp_normals_voxel, None,
                                                            grow_threshold)
    world = solver.VoxelToWorld(strands, bust_to_origin)
    save_hair_strands(os.path.join(save_path, "scalp_segment.hair"), world, bust_to_origin, translate=False)
    if write_smooth:
        smooth = smooth_strands(list(world), 4.0, 2.0, device=device)
        save_hair_strands(os.path.join(save_path, "scalp_segment_smooth.hair"), smooth, bust_to_origin, translate=False)
    np.save(os.path.join(save_path, "num_root.npy"), np.array(num_root))
    return world, num_root


def connect_segments(save_path, bust_to_origin, connect_threshold=0.005, connect_dot_threshold=0.7, occ_path=None,
                     ori_path=None, device="cuda:0", occ=None, ori=None, solver=None):
    """The `connect_segments` stage of HairGrow.py's __main__ (:925-952): reads scalp_segment.hair and num_root.npy
    from save_path, joins the non-root segments (shifted by bust_to_origin) with find_connect_info on the volume of
    occ_path / ori_path (or the arrays occ / ori, or the given solver), smooths every strand (4.0, 2.0) and writes
    strands.hair.  Returns (strands, solver)."""
    segment, points = load_strand(os.path.join(save_path, "scalp_segment.hair"))
    num_root = int(np.load(os.path.join(save_path, "num_root.npy")))
    bust = np.asarray(bust_to_origin, dtype=np.float64)
    strands = []
    beg = 0
    for i, seg in enumerate(segment):
        strand = points[beg:beg + seg]
        if i >= num_root:
            strand += bust
        strands.append(strand)
        beg += seg
    if solver is None:
        solver = HairGrowing(occ_path, ori_path, device=device, occ=occ, ori=ori)
    connected = solver.find_connect_info(strands[num_root:], connect_threshold, connect_dot_threshold)
    new_strands = strands[:num_root] + [c - bust for c in connected]
    new_strands = smooth_strands(new_strands, 4.0, 2.0, device=device)
    save_hair_strands(os.path.join(save_path, "strands.hair"), new_strands, bust, translate=False)
    return new_strands, solver


def connect_scalp(save_path, bust_to_origin, out_ratio, occ_path=None, ori_path=None, device="cuda:0", occ=None, ori=None,
                  infer_inner=False, solver=None):
    """The `connect_scalp` stage of HairGrow.py's __main__ (:954-976): reads strands.hair and num_root.npy from save_path,
    attaches the floating strands in voxel space (HairGrowing.connect_to_scalp on the volume of occ_path / ori_path or the
    arrays occ / ori, or the given solver), returns to world units, smooths every strand (4.0, 2.0) and writes
    connected_strands.hair.  out_ratio: the case's HairGenerate.out_ratio.  Returns (strands, solver)."""
    segment, points = load_strand(os.path.join(save_path, "strands.hair"))
    num_root = int(np.load(os.path.join(save_path, "num_root.npy")))
    bust = np.asarray(bust_to_origin, dtype=np.float64)
    strands = np.split(points, np.cumsum(segment)[:-1]) if len(segment) else []
    if solver is None:
        solver = HairGrowing(occ_path, ori_path, device=device, occ=occ, ori=ori)
    connected = solver.connect_to_scalp(solver.WorldToVoxel(strands, bust), num_root, out_ratio, infer_inner)
    world = []
    for ss in connected:
        w = voxel_to_points(torch.from_numpy(ss.copy())).numpy()
        w -= bust
        world.append(w)
    world = smooth_strands(world, 4.0, 2.0, device=device)
    save_hair_strands(os.path.join(save_path, "connected_strands.hair"), world, bust, translate=False)
    return world, solver
