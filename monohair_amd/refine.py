"""The driver refine -- mirror of the reference's PMVO.py:602-764: KNN-medoid smoothing, loss threshold, shell points, voxel
fit, Ori3D.mat / Occ3D.mat.  One device-resident pass (_refine_device) and the host-driven forms tests pin it against."""
import collections
import functools
import os
import threading

import numpy as np
import torch

from . import _lib
from . import dist as mdist
from . import pmvo_utils as U
from .timing import stage

REFINE_CHUNK = 5000                      # points per smoothing chunk (PMVO.py:602) and per batch of the sums over views
REFINE_K = 100                           # neighbours of a medoid (PMVO.py:605,660)
REPLACE_COS = 0.95                       # a direction less similar than this to its medoid is replaced (PMVO.py:625-640)
LOSS_STEP, LOSS_RANGE = 0.005, 4.0       # the depth step / range of the loss of a medoid direction (PMVO.py:619-623)


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
        g = U.GridKNN(data_points, k_hint=k, device=device)
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
    st, st2 = _lib.stream_ptr(main), _lib.stream_ptr(side)
    centers = torch.empty((n_all, 3), dtype=torch.float32, device=device)
    loss_all = torch.empty((n_all,), dtype=torch.float32, device=device)
    closes, g0 = _loss_groups(n_all // REFINE_CHUNK + 1), 0
    for i, (lo, hi, _, _, _) in enumerate(_chunk_slices(n_all, REFINE_CHUNK, 1, 0)):
        if hi > lo:
            _lib.check(L.mh_medoid_indexed(ctx, _lib.ptr(ori_dev), _lib.ptr(index_all, lo, K), hi - lo, K,
                                           _lib.ptr(centers, lo, 3), None, st), "mh_medoid_indexed")
            _lib.check(L.mh_replace_dissimilar(ctx, _lib.ptr(centers, lo, 3), _lib.ptr(ori_dev, lo, 3), REPLACE_COS, hi - lo, st),
                       "mh_replace_dissimilar")
        if i in closes and hi > g0:
            ev = torch.cuda.Event()
            ev.record(main)
            side.wait_event(ev)
            _lib.check(L.mh_refine_loss_maps(ctx, _lib.ptr(pts_dev, g0, 3), _lib.ptr(centers, g0, 3), LOSS_STEP, LOSS_RANGE,
                                             hi - g0, pmvo._side, float(pmvo.conf_threshold), _lib.ptr(loss_all, g0), None,
                                             REFINE_CHUNK, g0, n_all, st2), "mh_refine_loss_maps")
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
            _lib.check(L.mh_medoid_indexed(ctx, _lib.ptr(ori_dev), _lib.ptr(index_all, row_of[i], K), n, K, _lib.ptr(center), None,
                                           st), "mh_medoid_indexed")
            _lib.check(L.mh_refine_loss_maps(ctx, _lib.ptr(pts_dev, a, 3), _lib.ptr(center), LOSS_STEP, LOSS_RANGE, n, pmvo._side,
                                             float(pmvo.conf_threshold), _lib.ptr(loss_u), None, REFINE_CHUNK, a, n_all, st),
                       "mh_refine_loss_maps")
            _lib.check(L.mh_filter_points(ctx, _lib.ptr(pts_dev, a, 3), n, pmvo._side, float(pmvo.conf_threshold),
                                          float(pmvo.visible_threshold), None, None, None, _lib.ptr(head), REFINE_CHUNK, a,
                                          n_all, st), "mh_filter_points")
            _lib.check(L.mh_refine_combine(ctx, _lib.ptr(center), _lib.ptr(loss_u), _lib.ptr(head), _lib.ptr(head_top_all, a),
                                           REPLACE_COS, _lib.ptr(ori_dev, a, 3), _lib.ptr(loss_dev, a), n, st),
                       "mh_refine_combine")
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
    xfer = pmvo.transfer
    main, side = torch.cuda.current_stream(device), xfer.stream("refine_side")
    fu = np.ascontiguousarray(filter_unvisible_points) if filter_unvisible_points is not None else np.zeros((0, 3), np.float32)
    F = int(len(fu))
    with stage("refine: uploads + prefetch adoption", device):
        pts = xfer.upload_named("refine_p", np.asarray(points).reshape(-1, 3))
        ori_dev = xfer.upload_named("refine_o", np.asarray(ori).reshape(-1, 3))
        loss_dev = xfer.upload_named("refine_l", np.asarray(loss).reshape(-1))
        pf = pmvo.take_refine_prefetch(pts, REFINE_CHUNK, REFINE_K)
        # (what ran: tests, bench)
        pmvo.last_refine = {"device_pass": True, "prefetch_adopted": pf is not None, "shell_stage": "device"}
    fb = fq = hd = ht = None
    side.wait_stream(main)
    if F:
        with torch.cuda.stream(side):
            fb = xfer.upload_named("refine_fb", fu.reshape(-1, 3))                    # float32 (votes, scalp test, files)
            fq = xfer.upload_named("refine_fq", fu.reshape(-1, 3), np.float64) if fu.dtype == np.float64 else fb
            hd = torch.empty((F,), dtype=torch.uint8, device=device)
            _lib.check(pmvo._L.mh_filter_points(pmvo._ctx, _lib.ptr(fb), F, pmvo._side, float(pmvo.conf_threshold),
                                                float(args.PMVO.visible_threshold), None, None, None, _lib.ptr(hd),
                                                REFINE_CHUNK, 0, F, _lib.stream_ptr()), "mh_filter_points")
            ht = pmvo.head_top_mask_device(fb)
    return _DeviceState(main, side, xfer.stream("copy"), int(points.shape[0]), F, pts, ori_dev, loss_dev, pf, fb, fq, hd, ht)


def _device_neighbours(pmvo, d):
    """What the smoothing loop needs of the points alone -- optimize()'s prefetch, or made here -> (the spatial index of all
    points, the neighbour table, the head-filter votes (queued on the side stream), the scalp test)."""
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


def _shell_device(pmvo, d, grid, threshold):
    """Loss threshold, shell points, concatenation (PMVO.py:651-693): flags and stable compactions, the host reads two
    counters.  -> (points [cap,3], orientations [cap,3], kept points, kept points + kept shell points), or None when the
    host-driven stage has to run: fewer kept points than neighbours (the reference then asks for that many)."""
    L, ctx, device, st, n_all, F = pmvo._L, pmvo._ctx, pmvo.device, _lib.stream_ptr(d.main), d.n_all, d.F
    valid = torch.empty((n_all,), dtype=torch.uint8, device=device)
    _lib.check(L.mh_flag_less(ctx, _lib.ptr(d.loss), float(threshold), n_all, _lib.ptr(valid), st), "mh_flag_less")
    sel_p = torch.empty((n_all + F, 3), dtype=torch.float32, device=device)
    sel_o = torch.empty((n_all + F, 3), dtype=torch.float32, device=device)
    cnt = torch.zeros((2,), dtype=torch.int32, device=device)
    scratch = torch.empty(int(L.mh_select_scratch_bytes(max(n_all, F))), dtype=torch.uint8, device=device)
    _lib.check(L.mh_select_rows(ctx, _lib.ptr(valid), None, 0, n_all, _lib.ptr(d.pts), _lib.ptr(d.ori), _lib.ptr(sel_p),
                                _lib.ptr(sel_o), None, None, _lib.ptr(cnt, 0), _lib.ptr(scratch), scratch.numel(), st),
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
                                    _lib.ptr(sel_o), None, _lib.ptr(cnt, 0), _lib.ptr(cnt, 1), _lib.ptr(scratch), scratch.numel(),
                                    st), "mh_select_rows")
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
    sel_p, sel_o, n_valid, n_sel = sel
    (hp, hq), ev_shell = pmvo.transfer.download(d.cp, d.main, [sel_p[n_valid:n_sel], sel_o[n_valid:n_sel]])
    with stage("refine: voxel fit + reduce", pmvo.device):
        vox, vori = U.voxel_fit_device(sel_p, sel_o, n_sel, pmvo.device, voxel_min, voxel_size, grid_resolution)
    ev_shell.synchronize()
    return vox, vori, hp, hq


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
        # the smoothed arrays travel to pinned host memory on the copy stream while the shell stage runs
        (new_ori, new_loss), ev_res = pmvo.transfer.download(d.cp, d.main, [d.ori, d.loss])
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
    return ((mdist.world() == 1 or not mdist.refine_sharded()) and len(points) > 0
            and getattr(args, "knn", "device") == "device" and os.environ.get("MH_REFINE_DEVICE", "1") != "0"
            and os.environ.get("MH_REFINE_CHAIN", "1") != "0")


def _smooth_host(points, ori, loss, pmvo, args, writer, grid_all):
    """The host-driven forms of the smoothing loop, in place in `ori` and `loss`.  Neighbour indices and the head-top mask
    depend on the points only: ONE query for all chunks, then the sequentially dependent loop (chunk k+1 reads the
    orientations chunk k wrote, PMVO.py:614,640) runs on the device, stream-ordered, without a host round trip per chunk:
    _smooth_chain on one rank; _smooth_sharded with MH_REFINE_CHAIN=0, or with several ranks (mdist.refine_sharded), each of
    which queries the neighbours of the rows it owns only.  grid_all receives the spatial index of all points."""
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
                                                REFINE_CHUNK, 0, n_all, _lib.stream_ptr(side)), "mh_filter_points")
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
    with stage("refine: voxel fit + reduce", device):
        if mdist.world() > 1 and not mdist.refine_sharded():
            res = U.voxel_fit(select_points, select_ori, device, voxel_min, voxel_size, grid_resolution, dense=False)
            return res["voxels"].cpu().numpy(), res["ori"].cpu().numpy()
        return mdist.voxel_fit_reduced(select_points, select_ori, device, voxel_min, voxel_size, grid_resolution, sparse=True)


def _finish_volume(vox, vori, pmvo, args, infer_inner, mat_writer, writer, is_root, voxel_min, voxel_size, grid_resolution):
    """The network's orientation merged in for points seen in <= 2 views (PMVO.py:733-751), Ori3D.mat / Occ3D.mat, and the
    end of every background write.  -> the voxel list that was written."""
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
