"""The drivers filter_negative_points and optimize -- mirrors of the module-level functions of the reference's PMVO.py
(:535-595; refine, :602-764, is refine.py).  Chunking, file names and dtypes are the reference's (they are its
checkpoint/resume mechanism); with torch.distributed initialised the independent chunks are dealt round-robin to the ranks
(monohair_amd.dist).  RefinePrefetch, which optimize starts and refine adopts, is kept with its starter."""
import os
import threading
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib
from . import dist as mdist
from . import pmvo_utils as U


def _filter_single(points, pmvo, step, num_sub_p):
    """filter_negative_points on one rank: the candidates go up in a few large blocks (the float64 -> float32 conversion of
    block k+1 runs on the host while the GPU votes on block k), one vote launch per block -- the kernel is told where its
    points sit in the reference's N//30-sized pieces (PMVO.py:540-552; include/mh_pmvo.h: batch / row0 / total) -- and the
    surface points are compacted on the device (`covered[surface].astype(float32)` = the selected rows of the float32
    copy the votes were computed on).  -> (surface votes, shell votes [total] uint8 numpy, surface_points float32 [S,3]
    numpy; pinned)."""
    dev, xfer = pmvo.device, pmvo.transfer
    L, ctx = pmvo._L, pmvo._ctx
    total = min(int(points.shape[0]), step * num_sub_p)
    per = max(1, -(-step // 4)) * num_sub_p                      # four blocks, cut at piece boundaries
    bounds = [(lo, min(lo + per, total)) for lo in range(0, total, per)]
    surf = torch.empty((total,), dtype=torch.uint8, device=dev)
    filt = torch.empty((total,), dtype=torch.uint8, device=dev)
    out = torch.empty((total, 3), dtype=torch.float32, device=dev)
    cnt = torch.zeros((len(bounds) + 1,), dtype=torch.int32, device=dev)
    scratch = torch.empty(int(L.mh_select_scratch_bytes(per)), dtype=torch.uint8, device=dev)
    cs, st = torch.cuda.current_stream(dev), _lib.stream_ptr()
    for k, (lo, hi) in enumerate(bounds):
        # (the conversions of the four blocks on four worker threads side by side: 3.9-4.1 ms for the stage instead of 3.2 --
        # thread wake-ups and the GIL cost more than the 0.25 ms conversions they overlap; measured, dropped)
        blk = xfer.upload_named("filter%d" % k, points[lo:hi])
        # (the rows of a block are taken cell by cell -- 64 spatial neighbours per wave -- not in the candidates' raster order)
        order = U.spatial_order(blk)
        _lib.check(L.mh_filter_points_ordered(ctx, _lib.ptr(blk), hi - lo, pmvo._side, float(pmvo.conf_threshold),
                                              float(pmvo.visible_threshold), _lib.ptr(surf, lo), _lib.ptr(filt, lo), None, None,
                                              num_sub_p, lo, total, _lib.ptr(order), st), "mh_filter_points_ordered")
        _lib.check(L.mh_select_rows(ctx, _lib.ptr(surf, lo), None, 0, hi - lo, _lib.ptr(blk), None, _lib.ptr(out), None, None,
                                    _lib.ptr(cnt, k), _lib.ptr(cnt, k + 1), _lib.ptr(scratch), scratch.numel(), st),
                   "mh_select_rows")
    (hsurf, hfilt, hcnt), ev = xfer.download(cs, None, [surf, filt, cnt[len(bounds):]])
    ev.synchronize()
    (pts,), ev = xfer.download(cs, None, [out[:int(hcnt[0])]])
    ev.synchronize()
    return hsurf, hfilt, pts


def filter_negative_points(points, pmvo, args, step=30):
    """PMVO.py:535-557: surface / shell classification of the raw candidates, in N//30-sized pieces."""
    if points.shape[0] % step != 0:
        step = step + 1
    num_sub_p = points.shape[0] // 30
    if mdist.world() == 1 and num_sub_p > 0 and isinstance(points, np.ndarray):
        surf, filt, surface_points = _filter_single(points, pmvo, step, num_sub_p)
        surface_indexs, filter_indexs = surf.astype(bool), filt.astype(bool)
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
    num_sub_p = 5000
    M = int(pts_np.shape[0])
    step = M // num_sub_p + 1
    dev, xfer = pmvo.device, pmvo.transfer
    streams = pmvo.side_streams(3)     # kept on the object: their tap-list scratch (1.2 GB each) is reused
    main = torch.cuda.current_stream(dev)
    cp = xfer.stream("copy")
    o_all = torch.empty((M, 3), dtype=torch.float32, device=dev)
    l_all = torch.empty((M,), dtype=torch.float32, device=dev)
    h_all = torch.empty((M,), dtype=torch.bool, device=dev)
    # the arrays the caller gets: pinned, filled group by group
    host = [xfer.pinned_like(t) for t in (o_all, l_all, h_all)]
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
    dev_all, staged = xfer.upload_whole(pts_np, head=nhead * num_sub_p, after_head=lambda d: launch(d, 0, nhead))
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
    files = (U.NpyRowWriter(args.save_root + "/select_o.npy", (M, 3), np.float32),
             U.NpyRowWriter(args.save_root + "/min_loss.npy", (M,), np.float32),
             U.NpyRowWriter(args.save_root + "/high_conf_index.npy", (M,), np.bool_))
    chunks = sorted(done)
    GROUP = 8
    groups = []
    with torch.cuda.stream(cp):
        for g0 in range(0, len(chunks), GROUP):
            grp = chunks[g0:g0 + GROUP]
            for i in grp[-len(streams):]:                 # the last chunk of the group on each stream
                cp.wait_event(done[i])
            a, b = grp[0] * num_sub_p, min((grp[-1] + 1) * num_sub_p, M)
            _, ev = xfer.download(cp, None, [t[a:b] for t in (o_all, l_all, h_all)], into=[h[a:b] for h in host])
            groups.append((a, b, ev))
    select_ori, min_loss, high_conf_index = (h.numpy() for h in host)
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
    num_sub_p = 5000
    step = points.shape[0] // num_sub_p + 1
    pts_np = points if isinstance(points, np.ndarray) else torch.as_tensor(points).detach().cpu().numpy()
    if mdist.world() == 1:
        out = _optimize_single(pts_np, pmvo, args)
        assert len(out[2]) == len(out[0])
        return out
    pool = ThreadPoolExecutor(4)
    streams = pmvo.side_streams(3)
    counter = [0]
    main = torch.cuda.current_stream()

    def join():                        # results are read on the main stream: join the side streams first
        for st in streams:
            main.wait_stream(st)

    # ONE float64 -> float32 conversion (numpy's rounding = the reference's `.type(torch.float)`, PMVO.py:40), in the pinned
    # staging buffer: the result is both what is uploaded and select_p.npy (PMVO.py:575)
    dev_all, select_points = pmvo.transfer.upload_whole(pts_np)
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


class RefinePrefetch:
    """The point-only inputs of refine()'s smoothing loop, prepared while optimize() runs (single rank).

    refine's neighbour table `KDTree(points).query(points, 100)` (PMVO.py:605-612), the head-filter votes of every point
    (:110-137, per 5000-point chunk) and the scalp test (:98-107) depend on the points alone, and the points exist before
    optimize() starts.  A helper thread builds the grid, runs the self-query (with its host-side retries) and the two
    vote kernels on a low-priority stream of its own; the search kernels of optimize() keep the GPU, these fill what they
    leave.  refine() adopts the result only if the points it is handed equal these bit for bit (mh_buffers_differ on the
    device) and the thresholds are the ones used here; otherwise it computes everything itself as before."""

    def __init__(self, pmvo, pts_dev, sub_num, k):
        self.pmvo, self.pts_dev, self.sub_num, self.k = pmvo, pts_dev, int(sub_num), int(k)
        self.n = int(pts_dev.shape[0])
        self.conf_threshold, self.visible_threshold = float(pmvo.conf_threshold), float(pmvo.visible_threshold)
        self.scalp_tree = pmvo.scalp_tree
        self.error = None
        self.grid = self.index_all = self.head_all = self.head_top_all = None
        rng = (0, 0)
        try:
            rng = torch.cuda.Stream.priority_range()        # (least, greatest), e.g. (0, -1)
        except Exception:
            pass
        self.stream = pmvo.transfer.stream("prefetch", priority=rng[0])
        self.ready = torch.cuda.Event()
        self.ready.record(torch.cuda.current_stream(pmvo.device))      # pts_dev's upload is queued on the caller's stream
        self.done = torch.cuda.Event()
        self.thread = threading.Thread(target=self._run, daemon=True)
        self.thread.start()

    def _run(self):
        pm = self.pmvo
        try:
            with torch.cuda.device(pm.device), torch.cuda.stream(self.stream):
                self.stream.wait_event(self.ready)
                if self.n:
                    self.grid = U.GridKNN(self.pts_dev, k_hint=self.k, device=pm.device)
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
