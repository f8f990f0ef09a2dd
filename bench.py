#!/usr/bin/env python
"""bench.py -- PMVO iterations/sec on the synthetic 60-view 1080p / 256^3 workload (BASELINE.json).

One step = one PMVO iteration = one `PMVO.forward()` over a chunk of 5000 candidate points against all
V views (one step of the trange at /root/reference/PMVO.py:572-574): the H2D upload of the chunk, project /
visibility / tap lists (mh_project_taps_kernel), base-view ranking (mh_topk_kernel) and the fused loss search
(mh_search3_kernel), maps resident in HBM, no file IO.

    python bench.py [--gpus N --steps K --warmup W] [--dump-outputs DIR]

--dump-outputs DIR: after the timed region, what the last timed step returned (points, line_ori, min_loss, high_conf; rank
0's chunk at N > 1) is written as DIR/<name>.npy in float32; the inputs depend on the arguments only, so two builds can be
compared output for output.

N > 1: one process per GPU over RCCL.  Under `python -m torch.distributed.run ... bench.py --gpus N` the ranks are
already there (RANK / LOCAL_RANK / WORLD_SIZE); started plainly, `python bench.py --gpus N` launches the N ranks
itself (it re-executes under torch.distributed.run on 127.0.0.1).  Points shard across ranks (every GPU holds all
views; no collective inside an iteration -- SURVEY.md §8e), so per-GPU work is fixed as N grows: "scaling": "weak".
Rank 0 prints ONE JSON line.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import threading
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0        # /opt/skills/guides/MI355X_MICROARCH.md: HBM3E 8 TB/s spec
VALU_PEAK_TF = 157.3         # same guide: peak fp32 vector (256 CU x 4 SIMD x 64 FLOP/clk x 2.4 GHz)
FLOP_PER_PAIR = 8            # one (candidate, view, tap) evaluation
CHUNK = 5000                 # PMVO.py:566
PREWARM = int(os.environ.get("MH_BENCH_PREWARM", "256"))   # untimed set-up iterations before the --warmup ones (GPU clocks at their running state;
                             # round 6: 48 -> 256 = 0.16 s -- the first bench of a fresh box measured 1 442 it/s with 48, 1 633-1 646 after)
SETTLE = int(os.environ.get("MH_BENCH_SETTLE", "16"))   # iterations between two drains after the pre-warm (see main)
XGMI_LINK_GBS = 153.0        # per-link xGMI bandwidth, 7 links per GPU


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--views", type=int, default=60)
    ap.add_argument("--height", type=int, default=1920)
    ap.add_argument("--width", type=int, default=1080)
    ap.add_argument("--volume", type=int, default=256)
    ap.add_argument("--patch", type=int, default=7)          # big_wavy1.yaml:18
    ap.add_argument("--conf-threshold", type=float, default=0.15)
    ap.add_argument("--quantize", action="store_true", help="8-bit orientation/confidence maps (file hand-off)")
    ap.add_argument("--codes", action="store_true",
                    help="headline on maps uploaded as 8-bit file codes (PMVO.from_u8; the regime of real captures) -- for "
                         "profiling that regime; the default run reports it as secondary_8bit_maps")
    ap.add_argument("--cpu-points", type=int, default=0, help="points of the CPU baseline sample (0 = auto)")
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--no-secondary", action="store_true", help="skip the secondary legs")
    ap.add_argument("--variant", type=int, default=0)
    ap.add_argument("--option", action="append", default=[], metavar="KEY=VALUE",
                    help="mh_ctx_set_option on the headline context (A/B runs, e.g. --option reproject_rule=1 --option "
                         "sum_block=0 = the batch-independent arithmetic of rounds 1-4); recorded in config.options")
    ap.add_argument("--topk-order", type=int, default=-1, help="0 torch.topk's tie order (default), 1 index order (A/B)")
    ap.add_argument("--streams", type=int, default=3,
                    help="HIP streams the independent iterations alternate on (as monohair_amd.pmvo.optimize does)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write the outputs of the last timed step as DIR/<name>.npy (float32)")
    return ap.parse_args()


def spawn_ranks(a):
    """`python bench.py --gpus N` without a launcher: start the N ranks ourselves (one process per GPU, RCCL)."""
    import torch

    have = torch.cuda.device_count()
    if have < a.gpus and os.environ.get("MH_DEVICE_OVERRIDE") is None:     # (test hook: ranks share one GPU over gloo)
        sys.stderr.write("bench.py: --gpus %d asked for but this node shows %d GPU(s); refusing to report a %d-GPU "
                         "number from fewer devices\n" % (a.gpus, have, a.gpus))
        sys.exit(2)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"),
               MH_BENCH_SPAWNED="1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(a.gpus),
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    sys.exit(subprocess.call(cmd, env=env))


class Emitter:
    """exactly one JSON line, whoever gets there first (the main path or the watchdog of the collective legs)"""

    def __init__(self):
        self.lock = threading.Lock()
        self.done = False

    def emit(self, out):
        with self.lock:
            if self.done:
                return
            self.done = True
            print(json.dumps(out), flush=True)


DUMP_NAMES = ("points", "line_ori", "min_loss", "high_conf")      # forward()'s four results, in order


def dump_outputs(d, result):
    """--dump-outputs: the four device tensors forward() returned in the last timed step (the uploaded chunk [N,3], line
    orientation [N,3], minimal loss [N], high-confidence flag [N]) as d/<name>.npy, all float32 (the flag as 0 / 1).  N is at
    most CHUNK, so the files stay far below 64 MB.  Called after the timed region's closing barrier: the step is complete."""
    import numpy as np

    os.makedirs(d, exist_ok=True)
    shapes = {}
    for name, t in zip(DUMP_NAMES, result):
        arr = t.detach().cpu().numpy().astype(np.float32)
        np.save(os.path.join(d, name + ".npy"), arr)
        shapes[name] = list(arr.shape)
    return {"dir": d, "dtype": "float32", "shapes": shapes}


def main():
    a = parse()
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return spawn_ranks(a)

    import numpy as np
    import torch

    from monohair_amd import synth
    from monohair_amd.camera import camera_records, cameras_from_list
    from monohair_amd.pmvo import PMVO

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    # test hooks: MH_DEVICE_OVERRIDE pins every rank to one GPU and MH_DIST_BACKEND=gloo replaces RCCL, so that the
    # world_size > 1 code path can be exercised on a single-GPU box (RCCL refuses two ranks on one device)
    shared_gpu = os.environ.get("MH_DEVICE_OVERRIDE") is not None
    if shared_gpu:
        local = int(os.environ["MH_DEVICE_OVERRIDE"])
    backend = os.environ.get("MH_DIST_BACKEND", "nccl")
    dev = torch.device("cuda", local)
    torch.cuda.set_device(dev)
    dist = None
    ranks_seen, devices_seen = 1, [local]
    if world > 1:
        import torch.distributed as dist

        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=dev)
        else:
            dist.init_process_group(backend=backend)
        # every rank really is there and sits on its own GPU
        ident = [None] * world
        prop = torch.cuda.get_device_properties(dev)
        dist.all_gather_object(ident, (socket.gethostname(), torch.cuda.current_device(),
                                       str(getattr(prop, "uuid", "")), os.getpid()))
        ranks_seen = dist.get_world_size()
        devices_seen = [i[1] for i in ident]
        assert ranks_seen == world, (ranks_seen, world)
        if not shared_gpu:
            assert len({(i[0], i[1]) for i in ident}) == world, "two ranks share a GPU: %r" % (ident,)
    if a.gpus > 1:
        assert world == a.gpus, "--gpus %d but %d rank(s) were launched" % (a.gpus, world)
    n_gpus = world

    V, H, W, P = a.views, a.height, a.width, a.patch * a.patch
    if a.codes:
        a.no_cpu = a.quantize = True      # (the CPU leg and the 8-bit secondary leg belong to the default run)
        sc = synth.make_scene_codes(V, H, W, device=dev, seed=0)
        cams = cameras_from_list(sc["cams"])
        recs = camera_records(cams)
        pm = PMVO.from_u8(cams, sc["depth"], sc["ori_u8"], sc["conf_u8"], sc["mask_u8"], device=dev, image_size=[H, W],
                          patch_size=a.patch, visible_threshold=1, conf_threshold=a.conf_threshold)
        scene = None
        del sc
    else:
        scene = synth.make_scene(V, H, W, device=dev, seed=0, quantize=a.quantize)
        cams = cameras_from_list(scene["cams"])
        recs = camera_records(cams)
        pm = PMVO.from_planes(recs, scene["depth"], scene["ori"], scene["conf"], scene["mask"], device=dev,
                              patch_size=a.patch, visible_threshold=1, conf_threshold=a.conf_threshold, camera=cams)
    if a.variant:
        pm.set_option("search_variant", a.variant)
    if a.topk_order >= 0:
        pm.set_option("topk_order", a.topk_order)
    for kv in a.option:
        k, v = kv.split("=")
        pm.set_option(k, int(v))

    # candidate points of the 256^3 volume; keep the ones the reference would send to optimize()
    # (filter_negative_points, PMVO.py:535-557), then chunk by 5000 and deal the chunks to the ranks
    cand = synth.candidate_points(res=a.volume, seed=0)
    surf = []
    for i in range(0, len(cand), 200000):
        s, _, _ = pm.filter_points(cand[i:i + 200000])
        surf.append(s.cpu().numpy())
    surf = np.concatenate(surf)
    pts = cand[surf]
    nchunk = max(1, len(pts) // CHUNK)
    chunks = [pts[i * CHUNK:(i + 1) * CHUNK] for i in range(nchunk)]
    my = [chunks[i] for i in range(rank, nchunk, world)] or chunks[:1]      # HOST arrays, as optimize() gets them

    # consecutive iterations are independent chunks of `optimize` (PMVO.py:572-574); like the driver in
    # monohair_amd/pmvo.py they alternate between HIP streams so one chunk's tail overlaps the next one's head
    streams = pm.side_streams(max(1, a.streams))
    # set-up, not steps: the per-stream tap-list scratch (1.2 GB each) and the allocator pools of the per-iteration
    # outputs exist before anything is timed, whatever --warmup is
    for st in streams:
        with torch.cuda.stream(st):
            pm._get_scratch(CHUNK)
            hold = [torch.empty((V, CHUNK, 2), device=dev), torch.empty((V, CHUNK), device=dev),
                    torch.empty((V, CHUNK), device=dev), torch.empty((V, CHUNK), device=dev),
                    torch.empty((20, CHUNK), device=dev), torch.empty((20, CHUNK), device=dev, dtype=torch.int32),
                    torch.empty((CHUNK, 3), device=dev), torch.empty((CHUNK,), device=dev),
                    torch.empty((CHUNK,), device=dev, dtype=torch.bool)]
            del hold
            pm.forward(my[0][:1])       # one point: loads the kernels' code objects (not a workload step)
    torch.cuda.synchronize()

    def step(i):
        # the whole forward() of the reference (PMVO.py:39-78): host numpy chunk in (the H2D copy is part of the step,
        # PMVO.py:40), four device tensors out
        with torch.cuda.stream(streams[i % len(streams)]):
            return pm.forward(my[i % len(my)])

    # set-up, not counted as warm-up: ~40 ms of the same work so that the GPU's clock / power state and the allocator
    # pools are those of a running job whatever --warmup is (measured with --steps 20: --warmup 3 alone gives 1180-1220
    # it/s, --warmup 50 gives 1377; the first ~20 iterations after an idle period run 10-15 % slower).  Reported in
    # config.prewarm_steps.
    import gc

    gc.collect()
    gc.freeze()          # no full collection of the set-up's objects (scene, chunks) in the middle of the timed region
    for i in range(PREWARM):
        step(i)
    # settle: drain, then a few more iterations and another drain.  (Round 6: after a long run-ahead of the host, ONE
    # hipMemcpyAsync among the first steps after a device-wide drain blocked for ~7 ms -- the runtime reclaiming the copy
    # commands that piled up while the host was ahead -- which with the GPU queue still shallow is 7 ms of idle GPU inside a
    # 60 ms timed region: 1 470 instead of 1 640 it/s, on every box with 256 / 320 pre-warm steps, never with 16 / 48 / 1000 /
    # 2000; docs/HISTORY.md.  The chunk upload is a kernel now (mh_upload_pinned) and has no such call; the drain stays.)
    torch.cuda.synchronize()
    for i in range(SETTLE):
        step(i)
    torch.cuda.synchronize()
    for i in range(a.warmup):
        step(i)

    def barrier():
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    # --- timed region: exactly K steps
    trace = [] if os.environ.get("MH_BENCH_TRACE_STEPS") else None
    if trace is not None:               # (diagnostic: when did the host issue each step, which collections ran in between)
        gc.callbacks.append(lambda phase, info: trace.append((time.perf_counter(), "gc-" + phase, info.get("generation"))))
    barrier()
    t0 = time.perf_counter()
    last = None
    for i in range(a.steps):
        if trace is not None:
            import faulthandler

            faulthandler.dump_traceback_later(0.002, exit=False)      # a step that stalls for 2 ms shows where
        last = step(a.warmup + i)       # (the outputs of the LAST timed step stay alive: cpu_baseline checks them)
        if trace is not None:
            faulthandler.cancel_dump_traceback_later()
            trace.append((time.perf_counter(), "step", i))
    t_enq = time.perf_counter() - t0    # the host has ISSUED the K steps (it runs ahead of the GPU; the barrier waits for them)
    barrier()
    dt = time.perf_counter() - t0
    if trace is not None:
        del gc.callbacks[-1]
        prev = t0
        for t, what, k in trace:
            if what != "step" or t - prev > 3e-4:
                print("[trace] +%.3f ms  %s %s  (%.3f ms since the previous mark)" % ((t - t0) * 1e3, what, k, (t - prev) * 1e3),
                      file=sys.stderr)
            prev = t
    last_chunk = my[(a.warmup + a.steps - 1) % len(my)]
    dumped = dump_outputs(a.dump_outputs, last) if a.dump_outputs and rank == 0 else None
    timed_region_s = dt
    per_rank = [a.steps / dt]
    if dist is not None:
        # (both ends of every rank's interval are barriers, so the per-rank figures differ only by how early a rank left
        # the first and reached the last one; the headline uses the maximum, as the contract asks)
        t = torch.tensor([dt], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        every = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(every, t)
        per_rank = [a.steps / float(x.item()) for x in every]
        dt = max(float(x.item()) for x in every)

    ms = dt / a.steps * 1e3
    value = a.steps * world / dt
    out = {
        "metric": "PMVO iterations/sec (60x1080p views, 256^3 volume)",
        "value": round(value, 3),
        "unit": "iterations/s",
        "n_gpus": n_gpus,
        "ranks_seen": ranks_seen,
        "backend": ("nccl" if backend == "nccl" else backend) if world > 1 else None,
        "steps": a.steps,
        "warmup": a.warmup,
        "ms_per_step": round(ms, 4),
        "timed_region_s": round(dt, 7),
        "host_issue_ms_per_step": round(t_enq / a.steps * 1e3, 4),
        "per_rank_iterations_per_s": [round(v, 2) for v in per_rank],
        "higher_is_better": True,
        "scaling": "weak",
        "vs_baseline": None,
        "dtype": "f32",
        "data": "synthetic",
        "config": {
            "workload": "synthetic sphere, %d views @ %dx%d, %d^3 volume, %d points/iteration, patch %d, S=90, "
                        "10 base views (%s)" % (V, H, W, a.volume, CHUNK, a.patch, {
                            (60, 1920, 1080, 256): "BASELINE.json configs[2], the configuration the metric is quoted on",
                            (30, 1920, 1080, 128): "BASELINE.json configs[1]",
                            (120, 3840, 2160, 512): "BASELINE.json configs[4], one GPU's share"}.get(
                                (V, H, W, a.volume), "custom size")),
            "views": V, "image": [H, W], "volume": a.volume, "points_per_iteration": CHUNK, "patch": a.patch,
            "conf_threshold": a.conf_threshold, "surface_points": int(len(pts)), "iterations_full_pass": nchunk,
            "parallelism": "points sharded over %d GPU(s) (one process each), views replicated; no collective inside "
                           "an iteration" % world,
            "devices": devices_seen,
            "options": dict(kv.split("=") for kv in a.option),
            "maps": "8-bit file codes (PMVO.from_u8)" if a.codes else ("quantized-8bit" if a.quantize else "continuous"),
            "streams": len(streams),
            "prewarm_steps": PREWARM, "settle_steps": SETTLE,
            "step_input": "host numpy chunk [5000,3] float64, uploaded inside the step (PMVO.py:40); maps resident in HBM",
        },
    }
    if dumped is not None:
        out["dump_outputs"] = dumped
    em = Emitter()

    # --- legs that need every rank: the RCCL volume reduce and the sharded full pass (N > 1).  A watchdog prints the
    # line with whatever has been measured if a collective does not come back.
    if world > 1 and not a.no_secondary:
        def give_up():
            if rank == 0:
                out.setdefault("secondary_error", "collective legs timed out")
                em.emit(out)
            os._exit(0)

        wd = threading.Timer(240.0 if rank == 0 else 250.0, give_up)
        wd.daemon = True
        wd.start()
        try:
            out["secondary_volume_reduce"] = secondary_volume_reduce(dev, backend)
        except Exception as e:
            out["secondary_volume_reduce"] = {"error": repr(e)[:300]}
        try:
            out["secondary_full_pass"] = secondary_full_pass(dev, pm, cand, dist)
        except Exception as e:
            out["secondary_full_pass"] = {"error": repr(e)[:300]}
        try:
            out["secondary_gabor_sharded"] = secondary_gabor_sharded(a, dev, dist, backend)
        except Exception as e:
            out["secondary_gabor_sharded"] = {"error": repr(e)[:300]}
        wd.cancel()
    if rank != 0:
        if dist is not None:
            dist.destroy_process_group()
        return

    # --- the kernels of the timed loop, one by one (rank 0, outside the timed region): HIP events on the launch
    # stream around launches that ROTATE over the chunks, so that no launch finds its read set in the Infinity Cache
    try:
        out.update(kernel_rooflines(a, pm, my, dev, V, H, W, P, codes=a.codes))
    except Exception as e:
        out["roofline"] = {"error": repr(e)[:300]}
    if not a.no_secondary and world == 1:
        if not a.quantize:
            try:
                out["secondary_8bit_maps"] = secondary_quantized(a, dev, recs, cams, my, cand)
            except Exception as e:   # a secondary number must never cost the headline line
                out["secondary_8bit_maps"] = {"error": repr(e)[:200]}
        try:
            out["secondary_full_pass"] = secondary_full_pass(dev, pm, cand, None)
        except Exception as e:
            out["secondary_full_pass"] = {"error": repr(e)[:200]}
        try:
            out["secondary_gabor_bank"] = secondary_gabor(a, dev)
        except Exception as e:
            out["secondary_gabor_bank"] = {"error": repr(e)[:200]}
        try:
            out["secondary_gabor_stage"] = secondary_gabor_stage(a, dev)
        except Exception as e:
            out["secondary_gabor_stage"] = {"error": repr(e)[:200]}
        try:       # the N = 1 point of the view-sharded Gabor curve (the same leg runs on all ranks at N > 1)
            out["secondary_gabor_sharded"] = secondary_gabor_sharded(a, dev, None, backend)
        except Exception as e:
            out["secondary_gabor_sharded"] = {"error": repr(e)[:200]}
    # last: its 128 OpenMP workers keep spinning for a while after the parallel region and would slow the host side
    # of the secondary legs
    if not a.no_cpu and world == 1:      # the CPU leg runs on rank 0 at N=1 only
        try:
            out["cpu_baseline"], out["parity_check"] = cpu_baseline(a, scene, recs, last_chunk, ms, last)
        except ParityError:
            raise                        # the timed kernels did not produce the oracle's bits: no line at all
        except Exception as e:
            out["cpu_baseline"] = {"error": repr(e)[:200]}
    if world > 1 and not a.no_cpu and scene is not None:
        # N > 1: no CPU baseline leg, but the line still verifies itself -- rank 0's last timed step against the oracle on
        # its chunk (one untimed pass: about a second of host time)
        try:
            _, out["parity_check"] = cpu_baseline(a, scene, recs, last_chunk, ms, last, check_only=512)
            out["parity_check"]["rank"] = 0
        except ParityError:
            raise
        except Exception as e:
            out["parity_check"] = {"error": repr(e)[:200]}
    em.emit(out)
    if dist is not None:
        dist.destroy_process_group()


def kernel_rooflines(a, pm, my, dev, V, H, W, P, codes=False):
    """Per-kernel durations of one iteration with HIP events on the launch stream, each launch on a different chunk,
    and the roofline of each kernel from what it actually executed.
      mh_search3_kernel  (dominant, fp32 VALU bound): executed (candidate, view, tap) evaluations x 8 FLOP
      mh_project_taps_kernel (HBM): bytes it has to move for what it produces
      mh_project_gather_kernel (HBM; the API form of Compute_Visible_and_Ori): SURVEY §8d's 2*V*N*(12P+20)+12N"""
    import torch

    from monohair_amd import _lib

    L, ctx = pm._L, pm._ctx
    N = len(my[0])
    f = dict(dtype=torch.float32, device=dev)
    same = [c for c in my if len(c) == N]
    # EVERY full chunk this rank owns (the work per chunk varies by a factor of two across the volume: the eight-chunk sample
    # of rounds 2-3 read 6 % above the average of the pass, which is what the timed loop and the rocprofv3 trace see)
    reps = max(2, min(len(same), 64))
    dchunks = [torch.from_numpy(same[(i * len(same)) // reps]).to(dev).float().contiguous() for i in range(reps)]
    e = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    vis, ori, conf, mask = (torch.empty((V, N), **f), torch.empty((V, N, 2), **f), torch.empty((V, N), **f),
                            torch.empty((V, N), **f))
    bidx = torch.empty((20, N), dtype=torch.int32, device=dev)
    bval = torch.empty((20, N), **f)
    lo, ml = torch.empty((N, 3), **f), torch.empty((N,), **f)
    hc = torch.empty((N,), dtype=torch.bool, device=dev)
    scratch, need = pm._get_scratch(N)
    st = _lib.stream_ptr()
    ranks = list(pm.RANKS)

    def prepare(p):
        _lib.check(L.mh_forward_prepare(ctx, _lib.ptr(p), N, pm._side, float(pm.conf_threshold), _lib.ptr(vis),
                                        _lib.ptr(ori), _lib.ptr(conf), _lib.ptr(mask), _lib.ptr(scratch), need, st))

    def topk():
        _lib.check(L.mh_topk_views(ctx, _lib.ptr(vis), _lib.ptr(conf), N, _lib.ptr(bidx), _lib.ptr(bval), st))

    def search(p):
        _lib.check(L.mh_search_prepared(ctx, _lib.ptr(p), N, pm._side, float(pm.conf_threshold), len(ranks),
                                        ranks[1] - ranks[0], _lib.ptr(ori), _lib.ptr(bidx), _lib.ptr(bval),
                                        _lib.ptr(scratch), _lib.ptr(lo), _lib.ptr(ml), _lib.ptr(hc), None, None, None,
                                        st))

    prepare(dchunks[0]); topk(); search(dchunks[0])     # noqa: E702  (warm)
    torch.cuda.synchronize()
    # tap preparation: `reps` launches back to back, every one on another chunk
    e[0].record()
    for p in dchunks:
        prepare(p)
    e[1].record()
    torch.cuda.synchronize()
    t_taps = e[0].elapsed_time(e[1]) / reps
    # what each launch executes, read back from its own work arrays (not timed)
    pairs = taps_vis = nvis = 0
    for p in dchunks:
        prepare(p); topk()                               # noqa: E702
        torch.cuda.synchronize()
        cnt, nvalid = pm.search_work(N, bval)
        pairs += int((cnt.sum(0) * nvalid * pm.NUM_SAMPLE).sum().item())
        taps_vis += int(cnt.sum().item())
        nvis += int((vis != -1).sum().item())
    pairs, taps_vis, nvis = pairs / reps, taps_vis / reps, nvis / reps
    # base-view ranking and search: events around each launch inside an uninterrupted stream of iterations (two rounds
    # over the chunks, the second one is kept), so that the durations are those of a running job -- what the one-stream
    # rocprofv3 trace of this command shows (profiles/) -- and not of a launch into an idle GPU
    # search_variant 9 / 10 split the launch (csrc/pmvo_search.hip: mh_launch_search): 9 = what precedes the search in the
    # unfused sequence (group sizes of the batch, work classes, launch order), 10 = mh_search3_kernel alone
    ev = [[torch.cuda.Event(enable_timing=True) for _ in range(6)] for _ in range(2 * reps)]
    base_variant = a.variant
    for k in range(2 * reps):
        p = dchunks[k % reps]
        prepare(p)
        ev[k][0].record(); topk(); ev[k][1].record()         # noqa: E702
        split = base_variant in (0, 100)                     # (other variants -- A/B forms, the portable kernel -- are timed whole)
        if split:
            pm.set_option("search_variant", base_variant + 9)
        ev[k][2].record()
        if split:
            search(p)                                        # (ordering kernels)
            pm.set_option("search_variant", base_variant + 10)
        ev[k][3].record()
        ev[k][4].record(); search(p); ev[k][5].record()      # noqa: E702  (mh_search3_kernel)
    pm.set_option("search_variant", base_variant)
    torch.cuda.synchronize()
    t_topk = sum(ev[k][0].elapsed_time(ev[k][1]) for k in range(reps, 2 * reps)) / reps
    t_order = sum(ev[k][2].elapsed_time(ev[k][3]) for k in range(reps, 2 * reps)) / reps
    t_search = sum(ev[k][4].elapsed_time(ev[k][5]) for k in range(reps, 2 * reps)) / reps
    # API form with materialised patches, rotating chunks as well
    # (eight chunks spread over the pass: every call materialises 365 MB of patch tensors, and walking 57 of them through
    # fresh allocations measures the allocator's cold pages -- 0.21 ms -- not the kernel)
    gchunks = [dchunks[(i * reps) // 8] for i in range(min(8, reps))]
    pm.Compute_Visible_and_Ori(gchunks[0])
    torch.cuda.synchronize()
    e[0].record()
    for p in gchunks:
        pm.Compute_Visible_and_Ori(p)
    e[1].record()
    torch.cuda.synchronize()
    t_pg = e[0].elapsed_time(e[1]) / len(gchunks)

    nominal = 10 * V * N * 90 * P
    tf = pairs * FLOP_PER_PAIR / (t_search * 1e-3) / 1e12
    # bytes mh_project_taps_kernel has to move (per launch): points + centre record and mask sample of every (view, point)
    # + the patch of every visible pair in; vis/ori/conf/mask + one header per pair + the tap lists + list lengths out
    taps_in = 12 * N + V * N * (16 + 4) + nvis * P * (2 if codes else 16)      # a tap is 2 B of codes or a 16-B record
    taps_out = V * N * (4 + 8 + 4 + 4) + V * N * 16 + taps_vis * 16 + V * N
    pg_bytes = 2 * V * N * (12 * P + 20) + 12 * N
    pre = "8bit:" if codes else ""          # profiles/traffic.json keeps the 8-bit regime's PMC figures under this prefix
    prof = load_profile_facts(V, H, W, pre, dict(visible_pairs=nvis, taps_written=taps_vis, pair_evals_executed=pairs))
    return {
        "roofline": {
            "kernel": "mh_search3_kernel<256>", "bound": "valu",
            # which of the kernel's two tap bodies this context runs (same results; monohair_amd/csrc/capi.cpp: contexts of
            # 8-bit views take the select-only kernel, all others the key kernel; search_variant 100.. forces the select body)
            "tap_body": ("select (v_cmp + 2 v_cndmask, 7 instructions per evaluation)" if (codes or 100 <= a.variant < 200)
                         else "key ((loss, tap) as one integer, v_min3_u32: 5.5 instructions per evaluation)")
                        if a.variant != 1256 else "portable kernel",
            "achieved": round(tf, 2), "peak": VALU_PEAK_TF, "unit": "TFLOP/s", "frac": round(tf / VALU_PEAK_TF, 4),
            "traffic": prof.get("traffic", {}).get(pre + "mh_search3_kernel<256>"),
            "traffic_source": prof.get("source"), "valu_issue_source": prof.get("source"),
            "launch_ms": round(t_search, 4),
            "pair_evals_executed": int(pairs), "flop_per_pair_eval": FLOP_PER_PAIR,
            "gpair_per_s_executed": round(pairs / (t_search * 1e-3) / 1e9, 1),
            "pair_evals_nominal": nominal, "executed_fraction_of_nominal": round(pairs / nominal, 4),
            "visible_view_fraction": round(nvis / (V * N), 4),
            "note": "executed = sum over points of (taps of the views that see the point) x (usable base-view ranks) x 90 "
                    "samples, read back from the launch's own work arrays; launch_ms is mh_search3_kernel alone (HIP events on "
                    "its stream; the ordering kernels of the unfused sequence are kernels_ms.order)",
            "valu_issue": prof.get(pre + "search_valu_issue"),
        },
        "roofline_kernels": [
            {"kernel": ("mh_project_taps_codes_kernel<%d>" if codes else "mh_project_taps2_kernel<%d>") % a.patch, "bound": "hbm",
             "launch_ms": round(t_taps, 4),
             "algorithmic_bytes_per_launch": int(taps_in + taps_out),
             "achieved": round((taps_in + taps_out) / (t_taps * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "frac": round((taps_in + taps_out) / (t_taps * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
             "traffic": prof.get("traffic", {}).get(pre + "mh_project_taps_kernel<%d>" % a.patch),
             "traffic_source": prof.get("source"),
             "bytes_model": "in: 12N + V*N*20 + visible*P*%d; out: V*N*20 + V*N*16 + taps*16 + V*N" % (2 if codes else 16),
             "visible_pairs": int(nvis), "taps_written": int(taps_vis)},
            {"kernel": "mh_project_gather_kernel<%d>" % a.patch, "bound": "hbm", "launch_ms": round(t_pg, 4),
             "algorithmic_bytes_per_launch": pg_bytes,
             "achieved": round(pg_bytes / (t_pg * 1e-3) / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
             "frac": round(pg_bytes / (t_pg * 1e-3) / 1e9 / HBM_PEAK_GBS, 4),
             "traffic": prof.get("traffic", {}).get(pre + "mh_project_gather_kernel<%d>" % a.patch),
             "traffic_source": prof.get("source"),
             "note": "the API form of Compute_Visible_and_Ori (patch tensors materialised, SURVEY.md §8d byte count); "
                     "forward() uses mh_project_taps2_kernel instead; launches rotate over %d chunks" % len(gchunks)},
        ],
        "kernels_ms": {"project_taps": round(t_taps, 4), "topk": round(t_topk, 4), "order": round(t_order, 4),
                       "search": round(t_search, 4), "project_gather_api_kernel": round(t_pg, 4)},
    }


PROFILE_SOURCE = ("profiles/traffic.json (the builder's rocprofv3 --pmc passes of this command, committed; NOT measured in "
                  "this run)")


def load_profile_facts(V, H, W, pre="", counters=None):
    """Facts that cannot be measured from inside this process (rocprofv3 PMC passes of this same command), from the
    committed profiles/traffic.json: HBM bytes per launch and the search kernel's VALU issue figures.  They are only
    quoted when the work counters THIS run read back from its own launches (visible (view, point) pairs, taps written,
    executed evaluations per launch) equal the ones the file was profiled at to 1 % (the 8-bit PMC passes are made with
    `--codes` as the main regime, whose chunks differ by 0.5 % from the secondary leg's): otherwise every copied field is
    None and `source` says why."""
    try:
        t = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
        if not t.get("workload", "").startswith("%d views @ %dx%d" % (V, H, W)):
            return {}
        at = t.get("profiled_at", {})
        for k, v in (counters or {}).items():
            ref = at.get(pre + k)
            if ref is None or abs(float(v) - float(ref)) > 1e-2 * float(ref):
                return {"source": "profiles/traffic.json NOT quoted: this run's %s = %s, the file was profiled at %s"
                                  % (k, int(v), ref)}
        return {"source": PROFILE_SOURCE,
                "traffic": {k: v.get("traffic_bytes") for k, v in t.items() if isinstance(v, dict) and "traffic_bytes" in v},
                "search_valu_issue": t.get("search_valu_issue"), "8bit:search_valu_issue": t.get("8bit:search_valu_issue")}
    except Exception:
        return {}


def secondary_volume_reduce(dev, backend):
    """The one exchange of the data path: the 256 x 256 x 192 x 4 fp32 orientation/occupancy volume of
    the voxel fit, every rank owning an x-slab, assembled on rank 0 over xGMI.  Each form is timed with a barrier on both
    sides, max over ranks, and checked on the root; the proven bindings run first, the hand-bound C-ABI ones last (the
    caller's watchdog prints the line with what has been measured if one of them does not come back):
      slab_gather_torch   peers hold their slab only, torch.distributed.batch_isend_irecv (the default of voxel_fit_reduced)
      dense_reduce_torch  torch.distributed.reduce of a dense volume per rank
      slab_gather_c_abi   mh_volume_gather (slab-sized peers)      dense_reduce_c_abi  mh_volume_reduce mode 1"""
    import torch
    import torch.distributed as dist

    from monohair_amd import dist as mdist

    w, r = dist.get_world_size(), dist.get_rank()
    fake = bool(os.environ.get("MH_RCCL_LIB"))
    X, Y, Z, C = (64, 64, 48, 4) if fake else (256, 256, 192, 4)     # (the stand-in stages through /dev/shm: keep it small)
    nbytes = X * Y * Z * C * 4
    b = mdist.slab_bounds(X, w)
    res = {"volume": [X, Y, Z, C], "bytes_dense": nbytes, "unit": "ms", "ranks": w,
           "default_exchange": mdist.exchange_mode()}
    if backend != "nccl" and not fake:
        res["note"] = "gloo test backend without MH_RCCL_LIB: RCCL legs skipped"
        return res
    cdev = dev if backend == "nccl" else "cpu"
    lo, hi = int(b[r]), int(b[r + 1])
    slab0 = torch.full((hi - lo, Y, Z, C), float(r + 1), device=dev)

    def check(vol):
        if r != 0:
            return True
        want = torch.cat([torch.full((int(b[k + 1] - b[k]),), float(k + 1)) for k in range(w)]).to(dev)
        return bool(torch.equal(vol[:, 0, 0, 0], want) and torch.equal(vol[:, -1, -1, -1], want))

    def timed(make, fn, reps=5):
        ts, ok = [], True
        for k in range(reps + 1):                   # the first round is the warm-up (communicator set-up, buffers)
            slab, vol = make()
            dist.barrier()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn(slab, vol)
            torch.cuda.synchronize()
            t = torch.tensor([time.perf_counter() - t0], device=cdev, dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            if k:
                ts.append(float(t.item()))
            ok = ok and check(vol)
            del slab, vol
        return min(ts) * 1e3, ok

    def slabs():                                    # peers: their slab; root: the zero volume with its slab in place
        if r != 0:
            return slab0.clone(), None
        vol = torch.zeros((X, Y, Z, C), device=dev)
        vol[lo:hi] = slab0
        return vol[lo:hi], vol

    def dense():
        vol = torch.zeros((X, Y, Z, C), device=dev)
        vol[lo:hi] = slab0
        return None, vol

    moved = nbytes * (w - 1) / w
    legs = [("slab_gather_torch", slabs, lambda s_, v: mdist.slab_gather_torch(s_, v, (X, Y, Z, C), dev)),
            ("dense_reduce_torch", dense, lambda s_, v: dist.reduce(v, dst=0, op=dist.ReduceOp.SUM)),
            ("slab_gather_c_abi", slabs, lambda s_, v: mdist.volume_gather(s_, v, (X, Y, Z, C), dev)),
            ("dense_reduce_c_abi", dense, lambda s_, v: mdist.volume_reduce(v, dev, mode=1))]
    if backend != "nccl":                            # shared-GPU test hook: torch's dense reduce would need host staging
        legs = [l for l in legs if l[0] != "dense_reduce_torch"]
        res["note"] = "ranks share one GPU; RCCL entry points bound to MH_RCCL_LIB (test stand-in): times mean nothing"
    for name, make, fn in legs:
        try:
            ms, ok = timed(make, fn, reps=1 if fake else 5)
            res[name + "_ms"] = round(ms, 3)
            res[name + "_correct"] = ok
        except Exception as e:
            res[name + "_error"] = repr(e)[:200]
    for name in ("slab_gather_torch", "slab_gather_c_abi"):
        if name + "_ms" in res:
            res[name + "_GBps_into_root"] = round(moved / (res[name + "_ms"] * 1e-3) / 1e9, 1)
    res["xgmi_expectation"] = ("%d peers x %.0f GB/s links into the root: %.2f ms for %.0f MB"
                               % (w - 1, XGMI_LINK_GBS, moved / ((w - 1) * XGMI_LINK_GBS * 1e9) * 1e3, moved / 1e6))
    if "dense_reduce_torch_ms" in res:
        res["dense_reduce_GBps_volume"] = round(nbytes / (res["dense_reduce_torch_ms"] * 1e-3) / 1e9, 1)
    return res


def secondary_quantized(a, dev, recs, cams, my, cand=None):
    """The same iteration on maps that went through the reference's 8-bit file hand-off (integer degrees, conf/255 -- what
    every real capture delivers), uploaded as the pixel CODES themselves (PMVO.from_u8): the
    records are decoded on the GPU through the loaders' table, the two codes of a pixel stay resident for the tap gathers
    (2 B per tap), duplicate tap orientations are dropped exactly.  Timed like the headline loop; per-kernel times and
    rooflines like kernel_rooflines()."""
    import torch

    from monohair_amd import _lib, synth
    from monohair_amd.pmvo import PMVO

    V, H, W, P = a.views, a.height, a.width, a.patch * a.patch
    sc = synth.make_scene_codes(V, H, W, device=dev, seed=0)
    from monohair_amd.camera import cameras_from_list

    camd = cameras_from_list(sc["cams"])
    pm = PMVO.from_u8(camd, sc["depth"], sc["ori_u8"], sc["conf_u8"], sc["mask_u8"], device=dev, image_size=[H, W],
                      patch_size=a.patch, visible_threshold=1, conf_threshold=a.conf_threshold)
    del sc
    if a.variant:
        pm.set_option("search_variant", a.variant)
    streams = pm.side_streams(max(1, a.streams))

    def step(i):
        with torch.cuda.stream(streams[i % len(streams)]):
            return pm.forward(my[i % len(my)])

    for i in range(PREWARM + a.warmup):     # same set-up iterations as the headline loop
        step(i)
    torch.cuda.synchronize()
    # five timed rounds of --steps iterations; the median is the leg's value, all five are listed.  (tools/exp_slow_rounds.py:
    # the steady rate of this loop is flat to 1 %, but about one round in ten is 20 % slower -- a single call blocks ~6 ms
    # with no allocation, collection or ring growth anywhere, i.e. the host, 30 iterations ahead, waits on a device pause;
    # the median of three was caught by two such rounds more than once.)
    rounds = []
    for _ in range(5):
        t0 = time.perf_counter()
        for i in range(a.steps):
            step(a.warmup + i)
        torch.cuda.synchronize()
        rounds.append(time.perf_counter() - t0)
    dt = sorted(rounds)[2]
    out = {"value": round(a.steps / dt, 3), "unit": "iterations/s", "ms_per_step": round(dt / a.steps * 1e3, 4),
           "rounds_iterations_per_s": [round(a.steps / r, 1) for r in rounds],
           "maps": "8-bit file codes (PMVO.from_u8): 20 B/px decoded records + 2 B/px resident codes for the tap gathers"}
    try:
        out.update(kernel_rooflines(a, pm, my, dev, V, H, W, P, codes=True))
    except Exception as e:
        out["roofline"] = {"error": repr(e)[:300]}
    if cand is not None:
        # the whole exterior pass on these maps -- what a real capture's run of PMVO.py costs after the maps are loaded
        try:
            fp = secondary_full_pass(dev, pm, cand, None)
            out["full_pass"] = {k: fp[k] for k in ("value", "value_is", "steady_total_s", "filter_s", "optimize_s",
                                                   "refine_and_volume_s", "optimize_ms_per_iteration", "surface_points",
                                                   "iterations", "unit") if k in fp}
        except Exception as e:
            out["full_pass"] = {"error": repr(e)[:200]}
    return out


def secondary_full_pass(dev, pm, cand, dist):
    """Wall time of the whole exterior pass on this scene: filter_negative_points -> optimize ->
    refine (smoothing, shell points, voxel fit, Ori3D.mat / Occ3D.mat written), stages synchronised.  With N ranks the
    drivers shard the independent chunks over the GPUs and assemble the volume with mh_volume_reduce (monohair_amd/dist.py);
    the times are the maximum over the ranks."""
    import contextlib
    import io
    import shutil
    import tempfile
    import types

    import numpy as np
    import torch
    from scipy.spatial import KDTree

    from monohair_amd.pmvo import filter_negative_points, optimize, refine

    rng = np.random.default_rng(1)
    b = rng.normal(size=(2000, 3))
    b = b / np.linalg.norm(b, axis=1, keepdims=True) * 0.09          # stand-ins for the bust / scalp meshes
    scalp = b[b[:, 1] > 0.03] * (0.1 / 0.09)
    pm.set_head(KDTree(b), KDTree(scalp), scalp.max(0))
    if dist is not None:
        box = [tempfile.mkdtemp(prefix="mhbench_") if dist.get_rank() == 0 else None]
        dist.broadcast_object_list(box, src=0)
        tmp = box[0]
    else:
        tmp = tempfile.mkdtemp(prefix="mhbench_")
    args = types.SimpleNamespace(device=str(dev), output_path=tmp, save_root=tmp + "/optimize", save_path=tmp + "/refine",
                                 PMVO=types.SimpleNamespace(visible_threshold=1), data=types.SimpleNamespace(root=tmp))
    os.makedirs(args.save_path, exist_ok=True)
    T = {}

    def timed(name, fn):
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dist is not None:
            t = torch.tensor([dt], device=dev if dist.get_backend() == "nccl" else "cpu", dtype=torch.float64)
            dist.all_reduce(t, op=dist.ReduceOp.MAX)
            dt = float(t.item())
        T[name] = round(dt, 4)
        return r

    def one_pass(k):
        T.clear()
        # a fresh output directory per pass (overwriting the previous pass's 400 MB of .mat files would be timed too)
        args.output_path = tmp + "/pass%d" % k
        args.save_root, args.save_path = args.output_path + "/optimize", args.output_path + "/refine"
        args.data.root = args.output_path
        if dist is None or dist.get_rank() == 0:
            os.makedirs(args.save_path, exist_ok=True)
        with contextlib.redirect_stdout(io.StringIO()):               # the drivers print progress like the reference
            s_idx, s_pts, f_idx = timed("filter_s", lambda: filter_negative_points(cand, pm, args))
            sp, so, ml, _ = timed("optimize_s", lambda: optimize(s_pts, pm, args))
            timed("refine_and_volume_s", lambda: refine(sp, so, ml, pm, cand[:len(f_idx)][f_idx].astype(np.float32), args,
                                                       infer_inner=False, threshold=0.025, return_dense=False))
        T["total_s"] = round(sum(T.values()), 4)
        if dist is None or dist.get_rank() == 0:
            shutil.rmtree(args.output_path, ignore_errors=True)
        return dict(T), s_idx, s_pts, f_idx

    # The first pass also pays for this process's first allocations of the pass's buffers (what a one-shot `python PMVO.py`
    # run sees, next to its seconds of start-up and map loading); three more give the steady state.  The host side of
    # refine (numpy, file writes) shares the box with other jobs: the median pass is reported, all totals are listed.
    # everything this process has built so far (scenes, chunks, modules) goes to the collector's permanent generation: a
    # full collection in the middle of a 10 ms stage is a 20-30 ms pause with that many live objects
    import gc

    gc.collect()
    gc.freeze()
    first = one_pass(0)[0]
    runs = [one_pass(k) for k in (1, 2, 3)]
    runs.sort(key=lambda r: r[0]["total_s"])
    T, s_idx, s_pts, f_idx = runs[1]
    T["passes_total_s"] = [first["total_s"]] + [r[0]["total_s"] for r in runs]
    T["first_pass"] = first
    # what a user who runs the pass ONCE in a process sees is the first pass (this process's first use of the refine / volume
    # stages; the code objects are on the device since the context was created); the other three give the steady state
    T["value"] = first["total_s"]
    T["value_is"] = "first_pass.total_s"
    T["steady_total_s"] = T["total_s"]
    T["refine_path"] = dict(getattr(pm, "last_refine", {}))      # which form of refine ran (device-resident pass, prefetch adopted)
    T["optimize_ms_per_iteration"] = round(T["optimize_s"] * 1e3 / max(1, len(s_pts) // CHUNK + 1), 4)
    T.update(candidates=int(len(cand)), surface_points=int(s_idx.sum()), shell_points=int(f_idx.sum()),
             iterations=int(len(s_pts) // CHUNK + 1), unit="s", ranks=1 if dist is None else dist.get_world_size())
    if dist is None and not os.environ.get("MH_FULLPASS_PLAIN"):     # (tools/profile_fullpass.sh traces the plain passes only)
        # where the pass's time goes: one more pass with the drivers' stage timers on (device-synchronised at every stage
        # boundary, so it is slower than the passes above and not one of them)
        try:
            import monohair_amd.timing as tm

            tm.totals.clear()
            was, tm.ENABLED = tm.ENABLED, True
            keep = dict(T)               # (one_pass refills the shared dict)
            try:
                with contextlib.redirect_stderr(io.StringIO()):
                    inst = one_pass(9)[0]
            finally:
                tm.ENABLED = was
                T.clear()
                T.update(keep)
            T["instrumented_pass"] = {"total_s": inst["total_s"], "refine_and_volume_s": inst["refine_and_volume_s"],
                                      "stage_ms": {k: round(v * 1e3, 2) for k, v in tm.totals.items()},
                                      "note": "stage timers synchronise the device at every boundary: overlap between stages is "
                                              "lost here, the sum exceeds the untimed passes"}
        except Exception as e:
            T["instrumented_pass"] = {"error": repr(e)[:300]}
        try:
            T["roofline_kernels"] = full_pass_kernel_rows(dev, pm, cand, s_pts, cand[:len(f_idx)][f_idx])
        except Exception as e:          # (reported, never fatal for the line)
            T["roofline_kernels"] = {"error": repr(e)[:300]}
    if dist is None or dist.get_rank() == 0:
        shutil.rmtree(tmp, ignore_errors=True)
    return T


def full_pass_kernel_rows(dev, pm, cand, s_pts, shell_pts):
    """Roofline rows of the kernels of the exterior pass OUTSIDE the iterations: each launched
    alone on this scene's own arrays, HIP events on its stream, best of three.  Work models (stated per row):
      votes (mh_filter_rows_kernel + mh_filter_kernel for the rows with another summation order)
                              one centre record (16 B) + one mask sample (4 B) per (candidate, view)
      mh_knn_kernel           queries/s (latency of LDS sorts: no byte or FLOP model)
      mh_medoid_kernel        K^2 (|cos| + accumulate) pairs per point, 7 FLOP per pair (3 mul, 2 add, abs, add)
      mh_refine_loss_maps     one centre record per (point, view) + P taps of 16 B per visible (point, view)
      voxel fit               points/s through keys + stable sort + run heads + segmented medoid"""
    import ctypes

    import numpy as np
    import torch

    from monohair_amd import _lib
    from monohair_amd import pmvo_utils as U

    L, ctx = pm._L, pm._ctx
    V, P = pm.num_view, pm._side ** 2
    st = _lib.stream_ptr()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def timed(fn, reps=3):
        best = None
        for _ in range(reps + 1):
            torch.cuda.synchronize()
            ev[0].record()
            fn()
            ev[1].record()
            torch.cuda.synchronize()
            t = ev[0].elapsed_time(ev[1])
            best = t if best is None else min(best, t)
        return best

    rows = []
    cd = torch.from_numpy(np.ascontiguousarray(cand, dtype=np.float32)).to(dev)
    pts = torch.from_numpy(np.ascontiguousarray(s_pts, dtype=np.float32)).to(dev)
    M, N = int(cd.shape[0]), int(pts.shape[0])
    surf = torch.empty((M,), dtype=torch.uint8, device=dev)
    filt = torch.empty((M,), dtype=torch.uint8, device=dev)
    t = timed(lambda: _lib.check(L.mh_filter_points(ctx, _lib.ptr(cd), M, pm._side, float(pm.conf_threshold),
                                                    float(pm.visible_threshold), _lib.ptr(surf), _lib.ptr(filt), None, None,
                                                    M // 30, 0, M, st)))
    b = M * V * 20 + M * 12
    order = U.spatial_order(cd)
    t_sort = timed(lambda: U.spatial_order(cd))
    t_ord = timed(lambda: _lib.check(L.mh_filter_points_ordered(ctx, _lib.ptr(cd), M, pm._side, float(pm.conf_threshold),
                                                                float(pm.visible_threshold), _lib.ptr(surf), _lib.ptr(filt),
                                                                None, None, M // 30, 0, M, _lib.ptr(order), st)))
    for name, tt, note in (("mh_filter_rows_kernel<%d>, rows in the candidates' own (raster) order" % pm._side, t,
                            "every isolated 20-byte gather of a (point, view) pair moves its own line: the raster sweeps each "
                            "image once per slab of the volume"),
                           ("mh_filter_rows_kernel<%d>, rows in grid-cell order (mh_filter_points_ordered: what the drivers "
                            "launch)" % pm._side, t_ord, "a wave = one small cube; the ordering itself (mh_grid_build on a "
                            "5 mm grid) takes %.3f ms" % t_sort)):
        rows.append({"kernel": name, "bound": "hbm", "launch_ms": round(tt, 4), "points": M,
                     "algorithmic_bytes_per_launch": b, "achieved": round(b / tt / 1e6, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                     "frac": round(b / tt / 1e6 / HBM_PEAK_GBS, 4),
                     "point_views_per_s": round(M * V / tt / 1e6, 2), "point_views_unit": "G/s", "note": note})
    grid = U.GridKNN(pts, k_hint=100, device=dev)
    grid.query_nosync(pts, 100, self_query=True)
    t = timed(lambda: grid.query_nosync(pts, 100, self_query=True))
    idx, _ = grid.query_nosync(pts, 100, self_query=True)
    K = int(idx.shape[1])
    rows.append({"kernel": "mh_knn_kernel (k = %d self-query, two passes)" % K, "bound": "lds-latency", "launch_ms": round(t, 4),
                 "queries": N, "queries_per_s": round(N / t * 1e3, 0), "neighbours_per_s": round(N * K / t * 1e3, 0)})
    ori = torch.nn.functional.normalize(torch.randn((N, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(0)), dim=1)
    cen = torch.empty((N, 3), dtype=torch.float32, device=dev)
    t_all = timed(lambda: _lib.check(L.mh_medoid_indexed(ctx, _lib.ptr(ori), _lib.ptr(idx), N, K, _lib.ptr(cen), None, st)))
    n1 = min(N, CHUNK)
    t_one = timed(lambda: _lib.check(L.mh_medoid_indexed(ctx, _lib.ptr(ori), _lib.ptr(idx), n1, K, _lib.ptr(cen), None, st)))
    for name, n, tt in (("all points in one launch", N, t_all), ("one %d-point chunk of the Gauss-Seidel chain" % n1, n1, t_one)):
        fl = n * K * K * 7
        rows.append({"kernel": "mh_medoid_kernel (indexed, K = %d): %s" % (K, name), "bound": "valu", "launch_ms": round(tt, 4),
                     "pairs": n * K * K, "gpairs_per_s": round(n * K * K / tt / 1e6, 1),
                     "achieved": round(fl / tt / 1e9, 2), "peak": VALU_PEAK_TF, "unit": "TFLOP/s",
                     "frac": round(fl / tt / 1e9 / VALU_PEAK_TF, 4)})
    # visible (point, view) pairs of the surface points (the loss kernel gathers a patch only for those)
    nvis = 0
    for a0 in range(0, N, 20000):
        sub = pts[a0:a0 + 20000]
        vis = torch.empty((V, sub.shape[0]), dtype=torch.float32, device=dev)
        tmp = [torch.empty((V, sub.shape[0]) + sh, dtype=torch.float32, device=dev) for sh in ((2,), (), ())]
        scratch, need = pm._get_scratch(sub.shape[0])
        _lib.check(L.mh_forward_prepare(ctx, _lib.ptr(sub), sub.shape[0], pm._side, float(pm.conf_threshold), _lib.ptr(vis),
                                        _lib.ptr(tmp[0]), _lib.ptr(tmp[1]), _lib.ptr(tmp[2]), _lib.ptr(scratch), need, st))
        nvis += int((vis != -1).sum().item())
    loss = torch.empty((N,), dtype=torch.float32, device=dev)
    t = timed(lambda: _lib.check(L.mh_refine_loss_maps(ctx, _lib.ptr(pts), _lib.ptr(ori), 0.005, 4.0, N, pm._side,
                                                       float(pm.conf_threshold), _lib.ptr(loss), None, CHUNK, 0, N, st)))
    b = N * V * 16 + nvis * P * 16 + N * 28
    rows.append({"kernel": "mh_refine_loss_maps_kernel<%d> (lane = tap)" % pm._side, "bound": "hbm", "launch_ms": round(t, 4),
                 "points": N, "visible_pairs": nvis, "algorithmic_bytes_per_launch": b, "achieved": round(b / t / 1e6, 1),
                 "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(b / t / 1e6 / HBM_PEAK_GBS, 4)})
    nv = N + len(shell_pts)
    vp = torch.cat([pts, torch.from_numpy(np.ascontiguousarray(shell_pts, dtype=np.float32)).to(dev)], 0)
    vo = torch.nn.functional.normalize(torch.randn((nv, 3), device=dev, generator=torch.Generator(device=dev).manual_seed(1)), dim=1)
    import time as _t

    U.voxel_fit_device(vp, vo, nv, dev)
    torch.cuda.synchronize()
    t0 = _t.perf_counter()
    vox, _ = U.voxel_fit_device(vp, vo, nv, dev)
    tv = (_t.perf_counter() - t0) * 1e3
    rows.append({"kernel": "voxel fit (mh_voxel_key + radix sort + mh_segment_heads + mh_medoid_kernel<segmented>)",
                 "bound": "launch-latency", "wall_ms": round(tv, 4), "points": nv, "voxels": int(len(vox)),
                 "points_per_s": round(nv / tv * 1e3, 0)})
    return rows


def secondary_gabor(a, dev):
    """The other kernel family of the path: the per-view Gabor orientation bank on one
    synthetic view of the benchmark's image size, FP32-MFMA im2col kernel, HIP events around 10 launches.
    Compute bound: 2*180*289 FLOP per pixel against 12 B; peak = 157.3 TFLOP/s dense fp32 matrix."""
    import numpy as np
    import torch

    from monohair_amd.gabor import calOrientationGabor

    H, W = a.height, a.width
    g = torch.Generator(device="cpu").manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    img = (0.25 * torch.cos(2 * np.pi * (0.6 * xx + 0.8 * yy) / 4.0) + 0.02 * torch.randn((H, W), generator=g)).float().to(dev)
    gab = calOrientationGabor(device=dev)
    gab.filter_index(img)
    torch.cuda.synchronize()
    runs = []
    for _ in range(3):      # the first round after the host-side set-up runs at lower clocks: best of three, all listed
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            gab.filter_index(img)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / 10)
    ms = min(runs)
    tf = 2.0 * 180 * 289 * H * W / ms / 1e9
    prof = {}
    try:
        prof = json.load(open(os.path.join(ROOT, "profiles", "traffic.json"))).get("gabor_stage", {})
    except Exception:
        pass
    return {"metric": "Gabor bank views/s", "value": round(1e3 / ms, 1), "unit": "views/s", "ms_per_view": round(ms, 3),
            "image": [H, W], "kernel": "mh_gabor_mfma2_kernel", "rounds_ms": [round(r, 3) for r in runs],
            "roofline": {"bound": "mfma", "achieved": round(tf, 1), "peak": 157.3, "unit": "TFLOP/s",
                         "frac": round(tf / 157.3, 4), "traffic": prof.get("bank_traffic_bytes"),
                         "traffic_source": PROFILE_SOURCE if prof else None}}


def secondary_gabor_sharded(a, dev, dist, backend):
    """The Gabor stage as the north star shards it (GaborFilter.py:231-237 is a loop over the views): the
    --views gray uint8 images are resident on every rank, view i is filtered by rank i % N (monohair_amd.gabor.
    orientation_maps_device: DoG -> bank -> 8-bit codes, two HIP streams per rank), ONE all_gather of the 2 B/px code planes
    leaves all views' codes on every rank (what PMVO.from_u8 takes).  Barrier + synchronize on both sides, max over ranks,
    best of three rounds; the all_gather alone is timed the same way on zero planes.  Runs at every N including 1."""
    import numpy as np
    import torch

    from monohair_amd import dist as mdist
    from monohair_amd.gabor import calOrientationGabor, orientation_maps_device

    V, H, W = a.views, a.height, a.width
    world = dist.get_world_size() if dist is not None else 1
    rank = dist.get_rank() if dist is not None else 0
    g = torch.Generator(device="cpu").manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    img = (127 + 70 * torch.cos(2 * np.pi * (0.6 * xx + 0.8 * yy) / 4.0) + 6 * torch.randn((H, W), generator=g))
    img = img.clamp(0, 255).to(torch.uint8).to(dev)
    views = [img.roll(7 * k, 1) for k in range(V)]
    gab = calOrientationGabor(device=dev)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()

    def over_ranks(dt):
        if dist is None:
            return dt
        t = torch.tensor([dt], device=dev if backend == "nccl" else "cpu", dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    orientation_maps_device(views, dev, gab, return_codes=True)        # warm: streams, scratch, the collective
    rounds = []
    for _ in range(3):
        barrier()
        t0 = time.perf_counter()
        k8, c8 = orientation_maps_device(views, dev, gab, return_codes=True)
        barrier()
        rounds.append(over_ranks(time.perf_counter() - t0))
    mine = [i for i in range(V) if mdist.owner(i) == rank]
    local = [torch.zeros((2, H, W), dtype=torch.uint8, device=dev) for _ in mine]
    gathers = []
    for _ in range(3):
        barrier()
        t0 = time.perf_counter()
        mdist.all_gather_views(local, V, (2, H, W), torch.uint8, dev)
        barrier()
        gathers.append(over_ranks(time.perf_counter() - t0))
    dt, tg = min(rounds), min(gathers)
    check = [int(k8.sum().item()), int(c8.sum().item())]
    agree = True
    if dist is not None:
        every = [None] * world
        dist.all_gather_object(every, check)
        agree = all(e == every[0] for e in every)
    return {"metric": "Gabor stage views/s, views sharded over the ranks + one all_gather of the code planes",
            "value": round(V / dt, 1), "unit": "views/s", "n_gpus": world, "views": V, "image": [H, W],
            "wall_ms": round(dt * 1e3, 3), "rounds_ms": [round(r * 1e3, 3) for r in rounds],
            "all_gather_ms": round(tg * 1e3, 3), "all_gather_bytes": int(V * 2 * H * W),
            "views_per_rank": [len([i for i in range(V) if mdist.owner(i, world) == k]) for k in range(world)],
            "codes_checksum": check, "codes_agree_on_all_ranks": bool(agree),
            "scaling": "strong (the view count is fixed; each rank filters ceil(V/N) views)"}


def secondary_gabor_stage(a, dev):
    """The Gabor STAGE per view, device to device: gray uint8 image resident in HBM -> DoG prefilter
    (float64, mh_dog: 2 launches) -> 180-kernel bank (mh_gabor_mfma_kernel) -> confidence + the two 8-bit file codes the
    reference hands to PMVO (mh_gabor_finish_kernel).  One call of mh_gabor_view per view; HIP events around 10 views, and
    around the DoG alone."""
    import numpy as np
    import torch

    from monohair_amd.gabor import calOrientationGabor, difference_of_gaussians_device

    H, W = a.height, a.width
    g = torch.Generator(device="cpu").manual_seed(0)
    yy, xx = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    img = (127 + 70 * torch.cos(2 * np.pi * (0.6 * xx + 0.8 * yy) / 4.0) + 6 * torch.randn((H, W), generator=g))
    views = [(img.roll(7 * k, 1)).clamp(0, 255).to(torch.uint8).to(dev) for k in range(4)]
    gab = calOrientationGabor(device=dev)
    gab.view(views[0])
    torch.cuda.synchronize()
    runs, dogs = [], []
    for _ in range(3):
        e = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        e[0].record()
        for k in range(10):
            out = gab.view(views[k % 4])
        e[1].record()
        e[2].record()
        for k in range(10):
            difference_of_gaussians_device(views[k % 4], 0.4, 10, dev, out32=True)
        e[3].record()
        torch.cuda.synchronize()
        runs.append(e[0].elapsed_time(e[1]) / 10)
        dogs.append(e[2].elapsed_time(e[3]) / 10)
    one_stream_ms, dog_ms = min(runs), min(dogs)
    # what orientation_maps_device does: views rotate over two HIP streams (the DoG / finish launches of one view run in the
    # tail of the previous view's bank kernel); wall clock around 20 views
    sts = [torch.cuda.Stream() for _ in range(2)]
    for st in sts:
        with torch.cuda.stream(st):
            gab.view(views[0])
    torch.cuda.synchronize()
    rot = []
    for _ in range(3):
        t0 = time.perf_counter()
        for k in range(20):
            with torch.cuda.stream(sts[k % 2]):
                out = gab.view(views[k % 4])
        torch.cuda.synchronize()
        rot.append((time.perf_counter() - t0) * 1e3 / 20)
    ms = min(rot)
    tf = 2.0 * 180 * 289 * H * W / ms / 1e9
    dog_bytes = H * W * (1 + 16 + 16 + 4)        # codes in, two float64 planes written and read back, float32 out
    prof = {}
    try:
        prof = json.load(open(os.path.join(ROOT, "profiles", "traffic.json"))).get("gabor_stage", {})
    except Exception:
        pass
    return {"metric": "Gabor stage views/s (uint8 image -> DoG -> bank -> 8-bit codes)", "value": round(1e3 / ms, 1),
            "unit": "views/s", "ms_per_view": round(ms, 3), "image": [H, W], "launches_per_view": 5,
            "streams": 2, "rounds_ms": [round(r, 3) for r in rot],
            "one_stream_ms_per_view": round(one_stream_ms, 3), "one_stream_rounds_ms": [round(r, 3) for r in runs],
            "dog_ms": round(dog_ms, 4), "dog_fraction_of_stage": round(dog_ms / one_stream_ms, 4),
            "dog_GBps": round(dog_bytes / (dog_ms * 1e-3) / 1e9, 1), "dog_bytes_model": "H*W*(1 + 2*8 + 2*8 + 4)",
            "codes_checksum": [int(out[3].sum().item()), int(out[4].sum().item())],
            "roofline": {"kernel": "mh_gabor_mfma2_kernel (whole stage timed)", "bound": "mfma", "achieved": round(tf, 1),
                         "peak": 157.3, "unit": "TFLOP/s", "frac": round(tf / 157.3, 4),
                         "traffic": prof.get("traffic_bytes"), "mfma_busy": prof.get("mfma_busy"),
                         "traffic_source": PROFILE_SOURCE if prof else None,
                         "mfma_busy_source": PROFILE_SOURCE if prof else None}}


class ParityError(AssertionError):
    pass


def compare_with_oracle(gpu_result, o_res, n):
    """(orientation, loss, high-confidence flag) of a timed step vs oracle.forward on the same points -> the line's
    `parity_check` object; raises ParityError on any differing bit."""
    import numpy as np

    _, g_ori, g_loss, g_hc = gpu_result
    g_ori, g_loss, g_hc = g_ori[:n].cpu().numpy(), g_loss[:n].cpu().numpy(), g_hc[:n].cpu().numpy()
    _, o_ori, o_loss, o_hc = o_res
    exact = (np.array_equal(g_ori, o_ori, equal_nan=True) and np.array_equal(g_loss, o_loss, equal_nan=True)
             and np.array_equal(g_hc, o_hc))
    parity = {"points": int(n), "bit_exact": bool(exact), "finite_losses": int(np.isfinite(o_loss).sum()),
              "what": "(orientation, loss, high-confidence flag) returned by the LAST step of the timed region == "
                      "oracle.forward on the same chunk, compared in this run"}
    if not exact:
        bad = int((~((g_loss == o_loss) | (np.isnan(g_loss) & np.isnan(o_loss)))).sum())
        raise ParityError("bench.py: the timed step's outputs differ from the CPU oracle on %d of %d points" % (bad, n))
    return parity


def cpu_baseline(a, scene, recs, chunk, gpu_ms, gpu_result, check_only=0):
    """The CPU oracle (oracle/pmvo_oracle.c, OpenMP over points) timed on this host on a bounded sample of the
    same iteration: the first n points of the chunk against all views.  `chunk` is the chunk the LAST step of the timed
    region processed and `gpu_result` what that step returned: the oracle's (orientation, loss, high-confidence flag) for the
    sample is compared with it bit for bit -> (cpu_baseline, parity_check); a mismatch raises ParityError.
    check_only > 0 (the N > 1 runs, where the CPU baseline is not reported): one untimed oracle pass over the chunk, only the
    comparison is returned -> (None, parity_check).  This function is the one place bench.py uses the oracle."""
    import numpy as np

    import oracle
    from monohair_amd.pmvo import depth_offsets

    views = oracle.Views(recs, scene["depth"].cpu().numpy(), scene["ori"].cpu().numpy(),
                         scene["conf"].cpu().numpy(), scene["mask"].cpu().numpy())
    cores = oracle.num_threads()
    offs = depth_offsets(90)
    # (A/B runs with --option: the oracle follows the same arithmetic options as the context)
    opts = dict(kv.split("=") for kv in a.option)
    oracle.set_reproject_rule({0: "group", 1: "mid", 2: "chain"}[int(opts.get("reproject_rule", 0))],
                              int(opts.get("reproject_fma_min_cols", oracle.REF_FMA_MIN_COLS)))
    oracle.set_sum_block(int(opts.get("sum_block", 32)))
    # A point's answer depends on the batch it is in (the (rank, base view) group sizes select how the reference's sgemms
    # round, the batch's last samples sit in the trailing columns of its sums): the comparison is always WHOLE chunk against
    # whole chunk, whatever part of it the timed sample covers.
    if check_only:
        n = len(chunk)
        return None, compare_with_oracle(gpu_result, oracle.forward(views, chunk, a.patch, a.conf_threshold, offs), n)
    n = a.cpu_points if a.cpu_points > 0 else len(chunk)
    # repeat the sample until >= 12 s of CPU work have been timed (bounded: at most 40 repeats)
    t, reps = 0.0, 0
    while reps < 40 and (t < 12.0 or reps == 0):
        t0 = time.perf_counter()
        o_res = oracle.forward(views, chunk[:n], a.patch, a.conf_threshold, offs)
        t += time.perf_counter() - t0
        reps += 1
    if n < len(chunk):
        o_res = oracle.forward(views, chunk, a.patch, a.conf_threshold, offs)
    parity = compare_with_oracle(gpu_result, o_res, len(chunk))
    n_total = n * reps
    its = (n_total / float(CHUNK)) / t
    return {
        "value": round(its, 5),
        "unit": "iterations/s",
        "cores": cores,
        "kind": "port",
        "sample": "%d x %d points of one %d-point iteration, all %d views, C oracle (oracle/pmvo_oracle.c) with "
                  "OpenMP on %d threads, %.1f s of wall time; the unmodified reference (torch-CPU, 8 vCPU Xeon, "
                  "BASELINE.md §2) needs 250-500 s per iteration = 0.002-0.004 iterations/s" % (reps, n, CHUNK, a.views,
                                                                                              cores, t),
    }, parity


if __name__ == "__main__":
    main()
