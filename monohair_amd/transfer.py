"""class Transfer -- the one owner of a PMVO object's pinned host buffers, of the events that guard them and of its HIP
streams.

The lifetime rule of a pinned buffer whose copies go through mh_upload_pinned / mh_upload_async (torch's host caching
allocator does not track those copies: a dropped pinned block could be handed out again at once):
  * it may be REFILLED only after the event of the last copy out of it has passed;
  * it may be DROPPED only after every copy out of it is over -- replaced by a larger one (_release), or with the object
    (drain(), which PMVO.__del__ calls before the context goes).
Every upload buffer is an entry [pinned tensor, events of the copies out of it] in one of three containers, and _entries()
lists them all: a new kind of buffer is added there, nowhere else."""
import numpy as np
import torch

from . import _lib

_TORCH_OF = {np.dtype(np.float32): torch.float32, np.dtype(np.float64): torch.float64, np.dtype(np.uint8): torch.uint8}


class Transfer:
    SLOTS = 32          # slots of an upload ring

    def __init__(self, ctx, device):
        self._L, self._ctx, self.device = _lib.lib(), ctx, device
        self._rings = {}        # launch stream -> ring of upload_ring
        self._whole = None      # entry of upload_whole
        self._named = {}        # key -> entry of upload_named
        self._streams = {}      # name -> stream

    # ------------------------------------------------------------------ the lifetime rule
    def _entries(self):
        return [r["entry"] for r in self._rings.values()] + [e for e in [self._whole] if e] + list(self._named.values())

    @staticmethod
    def _release(entry):
        """wait for every asynchronous copy that still reads from an entry's pinned buffer"""
        for ev in entry[1] if entry else ():
            if ev is not None:
                ev.synchronize()

    def drain(self):
        """wait for every copy that still reads a pinned buffer of this object"""
        for entry in self._entries():
            self._release(entry)

    # ------------------------------------------------------------------ host -> device
    def upload_ring(self, points, stream=None):
        """Host numpy [N,3] -> float32 device tensor through a ring of PINNED staging slots per launch stream and
        an asynchronous copy.  `tensor.to(device)` from pageable memory blocks the host for ~0.2 ms per call (staging +
        wait) -- as long as a whole iteration takes on 8-bit maps, which made the loop of `optimize` host-bound there.
        The float64 -> float32 cast happens in the copy into the staging buffer (numpy's rounding = the reference's
        `.type(torch.float)`, PMVO.py:40)."""
        n = int(points.shape[0])
        if n == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=self.device)
        cs = torch.cuda.current_stream(self.device) if stream is None else stream
        ring = self._rings.get(cs.cuda_stream)
        if ring is None or ring["cap"] < n:
            # ONE pinned slab of 32 slots per launch stream (3 MB), allocated on the stream's first call (a ring that grew
            # slot by slot paid a pinned allocation -- milliseconds, and it drains the device -- up to 32 times per stream
            # during the first few hundred iterations of a loop); a slab that is too small is released, then replaced
            self._release(ring and ring["entry"])
            cap = max(n, 8192)
            slab = torch.empty((self.SLOTS, cap, 3), dtype=torch.float32, pin_memory=True)
            ring = self._rings[cs.cuda_stream] = {"cap": cap, "entry": [slab, [None] * self.SLOTS], "np": slab.numpy(),
                                                  "i": 0, "ptr": slab.data_ptr()}
        # slots are used in ring order (copies of one stream complete in order); a slot whose copy is still pending means the
        # host is 32 iterations ahead of a GPU-bound loop: only then does it wait
        k = ring["i"] % self.SLOTS
        ring["i"] += 1
        evs = ring["entry"][1]
        ev = evs[k]
        if ev is None:
            ev = evs[k] = torch.cuda.Event()
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

    def upload_whole(self, points, head=0, after_head=None):
        """One asynchronous upload of a whole [M,3] host array (float32 cast on the host, PMVO.py:40) through one pinned
        staging buffer that grows; the drivers then hand device slices to forward().
        head > 0: rows [0, head) are converted and copied first, `after_head(dev)` is called (the driver launches the first
        chunks there), then the rest is converted and copied -- the host-side conversion of a large float64 array (1 ms per
        300 k points) then runs while the GPU already works.  Returns (device tensor, float32 host view of the staged rows --
        valid until the next call)."""
        m = int(points.shape[0])
        if m == 0:
            return torch.empty((0, 3), dtype=torch.float32, device=self.device), np.zeros((0, 3), np.float32)
        self._release(self._whole)
        if self._whole is None or self._whole[0].shape[0] < m:
            self._whole = [torch.empty((m, 3), dtype=torch.float32, pin_memory=True), [torch.cuda.Event()]]
        pinned, (ev,) = self._whole
        host = pinned.numpy()[:m]
        dev = torch.empty((m, 3), dtype=torch.float32, device=self.device)
        cs = torch.cuda.current_stream(self.device)
        head = min(max(int(head), 0), m) if after_head is not None else 0
        for part, (lo, hi) in enumerate(((0, head), (head, m))):
            if hi > lo:
                np.copyto(host[lo:hi], points[lo:hi], casting="same_kind")
                _lib.check(self._L.mh_upload_async(self._ctx, pinned.data_ptr() + lo * 12, dev.data_ptr() + lo * 12,
                                                   (hi - lo) * 12, cs.cuda_stream), "mh_upload_async")
            if part == 0 and after_head is not None:
                after_head(dev)
        ev.record(cs)
        return dev, host

    def upload_named(self, key, arr, dtype=np.float32):
        """Host array -> fresh device tensor of `dtype` through a pinned staging buffer kept per `key`: one conversion /
        copy on the host (numpy's rounding for float64 -> float32 = the reference's `.type(torch.float)`, PMVO.py:40), one
        asynchronous copy on the current stream.  `tensor.to(device)` from pageable memory blocks the host for the whole
        transfer; the drivers upload a pass's arrays while the GPU works."""
        a, dt = np.asarray(arr), np.dtype(dtype)
        nbytes = a.size * dt.itemsize
        if nbytes == 0:
            return torch.empty(a.shape, dtype=_TORCH_OF[dt], device=self.device)
        entry = self._named.get(key)
        self._release(entry)                  # the previous copy out of this buffer
        if entry is None or entry[0].numel() < nbytes:
            entry = self._named[key] = [torch.empty(nbytes, dtype=torch.uint8, pin_memory=True), [torch.cuda.Event()]]
        np.copyto(entry[0].numpy()[:nbytes].view(dt).reshape(a.shape), a, casting="same_kind")
        dev = torch.empty(a.shape, dtype=_TORCH_OF[dt], device=self.device)
        cs = torch.cuda.current_stream(self.device)
        _lib.check(self._L.mh_upload_pinned(self._ctx, entry[0].data_ptr(), dev.data_ptr(), nbytes, cs.cuda_stream),
                   "mh_upload_pinned")
        entry[1][0].record(cs)
        return dev

    # ------------------------------------------------------------------ device -> host
    @staticmethod
    def pinned_like(t):
        """a pinned host tensor of a device tensor's shape and dtype (torch's host allocator recycles the blocks: these
        copies are torch's own, which it tracks)"""
        return torch.empty(t.shape, dtype=t.dtype, pin_memory=True)

    def download(self, cp, after, tensors, into=None):
        """Device tensors -> pinned host arrays, copied on stream `cp` once `after` (an event, a stream, or None: what the
        caller made `cp` wait for) has passed.  into: pinned tensors to fill (rows of pinned_like tensors), fresh ones by
        default.  -> (numpy arrays, event that ends the copies).  (A caller with many downloads in a row makes `cp` current
        around them: entering a stream context costs more host time than the copies' enqueue.)"""
        if torch.cuda.current_stream(self.device) != cp:
            with torch.cuda.stream(cp):
                return self.download(cp, after, tensors, into)
        host = [self.pinned_like(t) for t in tensors] if into is None else into
        if isinstance(after, torch.cuda.Event):
            cp.wait_event(after)
        elif after is not None:
            cp.wait_stream(after)
        for h, t in zip(host, tensors):
            h.copy_(t, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(cp)
        return [h.numpy() for h in host], ev

    # ------------------------------------------------------------------ streams
    def stream(self, name, priority=None):
        """A named HIP stream owned by this object, created on first use (the drivers' launch / copy / side / prefetch
        streams; the per-stream search scratch is keyed by them)."""
        if name not in self._streams:
            self._streams[name] = (torch.cuda.Stream(device=self.device) if priority is None
                                   else torch.cuda.Stream(device=self.device, priority=int(priority)))
        return self._streams[name]
