"""Helper (not a test): every buffer of one C-ABI call laid out in ONE uint8 tensor, guard | buffer | guard | ... | guard,
so that a write outside a buffer lands in memory the test owns and can be read back.

  - every buffer starts on a 256-byte boundary (as the tensor library aligns its own allocations);
  - every guard is at least GUARD = 4096 bytes: more than one workgroup's widest store (256 lanes x 16 B);
  - the guard behind a buffer begins at the buffer's exact last byte + 1, not at the next aligned address;
  - guards and the bodies of Out / Scratch buffers are filled from numpy.random.default_rng(seed).bytes: never a constant,
    which a kernel can write by accident.

Roles: In(array) must come back unchanged; Out(shape, dtype) is the extent the header documents; InOut(array) is updated in
place; Scratch(nbytes) is exactly what the entry point's *_scratch_bytes() returns.  Arena.check() -- one synchronise, one
copy to the host -- raises GuardError naming the buffer, the side and the first and last offending byte.  run_twice() runs a
call with fills 1 and 2; identical() then requires the two sets of outputs to agree byte for byte, which is what exposes a
dependence on uninitialised scratch or on an output's previous contents."""
import ctypes

import numpy as np
import torch

ALIGN = 256
GUARD = 4096


class In:
    def __init__(self, array):
        self.array = np.ascontiguousarray(array)
        self.nbytes = self.array.nbytes


class InOut(In):
    pass


class Out:
    def __init__(self, shape, dtype):
        self.shape = (shape,) if np.isscalar(shape) else tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.nbytes = int(np.prod(self.shape, dtype=np.int64)) * self.dtype.itemsize


class Scratch:
    def __init__(self, nbytes):
        self.nbytes = int(nbytes)


class GuardError(AssertionError):
    """buffer: its name; side: "front" / "behind" (a guard was hit), "inside" (an In changed), "differs" (two fills gave
    other bytes), "unwritten-changed" (a part documented as not written lost its fill).  first / last: the first and last
    offending byte: for "behind" relative to the buffer's end (0 = the byte right behind its last byte), for "front" relative
    to its first byte (-1 = the byte right in front of it), otherwise the offset inside the buffer."""

    def __init__(self, buffer, side, first, last, note=""):
        self.buffer, self.side, self.first, self.last = buffer, side, int(first), int(last)
        super().__init__("%s: %s, bytes %d .. %d%s" % (buffer, side, first, last, (" (%s)" % note) if note else ""))


def _up(x, a):
    return (x + a - 1) // a * a


class Arena:
    def __init__(self, buffers, seed, device):
        """buffers: {name: role}, laid out in this order"""
        self.roles = dict(buffers)
        self.offset = {}
        pos = GUARD
        for name, role in self.roles.items():
            pos = _up(pos, ALIGN)
            self.offset[name] = pos
            pos += role.nbytes + GUARD            # the guard begins at the exact end; the next start is rounded UP from it
        self.total = _up(pos, ALIGN)
        # the base itself must sit on the boundary the offsets assume
        fill = np.frombuffer(np.random.default_rng(seed).bytes(self.total), np.uint8).copy()
        self.fill = fill.copy()
        for name, role in self.roles.items():
            if isinstance(role, In):
                o = self.offset[name]
                fill[o:o + role.nbytes] = role.array.reshape(-1).view(np.uint8)
        self.initial = fill
        self.tensor = torch.from_numpy(fill.copy()).to(device)
        assert self.tensor.data_ptr() % ALIGN == 0 or self.tensor.device.type == "cpu"
        self.host = None

    # ---- addresses
    def ptr(self, name):
        return ctypes.c_void_p(self.tensor.data_ptr() + self.offset[name])

    def span(self, name):
        o = self.offset[name]
        return o, o + self.roles[name].nbytes

    def cpu_bytes(self):
        """the live bytes of a CPU arena (what a numpy "kernel" writes into)"""
        assert self.tensor.device.type == "cpu"
        return self.tensor.numpy()

    # ---- after the call
    def check(self):
        if self.tensor.device.type == "cuda":
            torch.cuda.synchronize(self.tensor.device)
        self.host = host = self.tensor.cpu().numpy().copy()
        names = list(self.roles)
        spans = [self.span(n) for n in names]
        # guards: before the first buffer, between neighbours (attributed to the nearer one), behind the last
        edges = [0] + [e for s in spans for e in s] + [self.total]
        for g in range(len(names) + 1):
            lo, hi = edges[2 * g], edges[2 * g + 1]
            bad = np.flatnonzero(host[lo:hi] != self.fill[lo:hi])
            if not len(bad):
                continue
            bad = bad + lo
            if g == 0:
                behind = bad[:0]
                front = bad
            elif g == len(names):
                behind, front = bad, bad[:0]
            else:
                mid = (lo + hi) // 2
                behind, front = bad[bad < mid], bad[bad >= mid]
            if len(behind):
                end = spans[g - 1][1]
                raise GuardError(names[g - 1], "behind", behind[0] - end, behind[-1] - end, "%d bytes" % len(behind))
            start = spans[g][0]
            raise GuardError(names[g], "front", front[0] - start, front[-1] - start, "%d bytes" % len(front))
        for name, (lo, hi) in zip(names, spans):
            if type(self.roles[name]) is In:
                bad = np.flatnonzero(host[lo:hi] != self.initial[lo:hi])
                if len(bad):
                    raise GuardError(name, "inside", bad[0], bad[-1], "an input was modified")
        return self

    def untouched(self):
        """after check(): nothing at all was written (a refused call)"""
        bad = np.flatnonzero(self.host != self.initial)
        if len(bad):
            for name in self.roles:
                lo, hi = self.span(name)
                if lo <= bad[0] < hi:
                    raise GuardError(name, "inside", bad[0] - lo, min(bad[-1], hi - 1) - lo, "written by a refused call")
            raise GuardError("arena", "inside", bad[0], bad[-1], "written by a refused call")

    def raw(self, name, which="host"):
        lo, hi = self.span(name)
        return {"host": self.host, "fill": self.fill}[which][lo:hi]

    def get(self, name):
        role = self.roles[name]
        raw = self.raw(name)
        if isinstance(role, Out):
            return raw.view(role.dtype).reshape(role.shape)
        if isinstance(role, In):
            return raw.view(role.array.dtype).reshape(role.array.shape)
        return raw

    def outputs(self):
        return {n: self.get(n).copy() for n, r in self.roles.items() if isinstance(r, (Out, InOut))}


def run_twice(run):
    """run(seed) -> {name: array} of the outputs of one call on an arena filled with `seed`: both sets, fills 1 and 2"""
    return run(1), run(2)


def identical(a, b, written=None):
    """the outputs of two fills agree byte for byte; written: {name: bool mask over the elements} restricts the comparison to
    what the entry point is documented to write (the rest is checked against its fill by the caller)"""
    assert sorted(a) == sorted(b)
    for name in a:
        x, y = np.ascontiguousarray(a[name]), np.ascontiguousarray(b[name])
        ne = x.reshape(-1).view(np.uint8) != y.reshape(-1).view(np.uint8)
        if written is not None and name in written:
            ne &= np.repeat(np.broadcast_to(written[name], x.shape).reshape(-1), x.dtype.itemsize)
        bad = np.flatnonzero(ne)
        if len(bad):
            raise GuardError(name, "differs", bad[0], bad[-1], "two fills give other bytes: element %d" %
                             (bad[0] // x.dtype.itemsize))
