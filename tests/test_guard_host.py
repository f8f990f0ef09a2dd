"""CPU-only: the guard harness of tests/guard_arena.py catches what it is for -- numpy "kernels" with planted errors on a CPU
arena are reported with the right buffer, side and offset -- and the ledger of tests/guard_cases.py is complete: every entry
point of include/mh_pmvo.h that writes caller-owned device memory is guarded or listed with a reason."""
import re

import numpy as np
import pytest

import guard_cases as G
from guard_arena import ALIGN, GUARD, Arena, GuardError, In, InOut, Out, Scratch, identical, run_twice
from test_abi import declared_parameters

N = 37            # 37 floats = 148 bytes: the buffer ends 108 bytes in front of the next 256-byte boundary


def _buffers():
    return {"x": In(np.arange(N, dtype=np.float32)), "y": Out(N, np.float32), "acc": InOut(np.ones(3, np.int64)),
            "scratch": Scratch(101)}


def _kernel(arena, plant=None):
    """y = 2 x, acc += 1, the scratch used as a byte counter; `plant` adds one error"""
    mem = arena.cpu_bytes()

    def view(name, dtype):
        lo, hi = arena.span(name)
        return mem[lo:hi].view(dtype)
    x, y, acc, s = view("x", np.float32), view("y", np.float32), view("acc", np.int64), view("scratch", np.uint8)
    s[:] = 7
    was = y[11:12].copy()
    y[:] = 2 * x
    acc += 1
    if plant == "behind-out":
        mem[arena.span("y")[1]] ^= 0x55
    elif plant == "front-out":
        mem[arena.span("y")[0] - 1] ^= 0x55
    elif plant == "behind-scratch":
        mem[arena.span("scratch")[1]] ^= 0x55
    elif plant == "in":
        x[5] = -1.0
    elif plant == "unwritten":
        y[11:12].view(np.uint32)[:] = was.view(np.uint32)        # element 11 left as it was


def _run(plant=None):
    def run(seed):
        arena = Arena(_buffers(), seed, "cpu")
        _kernel(arena, plant)
        return arena.check().outputs()
    return run


def test_layout():
    arena = Arena(_buffers(), 1, "cpu")
    names = list(arena.roles)
    assert arena.span(names[0])[0] >= GUARD
    for a, b in zip(names, names[1:]):
        assert arena.span(b)[0] - arena.span(a)[1] >= GUARD              # from the exact last byte + 1
    assert arena.total - arena.span(names[-1])[1] >= GUARD
    for n in names:
        assert arena.span(n)[0] % ALIGN == 0 and arena.span(n)[1] - arena.span(n)[0] == arena.roles[n].nbytes
    assert arena.span("y")[1] % ALIGN != 0 and arena.span("scratch")[1] % 4 != 0
    # seeded, not constant, and another seed gives other bytes
    other = Arena(_buffers(), 2, "cpu")
    assert len(np.unique(arena.fill)) == 256 and (arena.fill != other.fill).mean() > 0.9
    assert np.array_equal(arena.fill, Arena(_buffers(), 1, "cpu").fill)
    lo, hi = arena.span("x")
    assert np.array_equal(arena.cpu_bytes()[lo:hi].view(np.float32), np.arange(N, dtype=np.float32))


def test_a_well_behaved_kernel_passes():
    a, b = run_twice(_run())
    identical(a, b)
    assert sorted(a) == ["acc", "y"]
    assert np.array_equal(a["y"], 2 * np.arange(N, dtype=np.float32)) and np.array_equal(a["acc"], [2, 2, 2])


@pytest.mark.parametrize("plant,buffer,side,first,last", [
    ("behind-out", "y", "behind", 0, 0),
    ("front-out", "y", "front", -1, -1),
    ("behind-scratch", "scratch", "behind", 0, 0),
    ("in", "x", "inside", 22, 23),              # float 5 = -1.0 instead of 5.0: bytes 20 .. 23, of which the upper two differ
])
def test_a_planted_error_is_reported_with_buffer_and_offset(plant, buffer, side, first, last):
    with pytest.raises(GuardError) as e:
        _run(plant)(1)
    assert (e.value.buffer, e.value.side, e.value.first, e.value.last) == (buffer, side, first, last)
    assert buffer in str(e.value) and side in str(e.value)


def test_an_unwritten_element_shows_as_two_fills_that_differ():
    a, b = run_twice(_run("unwritten"))        # each run passes check(): nothing outside was touched
    with pytest.raises(GuardError) as e:
        identical(a, b)
    assert (e.value.buffer, e.value.side) == ("y", "differs") and 44 <= e.value.first <= e.value.last <= 47
    # ... unless the entry point documents that element as not written
    written = np.ones(N, bool)
    written[11] = False
    identical(a, b, {"y": written})


def test_a_refused_call_must_leave_everything():
    arena = Arena(_buffers(), 1, "cpu").check()
    arena.untouched()
    arena = Arena(_buffers(), 1, "cpu")
    _kernel(arena)
    with pytest.raises(GuardError) as e:
        arena.check().untouched()
    assert e.value.buffer == "y"


# ------------------------------------------------------------------------------------------------------ the ledger
HOST_ONLY = re.compile(r"^mh_(mat_|comm_|strands_accept$)")
NOT_CALLER_MEMORY = ("mh_ctx *ctx", "void *stream", "void *comm", "void *handle", "mh_ctx **out")


def writers():
    """entry points of include/mh_pmvo.h with a non-const pointer parameter that is caller-owned device memory"""
    out = []
    for name, (_, params) in declared_parameters(("mh_pmvo.h",)).items():
        if HOST_ONLY.match(name):
            continue
        if any("*" in p and not p.startswith("const ") and p not in NOT_CALLER_MEMORY for p in params):
            out.append(name)
    return sorted(out)


def test_the_ledger_is_complete():
    names = writers()
    assert len(names) > 80 and "mh_forward" in names and "mh_ctx_set_view" not in names and "mh_ctx_destroy" not in names
    both = set(G.GUARDED) & set(G.NOT_GUARDED)
    assert not both, both
    listed = set(G.GUARDED) | set(G.NOT_GUARDED)
    assert [n for n in names if n not in listed] == []
    assert [n for n in sorted(listed) if n not in names] == []
    assert all(G.GUARDED[n] for n in G.GUARDED)
    assert set(G.FAMILY) == listed and set(G.FAMILY.values()) <= set("ABCDEFG")
    # test_long_untouched_slots' two entry points carry a case of the new form
    assert {"mh_trace_seeds", "mh_trace_scalp"} <= set(G.GUARDED)


def test_not_guarded_holds_only_what_the_issue_allows():
    for name, reason in G.NOT_GUARDED.items():
        assert isinstance(reason, str) and len(reason) > 20, name
        assert G.FAMILY[name] in "BEG" or name == "mh_gabor_bank", (name, G.FAMILY[name])
    for fam in "ACDF":
        left = [n for n in G.NOT_GUARDED if G.FAMILY[n] == fam and n != "mh_gabor_bank"]
        assert left == [], (fam, left)


def test_every_scratch_taking_entry_point_has_an_undersized_case():
    for name, (_, params) in declared_parameters(("mh_pmvo.h",)).items():
        if "size_t scratch_bytes" in params and name in G.GUARDED:
            assert G.GUARDED[name][0].scratch, name
