"""GPU: every C-ABI call of tests/guard_cases.py on an arena of tests/guard_arena.py -- its buffers in one tensor with seeded
random guards between them.  Per case: no guard is hit, no input changes, two different fills give the same output bytes (no
dependence on uninitialised scratch or on an output's previous contents), what is documented as not written keeps its fill,
and the outputs equal the expected ones.  Entry points that take a scratch size refuse one byte less with MH_ERR_ARG and
write nothing at all."""
import numpy as np
import pytest

import guard_cases as G
from guard_arena import GuardError, identical, run_twice

pytestmark = pytest.mark.gpu

CASES = [pytest.param(c, id="%s-%s" % (e, c.id)) for e in sorted(G.GUARDED) for c in G.GUARDED[e]]
UNDERSIZED = [pytest.param(G.GUARDED[e][0], id=e) for e in sorted(G.GUARDED) if G.GUARDED[e][0].scratch]


def _equal(got, want):
    """the same shape, type and BITS (a NaN of another payload or sign is another value; so is a zero of the other sign)"""
    return got.shape == want.shape and got.dtype == want.dtype and \
        np.ascontiguousarray(got).tobytes() == np.ascontiguousarray(want).tobytes()


@pytest.mark.parametrize("case", CASES)
def test_guarded_call(case):
    call = case.build()
    written = {}

    def run(seed):
        rc, arena = G.execute(call, seed)
        assert rc == call.rc, (rc, G._lib_().mh_last_error())
        if rc != 0:                 # a refusal: every buffer still holds what it was given, every Out its fill
            arena.untouched()
            return {}
        outs = arena.outputs()
        for name, want in call.expect.items():
            if callable(want):          # a statement of its own, on all outputs of the call
                want(outs)
                continue
            got = outs[name]
            free, same = None, False
            if isinstance(want, G.Partial):
                want, free, same = want.values, want.free, want.same
            if isinstance(want, np.ma.MaskedArray):
                mask = np.ma.getmaskarray(want)
                required = ~mask                      # must hold the expected value; the same for both fills
                keeps = mask if free is None else mask & ~free      # must still hold the fill
                written[name] = required | free if same else required       # what both fills must agree on
                fill = arena.raw(name, "fill").view(got.dtype).reshape(got.shape)
                bad = np.flatnonzero((keeps & (got.view(_bits(got)) != fill.view(_bits(got)))).reshape(-1))
                if len(bad):
                    raise GuardError(name, "unwritten-changed", bad[0] * got.dtype.itemsize,
                                     (bad[-1] + 1) * got.dtype.itemsize - 1, "elements %d .. %d" % (bad[0], bad[-1]))
                g, w = got[required], np.asarray(want.data, dtype=want.dtype)[required]
                assert _equal(g, w), (name, np.flatnonzero(g != w)[:5])
            else:
                want = np.asarray(want)
                assert _equal(got, want.reshape(got.shape) if want.size == got.size else want), \
                    (name, got.reshape(-1)[:8], want.reshape(-1)[:8])
        return outs

    try:
        a, b = run_twice(run)
    finally:
        if call.after is not None:
            call.after()
    identical(a, b, written)


def _bits(a):
    return {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize]


@pytest.mark.parametrize("case", UNDERSIZED)
def test_scratch_one_byte_short_is_refused_and_nothing_is_written(case):
    call = case.build().undersized()
    rc, arena = G.execute(call, 1)
    assert rc == G.MH_ERR_ARG, rc
    arena.untouched()
