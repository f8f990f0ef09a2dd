"""GPU: the four entry points of the photo-consistent carve on the guard arena of tests/guard_arena.py, by the checks of
tests/test_guard_gpu.py (no guard is hit, no input changes, two fills give the same output bytes, the outputs equal the numpy
restatement).  Importing tests/hair_stereo_guard_cases.py enters the cases into the ledger of tests/guard_cases.py.  None of
the entry points takes a scratch."""
import pytest

import guard_cases as G
import hair_stereo_guard_cases as HS
import test_guard_gpu as TG

pytestmark = pytest.mark.gpu

CASES = [pytest.param(c, id="%s-%s" % (e, c.id)) for e in HS.ENTRIES for c in G.GUARDED[e]]


def test_the_stereo_pass_is_in_the_ledger():
    assert all(G.FAMILY[e] == "F" and e not in G.NOT_GUARDED for e in HS.ENTRIES)
    assert len(CASES) == 7 and not any(c.scratch for e in HS.ENTRIES for c in G.GUARDED[e])


@pytest.mark.parametrize("case", CASES)
def test_guarded_call(case):
    TG.test_guarded_call(case)
