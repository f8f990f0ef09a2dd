"""GPU: the four entry points of the silhouette carve on the guard arena of tests/guard_arena.py, by the checks of
tests/test_guard_gpu.py (no guard is hit, no input changes, two fills give the same output bytes, the outputs equal the numpy
restatement; a scratch one byte short is refused and nothing is written).  Importing tests/hair_carve_guard_cases.py enters the
cases into the ledger of tests/guard_cases.py."""
import pytest

import guard_cases as G
import hair_carve_guard_cases as HC
import test_guard_gpu as TG

pytestmark = pytest.mark.gpu

CASES = [pytest.param(c, id="%s-%s" % (e, c.id)) for e in HC.ENTRIES for c in G.GUARDED[e]]
UNDERSIZED = [pytest.param(G.GUARDED[e][0], id=e) for e in HC.ENTRIES if G.GUARDED[e][0].scratch]


def test_the_carve_is_in_the_ledger():
    assert all(G.FAMILY[e] == "F" and e not in G.NOT_GUARDED for e in HC.ENTRIES)
    assert len(CASES) == 10 and len(UNDERSIZED) == 2


@pytest.mark.parametrize("case", CASES)
def test_guarded_call(case):
    TG.test_guarded_call(case)


@pytest.mark.parametrize("case", UNDERSIZED)
def test_scratch_one_byte_short_is_refused_and_nothing_is_written(case):
    TG.test_scratch_one_byte_short_is_refused_and_nothing_is_written(case)
