"""The CPU oracle at sample counts other than 90, against the reference itself: tests/golden/pmvo_samples.npz holds the
reference's forward() with the default of sample_next_3d_pos set to S in {1, 16, 60, 100, 102} on the points of pmvo_small and
pmvo_quant, the samples of a direct call for the first 16 points, and its forward() at S = 1 on points handed to it alone
(tools/gen_golden_samples.py).  Every row, bit for bit, NaN == NaN: the oracle is the reference of
tests/test_search_shapes_gpu.py at those counts.  CPU only."""
import ast

import numpy as np
import pytest

import oracle
from conftest import golden_records, golden_scene, load_golden, rows_equal, scene_views

CASES = ["pmvo_small", "pmvo_quant"]
SAMPLE_COUNTS = (1, 16, 60, 100, 102)


def samples_golden():
    z = load_golden("pmvo_samples")[1]
    meta = ast.literal_eval(str(z["meta"]))
    assert tuple(meta["sample_counts"]) == SAMPLE_COUNTS
    return meta, z


@pytest.fixture(scope="module", params=CASES)
def case(request):
    meta, z = load_golden(request.param)
    views = scene_views(golden_scene(meta), golden_records(z))
    return request.param, meta, z, views


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_depth_offsets_of_other_counts(S):
    """depth_offsets(S) has not changed since the fixture was written (the generator stored ITS values, not a recording of the
    reference: what ties them to the reference is test_oracle_samples_equal_the_reference)"""
    from monohair_amd.pmvo import depth_offsets

    offs = depth_offsets(S)
    assert offs.shape == (S,) and offs.dtype == np.float32
    assert np.array_equal(offs, samples_golden()[1]["offsets__S%d" % S])


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_oracle_forward_equals_the_reference(case, S):
    from monohair_amd.pmvo import depth_offsets

    name, meta, z, views = case
    g = samples_golden()[1]
    ref = tuple(g["%s__S%d__%s" % (name, S, k)] for k in ("ori", "loss", "hc"))
    assert len(ref[1]) == len(z["points"])
    for kw in (dict(), dict(base_idx=z["base_idx"], base_val=z["base_val"])):     # the oracle's own ranking, the reference's
        got = oracle.forward(views, z["points"], meta["patch"], meta["thr"], depth_offsets(S), **kw)[1:]
        assert rows_equal(got, ref).all()
    assert np.isfinite(ref[1]).sum() > len(ref[1]) // 2


@pytest.mark.parametrize("S", SAMPLE_COUNTS)
def test_oracle_samples_equal_the_reference(case, S):
    from monohair_amd.pmvo import depth_offsets

    name, meta, z, views = case
    g, head = samples_golden()[1], samples_golden()[0]["head"]
    samples = oracle.sample_next(views, z["points"], z["base_idx"][0], z["Ori"], depth_offsets(S))
    ref = g["%s__S%d__samples" % (name, S)]
    assert ref.shape == (head, S, 3) and np.array_equal(samples[:head], ref, equal_nan=True)


def test_oracle_forward_of_one_point_and_one_sample_equals_the_reference(case):
    """N * S = 1: every fifth point handed to forward() alone at S = 1 -- the sample projected through the single-column sgemm,
    the views added as a contiguous dimension (oracle/pmvo_oracle.c: batch_is_single, tail_from_of)"""
    from monohair_amd.pmvo import depth_offsets

    name, meta, z, views = case
    g = samples_golden()[1]
    pick = g[name + "__S1__alone_pick"]
    ref = tuple(g["%s__S1__alone_%s" % (name, k)] for k in ("ori", "loss", "hc"))
    assert len(pick) == len(z["points"][::5]) and np.isfinite(ref[1]).sum() > len(pick) // 2
    got = [oracle.forward(views, z["points"][n:n + 1], meta["patch"], meta["thr"], depth_offsets(1))[1:] for n in pick]
    assert rows_equal(tuple(np.concatenate([r[k] for r in got]) for k in range(3)), ref).all()
    # ... and the batch matters: some of these rows differ from the same point's row in the whole batch
    whole = g[name + "__S1__loss"][pick]
    assert (np.isfinite(ref[1]) & (ref[1] != whole)).any()
