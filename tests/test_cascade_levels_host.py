"""CPU: the C oracle against tests/golden/cascade_views.npz and tests/golden/consensus_levels.npz (tools/gen_golden_cascade.py:
the reference's own results at 255 .. 4095 views and 127 .. 9728 group members, the sizes at which ATen's cascade sums take
up another level) on every element, and ATen itself, in its AVX2 build, against the transcriptions the generator proved the
fixtures' sensitivity with."""
import os
import subprocess
import sys

import numpy as np
import pytest

import cascade_cases as cc
import oracle
from conftest import GOLDEN

eq = lambda a, b: np.array_equal(a, b, equal_nan=True)       # noqa: E731


@pytest.fixture(scope="module")
def views_file():
    return cc.load("cascade_views")


@pytest.fixture(scope="module")
def groups_file():
    return cc.load("consensus_levels")


def test_fixtures_hold_every_size_and_were_made_in_the_pinned_order(views_file, groups_file):
    for meta, sizes in ((views_file[0], cc.VIEW_COUNTS), (groups_file[0], cc.GROUP_SIZES)):
        assert meta["capability"] == "AVX2" and meta["torch"].startswith("2.10.") and meta["threads"] == [1, 8]
        assert tuple(sorted(meta["cases"])) == sizes
    for V, c in views_file[0]["cases"].items():       # a sum without level 2 changes recorded losses wherever it can
        sh = c["share_differing_without_level2"]
        assert (min(sh["prj_loss"], sh["forward"], sh["refine_cascade_rows"]) > 0) == (V >= cc.V_FEELS_LEVEL2), V
        assert (sh["refine_row_sum_rows"] > 0) == (V >= 4 * cc.V_FEELS_LEVEL2), V
    for K, c in groups_file[0]["cases"].items():      # ... and moves the medoid
        assert (c["index_one_level"] != c["index"]) == (K >= cc.K_FEELS_LEVEL1), K
        assert (c["index_levels01"] != c["index"]) == (K >= cc.K_FEELS_LEVEL2), K


@pytest.mark.parametrize("V", cc.VIEW_COUNTS)
def test_oracle_view_sums_equal_the_reference(views_file, V):
    meta, z = views_file
    maps, rec, c = cc.views_case(meta, z, V)
    D, op, cp, vis = cc.loss_inputs(V, meta["cases"][V]["loss_seed"])
    loss, idx, hc = oracle.prj_loss(D, op, cp, vis, cc.THR)
    assert eq(loss, c["loss"]) and np.array_equal(idx, c["idx"]) and np.array_equal(hc, c["hc"])
    views = oracle.Views(rec, maps["depth"], maps["ori"], maps["conf"], maps["mask"])
    offs = np.load(os.path.join(GOLDEN, "depth_offsets.npy"))
    _, ori, ml, fhc = oracle.forward(views, c["points"], cc.PATCH, cc.THR, offs, base_idx=c["base_idx"], base_val=c["base_val"])
    assert eq(ml, c["fwd_loss"]) and eq(ori, c["fwd_ori"]) and np.array_equal(fhc, c["fwd_hc"])
    bidx, bval = oracle.topk_views(*[oracle.visible_and_ori(views, c["points"], cc.PATCH)[k] for k in ("visible", "Conf")])
    assert np.array_equal(bval, c["base_val"])
    surf, filt, unv, head = oracle.filter_votes(views, c["vote_points"], cc.PATCH, cc.THR, cc.VIS_THR)
    assert np.array_equal(surf, c["surface_index"]) and np.array_equal(filt, c["filter_index"])
    assert np.array_equal(unv, c["unvisible_index"])
    rl, _ = oracle.refine_loss(views, c["vote_points"], c["dirs"], cc.PATCH, cc.THR)
    rl[head & ~cc.head_top(c["vote_points"].astype(np.float32), cc.toy_head()[1])] = -1
    assert eq(rl, c["refine_loss"])
    assert np.isfinite(c["loss"]).all() and np.isfinite(c["fwd_loss"]).sum() > 8 and (np.isfinite(rl) & (rl != -1)).sum() > 20


@pytest.mark.parametrize("K", cc.GROUP_SIZES)
def test_oracle_member_sums_equal_the_reference(groups_file, K):
    meta, z = groups_file
    g = cc.group(K, meta["cases"][K]["seed"])
    out, idx = oracle.medoid_dense(g[None])
    assert int(idx[0]) == int(z["k%d_index" % K]) == meta["cases"][K]["index"] and np.array_equal(out, z["k%d_out" % K])
    out, idx = oracle.medoid_segmented(g, np.array([0, K], np.int32))
    assert int(idx[0]) == int(z["k%d_index" % K]) and np.array_equal(out, z["k%d_out" % K])


CHILD = r"""
import sys, numpy as np, torch
sys.path[:0] = [%r, %r]
import cascade_cases as cc, oracle
assert torch.backends.cpu.get_cpu_capability() == "AVX2"
torch.set_num_threads(1)
rng = np.random.default_rng(5)
for V in cc.VIEW_COUNTS:
    for shape in ((V, cc.N_SEARCH, cc.S), (V, cc.N_VOTES)):
        x = rng.random(shape, dtype=np.float32)
        want = torch.from_numpy(x).sum(dim=0).numpy()
        assert np.array_equal(cc.outer_sum(x), want), shape
        assert np.array_equal(oracle.outer_sum(x.reshape(V, -1)).reshape(want.shape), want), shape
        if V >= cc.V_FEELS_LEVEL2:
            assert not np.array_equal(cc.outer_sum(x, 2), want), shape
import ctypes
L = oracle.lib()
L.orc_aten_inner_sum.restype = ctypes.c_float
L.orc_aten_inner_sum.argtypes = [ctypes.c_void_p, ctypes.c_int]
for K in cc.GROUP_SIZES:
    x = np.ascontiguousarray(rng.random((1, 6, K), dtype=np.float32))
    want = torch.from_numpy(x).mean(dim=-1).numpy()[0]
    assert np.array_equal(cc.inner_sum(x[0]) / np.float32(K), want), K
    got = np.array([L.orc_aten_inner_sum(x[0, r].ctypes.data_as(ctypes.c_void_p), K) for r in range(6)], np.float32)
    assert np.array_equal(got / np.float32(K), want), K
print("ok")
"""


def test_aten_avx2_sums_equal_the_transcriptions_and_the_oracle():
    """torch.sum(dim=0) / torch.mean(dim=-1) of the fixtures' shapes in a child process that asks ATen for its AVX2 kernels
    (the order the project pins; a host whose default is AVX512 sums 16 floats per vector): equal to the numpy transcriptions
    the generator used and to the oracle's C statements.  Needs a host that offers AVX2."""
    import torch

    if "avx2" not in open("/proc/cpuinfo").read():
        pytest.skip("this host has no AVX2")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, ATEN_CPU_CAPABILITY="avx2")
    r = subprocess.run([sys.executable, "-c", CHILD % (os.path.join(root, "tests"), root)], env=env, capture_output=True,
                       text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stderr[-2000:]
    del torch
