"""GPU: the strand tracer's decisions on their bounds (tests/strand_bound_cases.py): mh_volume_pack, mh_trace_seeds,
mh_trace_scalp and mh_occ_check through the C ABI, the per-seed methods and both drivers of monohair_amd.hairgrow, against
the C oracle, the numpy restatement and what the reference recorded (tests/golden/strand_bounds.npz).  Every comparison
is equality."""
import os

import numpy as np
import pytest
import torch

import oracle
import strand_bound_cases as C
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -12345.5


@pytest.fixture(scope="module")
def setup():
    from monohair_amd.hairgrow import HairGrowing

    z = np.load(os.path.join(GOLDEN, "strand_bounds.npz"))
    c = C.build_cases()
    occ_r, ori_r = C.readers_arrays(c)
    hg = HairGrowing(None, None, device=DEV, occ=occ_r, ori=ori_r)
    vol = oracle.Volume(occ_r[..., 0], ori_r)
    assert (hg.W, hg.H, hg.Z) == C.DIMS
    return z, c, hg, vol


def split(pts, lens):
    o = np.concatenate([[0], np.cumsum(lens)])
    return [pts[o[i]:o[i + 1]] for i in range(len(lens))]


def test_volume_pack_keeps_every_bit(setup):
    """NaN, the denormals 1e-45 and 1e-39, -0.0 and -1 in the occupancy channel come through mh_volume_pack bit for bit"""
    z, c, hg, vol = setup
    got = hg._vox.cpu().numpy()
    want = C.vox_of_cases(c)
    assert np.array_equal(got.view(np.uint32), vol.vox.view(np.uint32))
    assert np.array_equal(got[..., 3].view(np.uint32), want[..., 3].view(np.uint32))
    assert np.array_equal(got, want, equal_nan=True)
    bits = set(got[..., 3].view(np.uint32).ravel().tolist())
    assert {np.array(v, np.float32).view(np.uint32).item() for v in C.OCC_VALUES} <= bits


def _launch_seeds(hg, seeds, thr):
    from monohair_amd import _lib

    n = len(seeds)
    seeds_d = torch.from_numpy(np.ascontiguousarray(seeds)).to(DEV)
    out = torch.full((n + 1, 513, 3), SENT, dtype=torch.float32, device=DEV)
    first = torch.full((n + 1,), -77, dtype=torch.int32, device=DEV)
    ln = torch.full((n + 1,), -77, dtype=torch.int32, device=DEV)
    with torch.cuda.device(hg.device):
        _lib.check(_lib.lib().mh_trace_seeds(hg._ctx, _lib.ptr(hg._vox), hg.W, hg.H, hg.Z, _lib.ptr(seeds_d), n, float(thr),
                                             _lib.ptr(out), _lib.ptr(first), _lib.ptr(ln), _lib.stream_ptr()), "mh_trace_seeds")
    out, first, ln = out.cpu().numpy(), first.cpu().numpy(), ln.cpu().numpy()
    assert first[n] == -77 and ln[n] == -77 and (out[n] == SENT).all()
    return out[:n], first[:n], ln[:n]


def _launch_scalp(hg, pts, nrm, thr):
    from monohair_amd import _lib

    n = len(pts)
    p_d = torch.from_numpy(np.ascontiguousarray(pts)).to(DEV)
    n_d = torch.from_numpy(np.ascontiguousarray(nrm)).to(DEV)
    out = torch.full((n + 1, 257, 3), SENT, dtype=torch.float32, device=DEV)
    ln = torch.full((n + 1,), -77, dtype=torch.int32, device=DEV)
    with torch.cuda.device(hg.device):
        _lib.check(_lib.lib().mh_trace_scalp(hg._ctx, _lib.ptr(hg._vox), hg.W, hg.H, hg.Z, _lib.ptr(p_d), _lib.ptr(n_d), n,
                                             float(thr), _lib.ptr(out), _lib.ptr(ln), _lib.stream_ptr()), "mh_trace_scalp")
    out, ln = out.cpu().numpy(), ln.cpu().numpy()
    assert ln[n] == -77 and (out[n] == SENT).all()
    return out[:n], ln[:n]


@pytest.mark.parametrize("rows", [None, 257, 600])
def test_trace_seeds_equals_oracle_and_record(setup, rows):
    """mh_trace_seeds on the cases of each threshold, alone and tiled to 257 and 600 rows (off the block), into buffers
    filled with a sentinel: first, len and every point equal the oracle and the record; nothing else is written"""
    z, c, hg, vol = setup
    ref = split(z["trace_pts"], z["trace_len"])
    for thr in sorted(set(z["trace_thr"])):
        sel = np.flatnonzero(z["trace_thr"] == thr)
        sel = sel if rows is None else sel[np.arange(rows) % len(sel)]
        seeds = z["trace_seeds"][sel]
        out, first, ln = _launch_seeds(hg, seeds, thr)
        o_out, o_first, o_ln = oracle.trace_seeds(vol, seeds, thr)
        assert np.array_equal(first, o_first) and np.array_equal(ln, o_ln)
        for k, i in enumerate(sel):
            name = c.trace[i]["name"]
            f, l = int(first[k]), int(ln[k])
            assert (out[k, :f] == SENT).all() and (out[k, f + l:] == SENT).all(), name
            assert np.array_equal(out[k, f:f + l], o_out[k, f:f + l]), name
            if z["trace_len"][i] == 0:
                assert l < 5, name
            else:
                assert (f, l) == (z["trace_first"][i], z["trace_len"][i]), name
                assert np.array_equal(out[k, f:f + l], ref[i]), name


@pytest.mark.parametrize("rows", [None, 257, 600])
def test_trace_scalp_equals_oracle_and_record(setup, rows):
    z, c, hg, vol = setup
    ref = split(z["scalp_pts"], z["scalp_len"])
    for thr in sorted(set(z["scalp_thr"])):
        sel = np.flatnonzero(z["scalp_thr"] == thr)
        sel = sel if rows is None else sel[np.arange(rows) % len(sel)]
        pts, nrm = z["scalp_points"][sel], z["scalp_normals"][sel]
        out, ln = _launch_scalp(hg, pts, nrm, thr)
        o_out, o_ln = oracle.trace_scalp(vol, pts, nrm, thr)
        assert np.array_equal(ln, o_ln)
        for k, i in enumerate(sel):
            name = c.scalp[i]["name"]
            assert ln[k] == z["scalp_len"][i], name
            assert np.array_equal(out[k, :ln[k]], ref[i]) and np.array_equal(out[k, :ln[k]], o_out[k, :ln[k]]), name
            # a walk that ends inside the head (len 0) has written the points it took: at most 26
            assert (out[k, (int(ln[k]) if ln[k] > 0 else 26):] == SENT).all(), name


def _is(got, want):
    """a returned strand (not the reference's False or None) equal to the recorded one"""
    return torch.is_tensor(got) and np.array_equal(got.cpu().numpy(), want)


def test_per_seed_methods_equal_the_record(setup, monkeypatch):
    """trace and traceFromScalp, one seed per call as the reference is called; trace's random shift is made zero, as it
    was for the record, and its flag volume holds 0, 2, 2.5, 3 and 4 at the seed voxel of the gate cases"""
    z, c, hg, vol = setup
    W, H, Z = C.DIMS
    monkeypatch.setattr(torch, "rand_like", lambda t, *a, **k: torch.zeros_like(t))
    ref = split(z["trace_pts"], z["trace_len"])
    flag = np.zeros((Z, H, W), np.float32)
    for i, t in enumerate(c.trace):
        seed = torch.from_numpy((t["seed"] - np.float32(0.5)).astype(np.float32))
        got = hg.trace(seed, flag, t["thr"], W, H, Z)
        assert np.array_equal(seed.numpy(), t["seed"]), t["name"]
        if z["trace_len"][i] == 0:
            assert got is False, t["name"]
        else:
            assert _is(got, ref[i]), t["name"]
    for (i, v), want in zip(c.gate, z["gate_len"]):
        t = c.trace[i]
        x, y, zz = C.voxel_of(t["seed"])
        for as_tensor in (False, True):
            flag = np.zeros((Z, H, W), np.float32)
            flag[zz, y, x] = v
            got = hg.trace(torch.from_numpy((t["seed"] - np.float32(0.5)).astype(np.float32)),
                           torch.from_numpy(flag) if as_tensor else flag, t["thr"], W, H, Z)
            assert (got is False) if want == 0 else _is(got, ref[i]), (t["name"], v)
    ref = split(z["scalp_pts"], z["scalp_len"])
    for i, s in enumerate(c.scalp):
        got = hg.traceFromScalp(torch.from_numpy(s["seed"].copy()), torch.from_numpy(s["normal"].copy()), s["thr"], W, H, Z, None)
        if z["scalp_len"][i] == 0:
            assert got is None, s["name"]
        else:
            assert _is(got, ref[i]), s["name"]


def test_drivers_equal_the_record(setup):
    """GenerateGuideStrandFromScalp and randomlyGenerateSegments as a whole: seeds with a trace of five or more points
    refused by flag >= 3, accepted strands with two points in one voxel (the generator asserts both)"""
    z, c, hg, vol = setup
    torch.manual_seed(int(z["driver_seed"]))
    strands, num_root = hg.GenerateGuideStrandFromScalp(torch.from_numpy(z["scalp_points"].copy()),
                                                        torch.from_numpy(z["scalp_normals"].copy()), None, float(z["guide_thr"]))
    assert num_root == int(z["guide_num_root"])
    assert np.array_equal(np.array([s.shape[0] for s in strands]), z["guide_len"])
    assert np.array_equal(torch.cat(strands).cpu().numpy(), z["guide_pts"])
    torch.manual_seed(int(z["driver_seed"]))
    strands = hg.randomlyGenerateSegments(float(z["random_thr"]))
    assert np.array_equal(np.array([s.shape[0] for s in strands]), z["random_len"])
    assert np.array_equal(torch.cat(strands).cpu().numpy(), z["random_pts"])


@pytest.fixture(scope="module")
def occ_setup(setup):
    occ = C.occ_volume()
    S, names = C.occ_strands()
    want = np.array([C.occ_status_np(s, occ) for s in S], np.int32)
    assert set(want.tolist()) == {0, 1, 2, 3}
    return torch.from_numpy(occ).to(DEV), S, names, want


@pytest.mark.parametrize("n", [None, 1, 255, 256, 257, 600])
def test_occ_check_equals_the_restatement(setup, occ_setup, n):
    """mh_occ_check: the ratio exactly 0.8 (4/5, 8/10, 12/15: rejected), 5/6, 9/11, all and none; indices exactly on
    k + 1/2; 256 / 256 / 192 and one below; negative indices (wrapped down to -dim, refused below); batches off the block"""
    z, c, hg, vol = setup
    occ_d, S, names, want = occ_setup
    n = len(S) if n is None else n
    batch = C.tile_strands(S, n)
    pts = torch.from_numpy(np.concatenate(batch, 0)).to(DEV)
    offs = torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in batch])]).astype(np.int64)).to(DEV)
    with torch.cuda.device(hg.device):
        status = hg._occ_status(pts, offs, n, occ_d).cpu().numpy()
    exp = want[np.arange(n) % len(S)]
    bad = np.flatnonzero(status != exp)
    assert len(bad) == 0, [(names[i % len(S)], int(status[i]), int(exp[i])) for i in bad[:8]]
