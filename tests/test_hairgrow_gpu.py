"""GPU: strand tracing (csrc/hairgrow.hip + monohair_amd.hairgrow) against the CPU oracle and the reference's own
HairGrowing run (tests/golden/hairgrow.npz)."""
import os

import numpy as np
import pytest
import torch

import oracle
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.fixture(scope="module")
def setup():
    from monohair_amd.hairgrow import HairGrowing

    z = np.load(os.path.join(GOLDEN, "hairgrow.npz"))
    occ = z["occ"].transpose(2, 1, 0)[..., None]           # [Z,Y,X,1] as get_ground_truth_3D_occ returns
    ori = z["ori"].transpose(2, 1, 0, 3)                    # [Z,Y,X,3]
    hg = HairGrowing(None, None, device=DEV, occ=occ, ori=ori)
    vol = oracle.Volume(occ[..., 0], ori)
    return z, hg, vol


def test_kernels_match_oracle_exactly(setup):
    z, hg, vol = setup
    assert np.array_equal(hg._vox.cpu().numpy(), vol.vox)
    rng = np.random.default_rng(0)
    seeds = (np.argwhere(vol.vox[..., 3] != 0)[:, ::-1] + rng.random((int((vol.vox[..., 3] != 0).sum()), 3))).astype(
        np.float32)
    out, first, ln = hg._trace_seeds(torch.from_numpy(seeds).to(DEV), 0.8)
    o_out, o_first, o_ln = oracle.trace_seeds(vol, seeds, 0.8)
    assert np.array_equal(first.cpu().numpy(), o_first) and np.array_equal(ln.cpu().numpy(), o_ln)
    out = out.cpu().numpy()
    for i in range(len(seeds)):
        assert np.array_equal(out[i, o_first[i]:o_first[i] + o_ln[i]], o_out[i, o_first[i]:o_first[i] + o_ln[i]])
    sp, sl = hg._trace_scalp(torch.from_numpy(z["scalp_points"]).to(DEV), torch.from_numpy(z["scalp_normals"]).to(DEV),
                             0.8)
    o_sp, o_sl = oracle.trace_scalp(vol, z["scalp_points"], z["scalp_normals"], 0.8)
    assert np.array_equal(sl.cpu().numpy(), o_sl)
    sp = sp.cpu().numpy()
    for i in range(len(o_sl)):
        assert np.array_equal(sp[i, :o_sl[i]], o_sp[i, :o_sl[i]])


def test_guide_strands_match_reference(setup):
    z, hg, vol = setup
    torch.manual_seed(77)
    strands, num_root = hg.GenerateGuideStrandFromScalp(torch.from_numpy(z["scalp_points"].copy()),
                                                        torch.from_numpy(z["scalp_normals"].copy()), None, 0.8)
    assert num_root == int(z["guide_num_root"])
    assert np.array_equal(np.array([s.shape[0] for s in strands]), z["guide_len"])
    assert np.array_equal(torch.cat(strands).cpu().numpy(), z["guide_pts"])


def test_random_segments_match_reference_and_hair_file(setup, tmp_path):
    from monohair_amd.pmvo_utils import load_strand, save_hair_strands

    z, hg, vol = setup
    torch.manual_seed(77)
    strands = hg.randomlyGenerateSegments(0.8)
    assert np.array_equal(np.array([s.shape[0] for s in strands]), z["random_len"])
    assert np.array_equal(torch.cat(strands).cpu().numpy(), z["random_pts"])
    world = hg.VoxelToWorld(strands, np.zeros(3, np.float32))
    p = str(tmp_path / "seg.hair")
    save_hair_strands(p, world, np.zeros(3), translate=False)
    seg, pts = load_strand(p)
    assert seg == [int(x) for x in z["random_len"]]
    assert np.allclose(pts, np.concatenate(world))


def test_per_seed_methods_equal_the_batched_drivers(setup):
    """trace / traceFromScalp (one seed per call, the reference's signatures) give the strands of the batched kernels"""
    z, hg, vol = setup
    W, H, Z = hg.W, hg.H, hg.Z
    sp, sn = torch.from_numpy(z["scalp_points"]), torch.from_numpy(z["scalp_normals"])
    o_sp, o_sl = oracle.trace_scalp(vol, z["scalp_points"], z["scalp_normals"], 0.8)
    for i in range(0, len(sp), max(1, len(sp) // 25)):
        s = hg.traceFromScalp(sp[i].clone(), sn[i].clone(), 0.8, W, H, Z, None)
        if o_sl[i] <= 0:
            assert s is None
        else:
            assert np.array_equal(s.cpu().numpy(), o_sp[i, :o_sl[i]])
    nz = np.argwhere(vol.vox[..., 3] != 0)[:, ::-1].astype(np.float32)
    flag = np.zeros((Z, H, W), np.float32)
    torch.manual_seed(5)
    jit = torch.rand(len(nz[:40]), 3)
    torch.manual_seed(5)
    for i in range(40):
        seed = torch.from_numpy(nz[i].copy())
        want_seed = (nz[i] + 0.5 + jit[i].numpy() * 0.5).astype(np.float32)
        got = hg.trace(seed, flag, 0.8, W, H, Z)
        assert np.array_equal(seed.numpy(), want_seed)              # shifted in place, like the reference
        o_out, o_first, o_ln = oracle.trace_seeds(vol, want_seed[None], 0.8)
        if o_ln[0] >= 5:
            assert np.array_equal(got.cpu().numpy(), o_out[0, o_first[0]:o_first[0] + o_ln[0]])
        else:
            assert got is False
    flag[:] = 3
    assert hg.trace(torch.from_numpy(nz[0].copy()), flag, 0.8, W, H, Z) is False


# ---------------------------------------------------------------- long strands, volume borders, W != H != Z
@pytest.fixture(scope="module")
def long_setup():
    """tests/golden/strands_long.npz (tools/gen_golden_strands_long.py): walks that reach both 256-step caps, leave
    through every face and go on over the clamped border voxels, on a 64 x 24 x 56 volume"""
    from monohair_amd.hairgrow import HairGrowing

    z = np.load(os.path.join(GOLDEN, "strands_long.npz"))
    G = tuple(int(g) for g in z["trace_shape"])
    occ = np.zeros(G, np.float32)
    occ[tuple(z["trace_occ_nz"].T.astype(np.int64))] = 1
    ori = np.zeros(G + (3,), np.float32)
    ori[tuple(z["trace_ori_nz"].T.astype(np.int64))] = z["trace_ori_nz_val"]
    occ = occ.transpose(2, 1, 0)[..., None]
    ori = ori.transpose(2, 1, 0, 3)
    hg = HairGrowing(None, None, device=DEV, occ=occ, ori=ori)
    vol = oracle.Volume(occ[..., 0], ori)
    assert len({hg.W, hg.H, hg.Z}) == 3
    return z, hg, vol


def _split(pts, lens):
    o = np.concatenate([[0], np.cumsum(lens)])
    return [pts[o[i]:o[i + 1]] for i in range(len(lens))]


def test_long_volume_pack_matches_oracle(long_setup):
    z, hg, vol = long_setup
    assert np.array_equal(hg._vox.cpu().numpy(), vol.vox)


@pytest.mark.parametrize("count", [None, 1])
def test_long_walks_match_oracle_and_reference(long_setup, count):
    """_trace_seeds / _trace_scalp == the oracle == the reference's recorded walks: first, len and every point, with a
    seed count that is not a multiple of the block size and with one seed (a 513-point strand)"""
    z, hg, vol = long_setup
    thr = float(z["grow_thr"])
    sel = np.arange(len(z["trace_seeds"])) if count is None else np.flatnonzero(z["trace_len"] == 513)[:1]
    assert len(sel) % 256 != 0
    seeds = np.ascontiguousarray(z["trace_seeds"][sel])
    out, first, ln = hg._trace_seeds(torch.from_numpy(seeds).to(DEV), thr)
    out, first, ln = out.cpu().numpy(), first.cpu().numpy(), ln.cpu().numpy()
    o_out, o_first, o_ln = oracle.trace_seeds(vol, seeds, thr)
    assert np.array_equal(first, o_first) and np.array_equal(ln, o_ln)
    ref = _split(z["trace_pts"], z["trace_len"])
    for k, i in enumerate(sel):
        assert np.array_equal(out[k, first[k]:first[k] + ln[k]], o_out[k, first[k]:first[k] + ln[k]]), i
        if z["trace_len"][i] == 0:
            assert ln[k] < 5
        else:
            assert ln[k] == z["trace_len"][i] and first[k] == z["trace_first"][i], i
            assert np.array_equal(out[k, first[k]:first[k] + ln[k]], ref[i]), i
    ssel = np.arange(len(z["scalp_len"])) if count is None else np.flatnonzero(z["scalp_len"] == 257)[:1]
    sp, sl = hg._trace_scalp(torch.from_numpy(np.ascontiguousarray(z["scalp_points"][ssel])).to(DEV),
                             torch.from_numpy(np.ascontiguousarray(z["scalp_normals"][ssel])).to(DEV), thr)
    sp, sl = sp.cpu().numpy(), sl.cpu().numpy()
    assert np.array_equal(sl, z["scalp_len"][ssel])
    ref = _split(z["scalp_pts"], z["scalp_len"])
    for k, i in enumerate(ssel):
        assert np.array_equal(sp[k, :sl[k]], ref[i]), i


def test_long_untouched_slots(long_setup):
    """The kernels write row i of their output only in [first, first+len) and nothing past row n-1: the buffers, one
    guard row longer than n, are filled with a sentinel before the launch through the C ABI.  A walk at both caps
    writes slots 0 and 512 of its row and leaves slot 0 of the next row alone."""
    from monohair_amd import _lib

    z, hg, vol = long_setup
    thr = float(z["grow_thr"])
    SENT = -12345.5
    seeds = torch.from_numpy(np.ascontiguousarray(z["trace_seeds"])).to(DEV)
    n = seeds.shape[0]
    out = torch.full((n + 1, 513, 3), SENT, dtype=torch.float32, device=DEV)
    first = torch.full((n + 1,), -77, dtype=torch.int32, device=DEV)
    ln = torch.full((n + 1,), -77, dtype=torch.int32, device=DEV)
    with torch.cuda.device(hg.device):
        _lib.check(_lib.lib().mh_trace_seeds(hg._ctx, _lib.ptr(hg._vox), hg.W, hg.H, hg.Z, _lib.ptr(seeds), n, thr,
                                             _lib.ptr(out), _lib.ptr(first), _lib.ptr(ln), _lib.stream_ptr()),
                   "mh_trace_seeds")
    out, first, ln = out.cpu().numpy(), first.cpu().numpy(), ln.cpu().numpy()
    assert first[n] == -77 and ln[n] == -77 and (out[n] == SENT).all()
    o_out, o_first, o_ln = oracle.trace_seeds(vol, z["trace_seeds"], thr)
    assert np.array_equal(first[:n], o_first) and np.array_equal(ln[:n], o_ln)
    assert (ln[:n] == 513).any()
    for i in range(n):
        f, l = int(first[i]), int(ln[i])
        assert (out[i, :f] == SENT).all() and (out[i, f + l:] == SENT).all(), i
        assert np.array_equal(out[i, f:f + l], o_out[i, f:f + l]), i
        if l == 513:
            assert f == 0 and (out[i, 0] != SENT).all() and (out[i, 512] != SENT).all()
    sp = torch.from_numpy(np.ascontiguousarray(z["scalp_points"])).to(DEV)
    sn = torch.from_numpy(np.ascontiguousarray(z["scalp_normals"])).to(DEV)
    m = sp.shape[0]
    out = torch.full((m + 1, 257, 3), SENT, dtype=torch.float32, device=DEV)
    ln = torch.full((m + 1,), -77, dtype=torch.int32, device=DEV)
    with torch.cuda.device(hg.device):
        _lib.check(_lib.lib().mh_trace_scalp(hg._ctx, _lib.ptr(hg._vox), hg.W, hg.H, hg.Z, _lib.ptr(sp), _lib.ptr(sn), m,
                                             thr, _lib.ptr(out), _lib.ptr(ln), _lib.stream_ptr()), "mh_trace_scalp")
    out, ln = out.cpu().numpy(), ln.cpu().numpy()
    assert ln[m] == -77 and (out[m] == SENT).all()
    o_sp, o_sl = oracle.trace_scalp(vol, z["scalp_points"], z["scalp_normals"], thr)
    assert np.array_equal(ln[:m], o_sl) and (o_sl == 257).any() and (o_sl == 0).any()
    for i in range(m):
        # a walk that ends inside the head (len 0, the reference's None) has written the points it took: at most 26
        w = int(o_sl[i]) if o_sl[i] > 0 else 26
        assert (out[i, w:] == SENT).all(), i
        assert np.array_equal(out[i, :o_sl[i]], o_sp[i, :o_sl[i]]), i


def test_strands_compact_rows(long_setup):
    """mh_strands_compact on rows of 0, 1, 257 and 513 points, with and without `first`, equals the numpy concatenation
    and writes nothing past the packed points"""
    from monohair_amd import _lib

    z, hg, vol = long_setup
    rng = np.random.default_rng(3)
    for stride, use_first in ((513, True), (257, False)):
        lens = np.array([0, 1, 257, stride, 0, 5, 1, stride, 64, 65, 0], np.int32)
        first = np.array([rng.integers(0, stride - l + 1) if use_first else 0 for l in lens], np.int32)
        rows = rng.random((len(lens), stride, 3)).astype(np.float32)
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)
        total = int(lens.sum())
        packed = torch.full((total + 7, 3), -5.0, dtype=torch.float32, device=DEV)
        d = lambda a: torch.from_numpy(a).to(DEV)      # noqa: E731
        rows_d, first_d, lens_d, offs_d = d(rows), d(first), d(lens), d(offs)
        with torch.cuda.device(hg.device):
            _lib.check(_lib.lib().mh_strands_compact(hg._ctx, _lib.ptr(rows_d), _lib.ptr(first_d) if use_first else None,
                                                     _lib.ptr(lens_d), _lib.ptr(offs_d), len(lens), stride,
                                                     _lib.ptr(packed), _lib.stream_ptr()), "mh_strands_compact")
        want = np.concatenate([rows[i, first[i]:first[i] + lens[i]] for i in range(len(lens))], 0)
        got = packed.cpu().numpy()
        assert np.array_equal(got[:total], want) and (got[total:] == -5.0).all()


def test_long_drivers_match_reference(long_setup):
    z, hg, vol = long_setup
    thr = float(z["grow_thr"])
    torch.manual_seed(77)
    strands, num_root = hg.GenerateGuideStrandFromScalp(torch.from_numpy(z["scalp_points"].copy()),
                                                        torch.from_numpy(z["scalp_normals"].copy()), None, thr)
    assert num_root == int(z["guide_num_root"])
    assert np.array_equal(np.array([s.shape[0] for s in strands]), z["guide_len"])
    assert np.array_equal(torch.cat(strands).cpu().numpy(), z["guide_pts"])
    torch.manual_seed(77)
    strands = hg.randomlyGenerateSegments(thr)
    assert np.array_equal(np.array([s.shape[0] for s in strands]), z["random_len"])
    assert np.array_equal(torch.cat(strands).cpu().numpy(), z["random_pts"])
    assert z["guide_len"].max() == 513 and z["random_len"].max() == 513


def test_long_per_seed_methods_match_reference(long_setup):
    """trace / traceFromScalp, one seed per call as the reference is called, seeds outside the volume included"""
    z, hg, vol = long_setup
    thr = float(z["grow_thr"])
    W, H, Z = hg.W, hg.H, hg.Z
    dims = np.array([W, H, Z])
    ref = _split(z["scalp_pts"], z["scalp_len"])
    outside = 0
    for i in range(len(ref)):
        s = hg.traceFromScalp(torch.from_numpy(z["scalp_points"][i].copy()), torch.from_numpy(z["scalp_normals"][i].copy()),
                              thr, W, H, Z, None)
        if z["scalp_len"][i] == 0:
            assert s is None, i
        else:
            assert np.array_equal(s.cpu().numpy(), ref[i]), i
            outside += bool(((z["scalp_points"][i] < 0) | (z["scalp_points"][i] >= dims)).any())
    ref = _split(z["trace_pts"], z["trace_len"])
    flag = np.zeros((Z, H, W), np.float32)
    torch.manual_seed(31)
    for i in range(len(ref)):
        seed = torch.from_numpy(z["trace_seeds_in"][i].copy())
        got = hg.trace(seed, flag, thr, W, H, Z)
        assert np.array_equal(seed.numpy(), z["trace_seeds"][i]), i        # shifted in place, the reference's draws
        if z["trace_len"][i] == 0:
            assert got is False, i
        else:
            assert np.array_equal(got.cpu().numpy(), ref[i]), i
            outside += bool(((z["trace_seeds"][i] < 0) | (z["trace_seeds"][i] >= dims)).any())
    assert outside >= 4
