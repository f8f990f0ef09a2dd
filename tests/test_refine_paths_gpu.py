"""The exits of refine() that no other test reaches -- fewer kept points than neighbours, no kept point, no shell point -- in
three forms of the driver (the device-resident pass, MH_REFINE_DEVICE=0, MH_REFINE_CHAIN=0), on the smallest scene with two
chunks: tests/golden/e2e_headfilter.npz (24 views of 240 x 136, patch 3; 6000 points = one full chunk and one of 1000, a third
of them head-filtered, 40 NaN input rows; 500 shell points), built as tests/golden_drivers.py builds it.  The smoothed arrays
do not depend on the threshold, so the reference's own files are the bar for them in every case."""
import os

import numpy as np
import pytest
import scipy.io

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FORMS = {"default": {}, "host_driven": {"MH_REFINE_DEVICE": "0"}, "four_launches": {"MH_REFINE_CHAIN": "0"}}
FILES = ["Occ3D.mat", "Ori3D.mat", "filter_unvisible.npy", "filter_unvisible_ori.npy", "min_loss.npy", "select_o.npy",
         "select_p.npy"]


@pytest.fixture(scope="module")
def scene():
    import golden_drivers

    z, meta, pm = golden_drivers.golden_pmvo("cuda:0")
    h = np.load(os.path.join(GOLDEN, "e2e_headfilter.npz"), allow_pickle=False)
    assert h["in_points"].shape == (6000, 3) and h["in_shell"].shape == (500, 3) and len(h["nan_rows"]) == 40
    return {"meta": meta, "pm": pm, "h": h}


def run_forms(scene, tmp_path, monkeypatch, threshold, shell):
    """refine() in the three forms -> {form: last_refine}; the files are under tmp_path/<form>/refine."""
    import golden_drivers
    from monohair_amd.pmvo import refine

    h, info = scene["h"], {}
    for form, env in FORMS.items():
        for k in ("MH_REFINE_DEVICE", "MH_REFINE_CHAIN"):
            monkeypatch.delenv(k, raising=False)
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        args = golden_drivers.driver_args(str(tmp_path / form), scene["meta"])
        refine(h["in_points"].copy(), h["in_ori"].copy(), h["in_loss"].copy(), scene["pm"], shell.copy(), args,
               infer_inner=False, threshold=threshold, genrate_ori_only=False, return_dense=False)
        info[form] = dict(scene["pm"].last_refine)
    return info


def check_common(scene, tmp_path):
    """What holds in every case: the reference's smoothed arrays, shell rows in their order, the same bytes in every form."""
    h = scene["h"]
    shell32 = h["in_shell"].astype(np.float32)
    for form in FORMS:
        d = tmp_path / form / "refine"
        assert sorted(os.listdir(d)) == FILES, form
        assert np.array_equal(np.load(d / "select_o.npy"), h["ref_select_o"], equal_nan=True), form
        assert np.array_equal(np.load(d / "min_loss.npy"), h["ref_min_loss"], equal_nan=True), form
        kept = np.load(d / "filter_unvisible.npy")
        assert kept.dtype == np.float32 and kept.ndim == 2 and kept.shape[1] == 3
        assert np.load(d / "filter_unvisible_ori.npy").shape == kept.shape
        at = 0
        for row in kept:                                  # rows of the shell array, in their original order
            while at < len(shell32) and shell32[at].tobytes() != row.tobytes():
                at += 1
            assert at < len(shell32), form
            at += 1
    for n in FILES:
        blobs = [open(tmp_path / form / "refine" / n, "rb").read() for form in FORMS]
        if n.endswith(".mat"):                            # (the header carries a creation time: compare the payloads)
            blobs = [b[128:] for b in blobs]
        assert blobs[0] == blobs[1] == blobs[2], n


def test_fewer_kept_points_than_neighbours(scene, tmp_path, monkeypatch):
    """A threshold that keeps 50 points: the reference then asks its tree for 50 neighbours, and the device-resident pass
    hands its shell stage to the host-driven one."""
    ref = scene["h"]["ref_min_loss"]
    s = np.sort(ref[~np.isnan(ref)])
    threshold = float(s[50])
    assert int((ref < threshold).sum()) == 50             # (strict <: s[49] < s[50] in the golden)
    info = run_forms(scene, tmp_path, monkeypatch, threshold, scene["h"]["in_shell"])
    assert info["default"] == {"device_pass": True, "prefetch_adopted": False,
                               "shell_stage": "host (fewer kept points than neighbours)"}, info
    assert not info["host_driven"]["device_pass"] and not info["four_launches"]["device_pass"]
    check_common(scene, tmp_path)


def test_no_point_kept(scene, tmp_path, monkeypatch):
    """Threshold -1: below the golden's smallest loss (-1.19e-07).  No shell stage, an empty volume."""
    assert np.nanmin(scene["h"]["ref_min_loss"]) > -1.0
    info = run_forms(scene, tmp_path, monkeypatch, -1.0, scene["h"]["in_shell"])
    assert info["default"]["device_pass"], info
    check_common(scene, tmp_path)
    for form in FORMS:
        for n in ("filter_unvisible.npy", "filter_unvisible_ori.npy"):
            a = np.load(tmp_path / form / "refine" / n)
            assert a.shape == (0, 3) and a.dtype == np.float32, (form, n)
        occ = scipy.io.loadmat(tmp_path / form / "refine" / "Occ3D.mat")["Occ"]
        assert (occ.nnz if hasattr(occ, "nnz") else np.count_nonzero(occ)) == 0, form


def test_no_shell_points(scene, tmp_path, monkeypatch):
    """An empty shell array at the golden's threshold: the device-resident pass goes through without a shell stage."""
    shell = np.zeros((0, 3), scene["h"]["in_shell"].dtype)
    info = run_forms(scene, tmp_path, monkeypatch, scene["meta"]["threshold"], shell)
    assert info["default"] == {"device_pass": True, "prefetch_adopted": False, "shell_stage": "device"}, info
    check_common(scene, tmp_path)
    for form in FORMS:
        assert np.load(tmp_path / form / "refine" / "filter_unvisible.npy").shape == (0, 3)
