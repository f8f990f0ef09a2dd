"""GPU: the synthetic hair capture through the pipeline WITHOUT its ground-truth geometry -- `synth_hair.write_case`, then
`ours/colmap_points.obj` and `render_depth/` moved aside and made again by `python -m monohair_amd.haircarve` from the hair
masks, the cameras and the bust, then `PMVO.py`, `HairGrow.py` and `python -m monohair_amd.hairmetrics` -- at the size of
tests/test_hair_capture_e2e_gpu.py: 24 views of 240 x 136, 500 strands, patch 3, seed 3, carve voxel 0.0025.

Asserted: every file is written, connected_strands.hair is finite and valid, select_p has rows, and the optimised line
directions agree with the ground-truth strands more often on the carved case than on the same case with every orientation code
turned by 90 degrees (the control of docs/PARITY.md f6).
Recorded, no bound asserted (docs/PARITY.md f11 holds the figures of an MI355X run): carved depth minus ground-truth depth over
the pixels that are hair in both, the size of the hull, the share of select_p rows and the three F-scores next to those of the
ground-truth geometry (f6: 0.9893 and 0.0074 / 0.0767 / 0.2212)."""
import json
import os
import shutil

import numpy as np
import pytest

from conftest import ROOT
from test_hair_capture_e2e_gpu import H, POINTS, STRANDS, V, W, _common, _run, _share

pytestmark = pytest.mark.gpu

CARVE_VS = 0.0025
F6 = dict(share=0.9893, f_score=(0.0074, 0.0767, 0.2212))


@pytest.fixture(scope="module")
def carved_run(tmp_path_factory):
    from monohair_amd import synth_hair

    data = str(tmp_path_factory.mktemp("carve") / "data")
    base = synth_hair.write_case(data, "synthetic_hair", V=V, H=H, W=W, seed=0, n_strands=STRANDS, n_points=POINTS)
    aside = os.path.join(data, "ground_truth")
    os.makedirs(aside)
    shutil.move(os.path.join(base, "ours", "colmap_points.obj"), os.path.join(aside, "colmap_points.obj"))
    shutil.move(os.path.join(base, "render_depth"), os.path.join(aside, "render_depth"))
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = _run(["-m", "monohair_amd.haircarve"] + _common(data) + ["--name=t", "--voxel-size", str(CARVE_VS)], env)
    print(r.stdout[-400:])
    assert os.path.exists(os.path.join(base, "ours", "colmap_points.obj"))
    assert len(os.listdir(os.path.join(base, "render_depth"))) == V
    _run([os.path.join(ROOT, "PMVO.py")] + _common(data) + ["--name=t"], env)
    return data, base, aside, env


def test_carved_depth_against_the_ground_truth_depth(carved_run):
    """recorded: how far the hull's depth lies from the strands' over the pixels that are hair in both"""
    from PIL import Image
    from monohair_amd.pmvo_utils import read_obj

    data, base, aside, env = carved_run
    diff = []
    for f in sorted(os.listdir(os.path.join(aside, "render_depth"))):
        gt = np.load(os.path.join(aside, "render_depth", f))[..., 0]
        got = np.load(os.path.join(base, "render_depth", f))
        assert got.dtype == np.float32 and got.shape == (H, W, 3) and np.isfinite(got).all()
        hair = np.array(Image.open(os.path.join(base, "hair_mask", f[:-4] + ".png")))[..., 0] >= 52
        both = hair & (gt < 255.0) & (got[..., 0] < 255.0)
        diff.append((got[..., 0][both].astype(np.float64) - gt[both]) / 255.0 * 2.0 * 1000.0)
    diff = np.concatenate(diff)
    v, t = read_obj(os.path.join(base, "ours", "colmap_points.obj"))
    assert len(diff) > 0 and len(t) > 0 and t.max() < len(v)
    print("carved depth minus ground-truth depth over %d hair pixels, mm: median %.3f, 10th %.3f, 90th %.3f; within 0.8 mm: %.4f"
          % (len(diff), np.median(diff), np.percentile(diff, 10), np.percentile(diff, 90), float((np.abs(diff) <= 0.8).mean())))
    print("hull: %d vertices, %d triangles" % (len(v), len(t)))


def test_carved_case_beats_the_control_turned_by_90_degrees(carved_run, tmp_path):
    from PIL import Image

    data, base, aside, env = carved_run
    control = str(tmp_path / "data")
    shutil.copytree(base, os.path.join(control, "synthetic_hair"), ignore=shutil.ignore_patterns("output"))
    ori_dir = os.path.join(control, "synthetic_hair", "best_ori")
    for f in sorted(os.listdir(ori_dir)):
        k = np.array(Image.open(os.path.join(ori_dir, f)))
        assert k.dtype == np.uint8 and k.shape == (H, W) and k.max() < 180
        Image.fromarray(((k.astype(np.int64) + 90) % 180).astype(np.uint8)).save(os.path.join(ori_dir, f))
    _run([os.path.join(ROOT, "PMVO.py")] + _common(control) + ["--name=t"], env)
    share, n = _share(data, "t")
    control_share, n_control = _share(control, "t")
    print("share of select_p rows that agree with the ground truth: carved case %.4f of %d, control %.4f of %d; "
          "ground-truth geometry (PARITY f6) %.4f" % (share, n, control_share, n_control, F6["share"]))
    assert n > 0 and n_control > 0
    assert share > control_share


def test_strands_grown_on_the_carved_case_are_valid_and_scored(carved_run):
    from monohair_amd.pmvo_utils import load_strand

    data, base, aside, env = carved_run
    _run([os.path.join(ROOT, "HairGrow.py")] + _common(data) + ["--name=t", "--HairGenerate.num_scalp_samples=2000"], env)
    out = os.path.join(base, "output", "t_seed3", "refine")
    for f in ("select_p.npy", "select_o.npy", "Occ3D.mat", "Ori3D.mat", "connected_strands.hair"):
        assert os.path.exists(os.path.join(out, f)), f
    assert len(np.load(os.path.join(out, "select_p.npy"))) > 0
    segments, points = load_strand(os.path.join(out, "connected_strands.hair"))
    segments = np.asarray(segments)
    assert len(segments) > 0 and (segments >= 1).all() and int(segments.sum()) == len(points) and np.isfinite(points).all()
    report = os.path.join(out, "scores.json")
    _run(["-m", "monohair_amd.hairmetrics", os.path.join(out, "connected_strands.hair"), os.path.join(base, "gt_strands.hair"),
          "--json", report], env)
    res = json.load(open(report))
    print("carved case: f-scores", res["f_score"], "precision", res["precision"], "recall", res["recall"],
          "; ground-truth geometry (PARITY f6)", F6["f_score"])
    assert res["counts"]["pred"]["valid"] > 0 and res["counts"]["gt"]["valid"] > 0
