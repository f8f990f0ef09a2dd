"""GPU: the ground-truth volume of the synthetic hair capture beside the volumes the pipeline fits, at the size of
tests/test_hair_capture_e2e_gpu.py (24 views of 240 x 136, 500 strands, patch 3, --seed=3) and through the commands a user runs.

(a) scores the fitted volume of the true capture, and that of the control whose orientation codes are all turned by 90
    degrees, against the volume `hairvolume voxelize` makes of gt_strands.hair: F at reach 1 / 30 degrees must be higher for the
    true capture.  The volume-level figures are printed, their size is not asserted.
(b) runs the strand stage on the ground-truth volume (`HairGrow.py --name=gt`) and scores connected_strands.hair against
    gt_strands.hair: what the strand stage makes of a perfect volume.  No bound is asserted: that the ideal volume grows better
    strands than the fitted one is the hypothesis this measurement exists to test."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

V, H, W, STRANDS, POINTS = 24, 240, 136, 500, 64


def _run(argv, env):
    r = subprocess.run([sys.executable] + argv, cwd=ROOT, env=env, stdin=subprocess.DEVNULL, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _common(data):
    return ["--yaml=configs/reconstruct/synthetic_hair", "--data.root=%s" % data, "--data.image_size=[%d,%d]" % (H, W),
            "--PMVO.patch_size=3", "--seed=3"]


def _refine(data, name):
    return os.path.join(data, "synthetic_hair", "output", name + "_seed3", "refine")


@pytest.fixture(scope="module")
def true_run(tmp_path_factory):
    from monohair_amd import synth_hair

    data = str(tmp_path_factory.mktemp("hairvol") / "data")
    synth_hair.write_case(data, "synthetic_hair", V=V, H=H, W=W, seed=0, n_strands=STRANDS, n_points=POINTS)
    env = dict(os.environ, PYTHONPATH=ROOT)
    _run([os.path.join(ROOT, "PMVO.py")] + _common(data) + ["--name=t"], env)
    r = _run(["-m", "monohair_amd.hairvolume", "voxelize", os.path.join(data, "synthetic_hair", "gt_strands.hair"), "--out",
              _refine(data, "gt")], env)
    print(r.stdout)
    return data, env


def test_fitted_volume_of_the_true_capture_beats_the_control(true_run, tmp_path):
    from PIL import Image

    from monohair_amd import hairvolume

    data, env = true_run
    control = str(tmp_path / "data")
    shutil.copytree(os.path.join(data, "synthetic_hair"), os.path.join(control, "synthetic_hair"),
                    ignore=shutil.ignore_patterns("output"))
    ori_dir = os.path.join(control, "synthetic_hair", "best_ori")
    for f in sorted(os.listdir(ori_dir)):
        k = np.array(Image.open(os.path.join(ori_dir, f)))
        assert k.dtype == np.uint8 and k.shape == (H, W) and k.max() < 180
        Image.fromarray(((k.astype(np.int64) + 90) % 180).astype(np.uint8)).save(os.path.join(ori_dir, f))
    _run([os.path.join(ROOT, "PMVO.py")] + _common(control) + ["--name=t"], env)
    gt = hairvolume.load_volume(_refine(data, "gt"))
    res = {}
    for name, root in (("true capture", data), ("control", control)):
        res[name] = hairvolume.score_volumes(hairvolume.load_volume(_refine(root, "t")), gt)
        print("%s: %d fitted voxels against %d ground-truth voxels" % (name, res[name]["counts"]["pred"]["voxels"],
                                                                       res[name]["counts"]["gt"]["voxels"]))
        for line in hairvolume.format_scores(res[name]):
            print("  " + line)
    k = [list(t) for t in hairvolume.DEFAULT_THRESHOLDS].index([1, 30.0])
    for r in res.values():
        assert r["counts"]["pred"]["voxels"] > 0 and r["counts"]["gt"]["voxels"] > 0
    assert res["true capture"]["f_score"][k] > res["control"]["f_score"][k]


def test_strands_grown_on_the_ground_truth_volume_are_scored(true_run):
    from monohair_amd.pmvo_utils import load_strand

    data, env = true_run
    _run([os.path.join(ROOT, "HairGrow.py")] + _common(data) + ["--name=gt", "--HairGenerate.num_scalp_samples=2000"], env)
    out = _refine(data, "gt")
    pred = os.path.join(out, "connected_strands.hair")
    assert os.path.exists(pred)
    segments, points = load_strand(pred)
    assert len(segments) > 0 and points.shape == (int(sum(segments)), 3) and np.isfinite(points).all()
    report = os.path.join(out, "scores.json")
    r = _run(["-m", "monohair_amd.hairmetrics", pred, os.path.join(data, "synthetic_hair", "gt_strands.hair"), "--json",
              report], env)
    print(r.stdout)
    res = json.load(open(report))
    print("strands grown on the ground-truth volume: f-scores", res["f_score"], "precision", res["precision"], "recall",
          res["recall"])
    assert res["counts"]["pred"]["valid"] > 0 and res["counts"]["gt"]["valid"] > 0
