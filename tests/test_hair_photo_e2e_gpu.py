"""GPU: the synthetic capture from PHOTOGRAPHS -- `synth_hair.photo_planes`, the Gabor stage, `PMVO.py`, `HairGrow.py`,
`python -m monohair_amd.hairmetrics` -- at 24 views of 240 x 136 and 500 strands, seed 0, the renderer's defaults.

E1 asks whether the Gabor stage finds the drawn strand directions: on the confident hair pixels of the geometric capture that
    also pass the Gabor confidence cut of configs/reconstruct/synthetic_hair.yaml, the share of Gabor codes within 15 degrees
    of the geometric code must beat the same share against the codes turned by 90 degrees and the chance level 1/6, and the
    cut must keep at least a quarter of those pixels.
    Measured on an MI355X: share 0.5944, turned 0.0254, |P| = 298 552 of |C| = 299 931 (0.9954), median error 11 degrees
    (docs/PARITY.md f7).
E2 runs the pipeline on write_case(photo=True) -- best_ori/ and conf/ are what gabor.batch_generate made of the photographs --
    against a control whose orientation codes are all turned by 90 degrees, then the strand stage and the scores.
    Measured: share 0.9824 of 33 158 select_p rows on the photographed capture (the geometric capture: 0.9893), 0.0020 of
    33 158 on the control; F-scores 0.0071 / 0.0709 / 0.2071 at 1 mm / 10, 2 mm / 20 and 3 mm / 30 degrees (geometric: 0.0074 /
    0.0767 / 0.2212).  They are recorded in docs/PARITY.md f7; no bound is asserted on them."""
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
DEV = "cuda:0"


def _run(argv, env):
    r = subprocess.run([sys.executable] + argv, cwd=ROOT, env=env, stdin=subprocess.DEVNULL, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def _common(data):
    return ["--yaml=configs/reconstruct/synthetic_hair", "--data.root=%s" % data, "--data.image_size=[%d,%d]" % (H, W),
            "--PMVO.patch_size=3", "--seed=3"]


def _share(data, name):
    """the share of refine/select_p rows within 5 mm of a ground-truth sample whose tangent is within 30 degrees of select_o"""
    from monohair_amd import hairmetrics as hm
    from monohair_amd.pmvo_utils import load_strand

    out = os.path.join(data, "synthetic_hair", "output", name + "_seed3", "refine")
    p = np.load(os.path.join(out, "select_p.npy")).astype(np.float32)
    o = np.load(os.path.join(out, "select_o.npy")).astype(np.float64)
    norm = np.linalg.norm(o, axis=1)
    ok = np.isfinite(norm) & (norm > 0)
    o = np.where(ok[:, None], o / np.where(ok, norm, 1.0)[:, None], 0.0)
    segs, gt = load_strand(os.path.join(data, "synthetic_hair", "gt_strands.hair"))
    counts, samples = hm.resample_strands(segs, gt.astype(np.float32), 0.001)
    tan, valid = hm.strand_tangents(counts, samples)
    flags = hm.match_flags(p, o, ok.astype(np.uint8), samples, tan, valid, dist=[0.005], angle_deg=[30.0])
    return float((flags & 1).sum()) / max(len(p), 1), len(p)


def _conf_threshold():
    import yaml

    with open(os.path.join(ROOT, "configs", "reconstruct", "synthetic_hair.yaml")) as f:
        return float(yaml.safe_load(f)["PMVO"]["conf_threshold"])


def test_gabor_on_the_photographs_recovers_the_strand_directions(tmp_path):
    from monohair_amd import gabor, synth, synth_hair as sh
    from monohair_amd.camera import cameras_from_list
    from monohair_amd.pmvo_utils import read_obj

    strands = sh.make_hairstyle(STRANDS, POINTS, seed=0)
    cams = cameras_from_list(synth.make_cameras(V, H, W, scale=1.7, rings=1))
    synth.sphere_obj(str(tmp_path / "bust.obj"), sh.BUST_R, 24, 48)          # the bust write_case writes
    bust = read_obj(str(tmp_path / "bust.obj"))
    gray = sh.photo_planes(strands, cams, H, W, seed=0, bust=bust, device=DEV)
    assert tuple(gray.shape) == (V, H, W)
    k8, c8 = gabor.orientation_maps_device([gray[v] for v in range(V)], device=DEV, return_codes=True)
    depth, ori, conf, mask = sh.capture_planes(strands, cams, H, W, bust=bust, device=DEV)
    k8, c8, ori, conf, mask = (t.cpu().numpy() for t in (k8, c8, ori, conf, mask))
    C = (mask == 255) & (conf >= 128)
    P = C & (c8.astype(np.float64) > 255.0 * _conf_threshold())

    def within(ref):
        d = np.abs((k8[P].astype(np.int64) - ref[P].astype(np.int64) + 90) % 180 - 90)
        return d

    err = within(ori)
    share = float((err <= 15).mean())
    turned = float((within((ori.astype(np.int64) + 90) % 180) <= 15).mean())
    print("Gabor on the photographs: share %.4f, turned %.4f, |P| = %d of |C| = %d (%.4f), median error %.1f degrees"
          % (share, turned, int(P.sum()), int(C.sum()), P.sum() / max(int(C.sum()), 1), float(np.median(err))))
    assert C.sum() > 0
    assert P.sum() * 4 >= C.sum()
    assert share > turned
    assert share > 1.0 / 6.0


@pytest.fixture(scope="module")
def true_run(tmp_path_factory):
    from monohair_amd import synth_hair

    data = str(tmp_path_factory.mktemp("hair_photo") / "data")
    base = synth_hair.write_case(data, "synthetic_hair", V=V, H=H, W=W, seed=0, n_strands=STRANDS, n_points=POINTS,
                                 photo=True)
    for d in ("capture_images", "best_ori", "conf", "Ori", "gt_best_ori", "gt_conf", "hair_mask", "render_depth"):
        assert len(os.listdir(os.path.join(base, d))) == V, d
    env = dict(os.environ, PYTHONPATH=ROOT)
    _run([os.path.join(ROOT, "PMVO.py")] + _common(data) + ["--name=t"], env)
    return data, env


def test_written_photographs_are_gray_pictures_and_the_codes_are_gabors(true_run):
    from PIL import Image

    data, _ = true_run
    base = os.path.join(data, "synthetic_hair")
    img = Image.open(os.path.join(base, "capture_images", "view_000.png"))
    assert img.mode == "L" and img.size == (W, H)
    a = np.array(img)
    assert len(np.unique(a)) > 32                                    # a picture, not a code plane
    gt = np.array(Image.open(os.path.join(base, "gt_best_ori", "view_000.png")))
    got = np.array(Image.open(os.path.join(base, "best_ori", "view_000.png")))
    assert gt.shape == got.shape == (H, W) and got.max() < 180 and not np.array_equal(gt, got)


def test_photographed_capture_beats_the_control_turned_by_90_degrees(true_run, tmp_path):
    from PIL import Image

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
    true_share, n_true = _share(data, "t")
    control_share, n_control = _share(control, "t")
    print("share of select_p rows that agree with the ground truth: photographed capture %.4f of %d, control %.4f of %d"
          % (true_share, n_true, control_share, n_control))
    assert n_true > 0 and n_control > 0
    assert true_share > control_share


def test_strands_grown_from_photographs_are_scored_against_the_ground_truth(true_run):
    data, env = true_run
    _run([os.path.join(ROOT, "HairGrow.py")] + _common(data) + ["--name=t", "--HairGenerate.num_scalp_samples=2000"], env)
    out = os.path.join(data, "synthetic_hair", "output", "t_seed3", "refine")
    pred = os.path.join(out, "connected_strands.hair")
    assert os.path.exists(pred)
    report = os.path.join(out, "scores.json")
    r = _run(["-m", "monohair_amd.hairmetrics", pred, os.path.join(data, "synthetic_hair", "gt_strands.hair"), "--json",
              report], env)
    print(r.stdout)
    assert os.path.exists(report)
    res = json.load(open(report))
    print("f-scores", res["f_score"], "precision", res["precision"], "recall", res["recall"])
    assert res["counts"]["pred"]["valid"] > 0 and res["counts"]["gt"]["valid"] > 0
