"""GPU, in process (no PMVO.py run): the capture agreement on a synthetic capture whose strands are known -- 200 strands of 32
points, 8 views of 120 x 68 with the bust, written by synth_hair.write_case and read back through the loaders PMVO.py uses.

(a) the true strands agree with their own capture more than with the same capture whose orientation codes are all turned by 90
    degrees; (b) mixed with decoys -- every strand turned by 90 degrees about the horizontal x axis through its own centroid (the
    model's gravity is -y: hanging hair comes to lie across the view) -- pruning at the defaults keeps a larger share of the true
    strands than of the decoys, and the pruned set is more precise against the true strands than the mix; (c) the two commands
    write what the API returns.  The measured figures are printed; only the inequalities are asserted."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
V, H, W, STRANDS, POINTS = 8, 120, 68, 200, 32


@pytest.fixture(scope="module")
def case(tmp_path_factory):
    from monohair_amd import synth_hair as sh
    from monohair_amd.camera import load_cam, parsing_camera
    from monohair_amd.pmvo_utils import load_maps_u8, read_obj, write_strand

    data = str(tmp_path_factory.mktemp("hairreproj") / "data")
    counts, points = sh.make_hairstyle(n_strands=STRANDS, n_points=POINTS, seed=0)
    base = sh.write_case(data, "synthetic_hair", V=V, H=H, W=W, strands=(counts, points), device=DEV)
    cams = parsing_camera(load_cam(os.path.join(base, "ours", "cam_params.json")), os.path.join(base, "capture_images"))
    planes = tuple(np.stack(list(d.values())) for d in load_maps_u8(cams, os.path.join(base, "best_ori"),
                                                                     os.path.join(base, "conf"),
                                                                     os.path.join(base, "hair_mask")))
    bust = read_obj(os.path.join(base, "ours", "bust_long_tsfm.obj"))
    # the decoys: R = a quarter turn about x, (x, y, z) -> (x, -z, y), about each strand's centroid
    p = points.astype(np.float64).reshape(STRANDS, POINTS, 3)
    c = p.mean(1, keepdims=True)
    d = p - c
    decoys = (np.stack([d[..., 0], -d[..., 2], d[..., 1]], -1) + c).reshape(-1, 3).astype(np.float32)
    mix = (np.concatenate([counts, counts]), np.concatenate([points, decoys]))
    mix_path = os.path.join(base, "mix.hair")
    write_strand(mix[1], mix_path, [int(k) for k in mix[0]])
    return dict(data=data, base=base, cams=cams, planes=planes, bust=bust, true=(counts, points), mix=mix, mix_path=mix_path)


def test_agreement_falls_on_a_capture_turned_by_90_degrees(case):
    from monohair_amd import hairreproj

    ori, conf, mask = case["planes"]
    assert ori.shape == (V, H, W) and ori.max() < 180
    turned = ((ori.astype(np.int64) + 90) % 180).astype(np.uint8)
    res = {}
    for name, o in (("own capture", ori), ("turned", turned)):
        res[name] = hairreproj.score_support(case["true"], case["cams"], (o, conf, mask), bust=case["bust"], device=DEV)
        print(name)
        for line in hairreproj.format_scores(res[name])[:1]:
            print("  " + line)
    k = res["own capture"]["angles_deg"].index(20.0)
    own, other = res["own capture"]["overall"], res["turned"]["overall"]
    assert own["counts"]["confident"] > 0 and other["counts"]["confident"] > 0
    assert own["counts"]["visible"] == own["counts"]["on_hair"] > 0           # its own capture: exact by construction
    assert own["agreement"][k] > other["agreement"][k]


def test_pruning_separates_true_strands_from_decoys(case):
    from monohair_amd import hairmetrics, hairreproj

    result, rows = hairreproj.score_support(case["mix"], case["cams"], case["planes"], bust=case["bust"], device=DEV,
                                            return_counts=True)
    pruned, keep = hairreproj.prune_strands(case["mix"], rows)
    kept_true, kept_decoy = float(keep[:STRANDS].mean()), float(keep[STRANDS:].mean())
    print("mix: " + hairreproj.format_scores(result)[0])
    print("kept share of the true strands %.4f, of the decoys %.4f" % (kept_true, kept_decoy))
    assert kept_true > kept_decoy
    before = hairmetrics.score_strands(case["mix"], case["true"], device=DEV)
    after = hairmetrics.score_strands(pruned, case["true"], device=DEV)
    k = [list(t) for t in before["thresholds"]].index([0.003, 30.0])
    print("precision at 3 mm / 30 deg: mix %.4f, pruned %.4f" % (before["precision"][k], after["precision"][k]))
    assert after["precision"][k] > before["precision"][k]


def _run(argv, env):
    r = subprocess.run([sys.executable] + argv, cwd=ROOT, env=env, stdin=subprocess.DEVNULL, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_the_commands_write_what_the_api_returns(case, tmp_path):
    from monohair_amd import hairreproj
    from monohair_amd.pmvo_utils import load_strand

    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--yaml=configs/reconstruct/synthetic_hair", "--data.root=%s" % case["data"],
              "--data.image_size=[%d,%d]" % (H, W), "--strands", case["mix_path"]]
    report = str(tmp_path / "support.json")
    r = _run(["-m", "monohair_amd.hairreproj", "score"] + common + ["--json", report], env)
    print(r.stdout[-1500:])
    api, rows = hairreproj.score_support(case["mix_path"], case["cams"], case["planes"], bust=case["bust"],
                                         conf_threshold=0.15, device=DEV, return_counts=True)
    assert json.load(open(report)) == json.loads(json.dumps(api))
    assert api["strands"] == 2 * STRANDS and api["overall"]["counts"]["confident"] > 0
    out = str(tmp_path / "pruned.hair")
    _run(["-m", "monohair_amd.hairreproj", "prune"] + common + ["--out", out, "--min-cover", "0.5", "--min-agree", "0.5"], env)
    (kc, kp), keep = hairreproj.prune_strands(case["mix_path"], rows)
    segments, points = load_strand(out)
    assert 0 < len(segments) < 2 * STRANDS and segments == [int(c) for c in kc]
    assert points.astype(np.float32).tobytes() == kp.tobytes()
    # the input is never overwritten
    r = subprocess.run([sys.executable, "-m", "monohair_amd.hairreproj", "prune"] + common + ["--out", case["mix_path"]],
                       cwd=ROOT, env=env, stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "input file" in r.stderr
    assert load_strand(case["mix_path"])[0] == [int(c) for c in case["mix"][0]]
