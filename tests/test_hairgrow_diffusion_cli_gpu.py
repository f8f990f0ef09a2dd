"""GPU: `HairGrow.py --scalp_diffusion` on the synthetic capture of tests/test_hairgrow_cli_gpu.py -- from PMVO's Occ3D.mat /
Ori3D.mat to connected_strands.hair with no hand-made file: the stage in front writes Occ3D_diffusion.mat /
Ori3D_diffusion.mat (equal to the API's result on the saved samples), the three stages run on them, a second run leaves the
files alone and repeats every .hair file, --HairGenerate.diffuse_scalp writes them again, and without --scalp_diffusion
nothing of this happens."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

HAIR_FILES = ("scalp_segment.hair", "scalp_segment_smooth.hair", "strands.hair", "connected_strands.hair")
STAGES = ("generate_segments", "connect_segments", "connect_scalp")
MATS = ("Occ3D_diffusion.mat", "Ori3D_diffusion.mat")


def test_scalp_diffusion_switch_runs_from_pmvo_output_to_connected_strands(tmp_path):
    import torch

    import HairGrow
    from monohair_amd import synth
    from monohair_amd.hairgrow import diffusion_scalp
    from monohair_amd.pmvo_utils import get_ground_truth_3D_occ, get_ground_truth_3D_ori, voxel_to_points

    data = tmp_path / "data"
    synth.write_case(str(data), "synthetic_sphere", V=24, H=240, W=136, res=32)
    common = ["--yaml=%s" % os.path.join(ROOT, "configs", "reconstruct", "synthetic_sphere"), "--data.root=%s" % data,
              "--data.image_size=[240,136]", "--PMVO.patch_size=3", "--seed=3"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "PMVO.py")] + common + ["--name=d1"], cwd=ROOT,
                       env=dict(os.environ, PYTHONPATH=ROOT), stdin=subprocess.DEVNULL, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    grow = common + ["--HairGenerate.num_scalp_samples=2000"]
    out = data / "synthetic_sphere" / "output" / "d1_seed3" / "refine"
    assert (out / "Occ3D.mat").exists() and not any((out / m).exists() for m in MATS)

    T = HairGrow.main(grow + ["--name=d1", "--scalp_diffusion"])
    assert all(s + "_s" in T for s in STAGES) and "diffuse_scalp_s" in T and "scalp_samples_s" in T
    for f in HAIR_FILES + MATS + ("scalp_samples.npz",):
        assert (out / f).exists(), f
    # the two files hold what the API returns for the saved samples on PMVO's volume
    smp = np.load(out / "scalp_samples.npz")
    nrm = torch.from_numpy(smp["normals"] * np.array([1, -1, -1], np.float32))
    occ = torch.from_numpy(get_ground_truth_3D_occ(str(out / "Occ3D.mat"))).permute(3, 0, 1, 2)
    ori = torch.from_numpy(get_ground_truth_3D_ori(str(out / "Ori3D.mat"))).permute(3, 0, 1, 2)
    o, c, det = diffusion_scalp(voxel_to_points(torch.from_numpy(smp["points"].copy())), nrm, ori, occ, return_details=True)
    assert det["status"].shape == (2000,) and float(c.sum()) >= float(occ.sum())
    assert np.array_equal(get_ground_truth_3D_occ(str(out / MATS[0]))[..., 0], c[0].cpu().numpy())
    assert np.array_equal(get_ground_truth_3D_ori(str(out / MATS[1])), o.permute(1, 2, 3, 0).cpu().numpy())
    first = {f: (out / f).read_bytes() for f in HAIR_FILES + MATS}
    stamp = {m: os.stat(out / m).st_mtime_ns for m in MATS}

    # a second run finds the files: they stay, and every .hair file repeats
    T = HairGrow.main(grow + ["--name=d1", "--scalp_diffusion"])
    assert "diffuse_scalp_s" not in T and all(s + "_s" in T for s in STAGES)
    assert all(os.stat(out / m).st_mtime_ns == stamp[m] for m in MATS)
    for f in HAIR_FILES:
        assert (out / f).read_bytes() == first[f], f

    # forced: written again, the same bytes (behind the MAT header's text, which carries the creation time)
    T = HairGrow.main(grow + ["--name=d1", "--scalp_diffusion", "--HairGenerate.diffuse_scalp"] +
                      ["--HairGenerate.%s=" % s for s in STAGES])
    assert "diffuse_scalp_s" in T
    for m in MATS:
        assert os.stat(out / m).st_mtime_ns != stamp[m] and (out / m).read_bytes()[116:] == first[m][116:], m

    # without the switch: no diffusion file, whatever HairGenerate.diffuse_scalp says
    out2 = data / "synthetic_sphere" / "output" / "d2_seed3" / "refine"
    out2.mkdir(parents=True)
    for f in ("Occ3D.mat", "Ori3D.mat"):
        shutil.copy(out / f, out2 / f)
    T = HairGrow.main(grow + ["--name=d2", "--HairGenerate.diffuse_scalp"])
    assert "diffuse_scalp_s" not in T and (out2 / "connected_strands.hair").exists()
    assert not any((out2 / m).exists() for m in MATS)
