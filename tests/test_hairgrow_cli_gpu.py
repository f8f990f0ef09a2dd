"""GPU: the drop-in command `HairGrow.py` -- its three stages driven one at a time on the volume of the reference's recorded
run (tests/golden/hair_connect.npz and hair_scalp.npz, case "shell": every file byte for byte), and the command as a user
runs it after `PMVO.py` on a synthetic capture (sampled scalp, repeatable from the saved samples, resumable stage by
stage)."""
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest
import yaml

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

HAIR_FILES = ("scalp_segment.hair", "scalp_segment_smooth.hair", "strands.hair", "connected_strands.hair")
STAGES = ("generate_segments", "connect_segments", "connect_scalp")


def test_stages_reproduce_the_reference_run_byte_for_byte(tmp_path):
    import scipy.io
    import torch

    import HairGrow

    z = np.load(os.path.join(GOLDEN, "hair_connect.npz"))
    zs = np.load(os.path.join(GOLDEN, "hair_scalp.npz"))
    save_path = tmp_path / "data" / "shell" / "output" / "chain" / "refine"
    save_path.mkdir(parents=True)
    # the volume files in PMVO's layout (tools/gen_golden_connect.py:157-159): Ori [Y,X,3*Z] (last index c*Z+z), Occ [Y,X,Z]
    G = tuple(int(g) for g in z["vol_shape"])
    occ = np.zeros(G, np.float32)
    occ[tuple(z["occ_nz"].T.astype(np.int64))] = 1
    ori = np.zeros(G + (3,), np.float32)
    ori[tuple(z["ori_nz"].T.astype(np.int64))] = z["ori_nz_val"]
    o = ori.transpose((0, 1, 3, 2)).reshape(G[0], G[1], G[2] * 3).transpose((1, 0, 2))
    scipy.io.savemat(str(save_path / "Ori3D.mat"), {"Ori": o})
    scipy.io.savemat(str(save_path / "Occ3D.mat"), {"Occ": occ.transpose((1, 0, 2))})
    del occ, ori, o
    np.savez(tmp_path / "samples.npz", points=z["scalp_points"], normals=z["scalp_normals"])
    case = dict(_parent_=os.path.join(ROOT, "configs", "reconstruct", "base.yaml"), name="chain", seed=0,
                bust_to_origin=[float(b) for b in z["bust"]], data=dict(root=str(tmp_path / "data"), case="shell"),
                PMVO=dict(infer_inner=False),
                HairGenerate=dict(connect_threshold=0.005, connect_dot_threshold=0.7, grow_threshold=0.8, out_ratio=0.2,
                                  scalp_samples=str(tmp_path / "samples.npz")))
    (tmp_path / "shell.yaml").write_text(yaml.safe_dump(case))

    def stage(on, seed):
        argv = ["--yaml=%s" % (tmp_path / "shell")] + ["--HairGenerate.%s=" % s for s in STAGES if s != on]
        args = HairGrow.config_parser(argv)
        assert args.save_path == str(save_path) and [bool(args.HairGenerate[s]) for s in STAGES] == [s == on for s in STAGES]
        assert np.array_equal(args.bust_to_origin, z["bust"])
        seed()                                   # as the generators seeded the reference's run, after the command's own seeding
        T = HairGrow.run(args)
        assert on + "_s" in T and not any(s + "_s" in T for s in STAGES if s != on) and T["total_s"] > 0
        return T

    stage("generate_segments", lambda: torch.manual_seed(77))
    assert (save_path / "scalp_segment.hair").read_bytes() == z["seg_hair"].tobytes()
    assert (save_path / "scalp_segment_smooth.hair").read_bytes() == z["seg_smooth_hair"].tobytes()
    assert int(np.load(save_path / "num_root.npy")) == int(z["num_root"])
    assert not (save_path / "strands.hair").exists() and not (save_path / "scalp_samples.npz").exists()
    stage("connect_segments", lambda: np.random.seed(1234))
    assert np.random.random() == float(z["shell_next_random"])
    assert (save_path / "strands.hair").read_bytes() == z["strands_hair"].tobytes()
    assert not (save_path / "connected_strands.hair").exists()
    stage("connect_scalp", lambda: None)
    assert (save_path / "connected_strands.hair").read_bytes() == zs["connected_strands_hair"].tobytes()


def _run(script, argv, env):
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, cwd=ROOT, env=env, stdin=subprocess.DEVNULL,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r


def test_command_after_pmvo_samples_repeats_and_resumes(tmp_path):
    import json

    from monohair_amd import synth
    from monohair_amd.pmvo_utils import load_strand

    data = tmp_path / "data"
    synth.write_case(str(data), "synthetic_sphere", V=24, H=240, W=136, res=32)
    env = dict(os.environ, PYTHONPATH=ROOT)
    common = ["--yaml=configs/reconstruct/synthetic_sphere", "--data.root=%s" % data, "--data.image_size=[240,136]",
              "--PMVO.patch_size=3", "--seed=3"]
    grow = common + ["--HairGenerate.num_scalp_samples=2000"]
    _run("PMVO.py", common + ["--name=t1"], env)
    r = _run("HairGrow.py", grow + ["--name=t1"], env)
    T = json.loads(r.stdout.strip().splitlines()[-1])
    assert all(s + "_s" in T for s in STAGES) and "scalp_samples_s" in T and "load_volume_s" in T
    out = data / "synthetic_sphere" / "output" / "t1_seed3" / "refine"
    for f in HAIR_FILES + ("num_root.npy", "scalp_samples.npz"):
        assert (out / f).exists(), f
    smp = np.load(out / "scalp_samples.npz")
    assert smp["points"].shape == (2000, 3) == smp["normals"].shape
    assert smp["points"].dtype == np.float32 == smp["normals"].dtype
    assert np.allclose(np.linalg.norm(smp["normals"], axis=1), 1, atol=1e-6)
    num_root = int(np.load(out / "num_root.npy"))
    assert num_root >= 1
    segs, pts = load_strand(str(out / "connected_strands.hair"))
    assert len(segs) >= num_root and pts.shape == (sum(segs), 3) and np.isfinite(pts).all()
    first = {f: (out / f).read_bytes() for f in HAIR_FILES}

    # the saved samples fed back under another name: nothing is sampled, every .hair file repeats
    out2 = data / "synthetic_sphere" / "output" / "t2_seed3" / "refine"
    out2.mkdir(parents=True)
    for f in ("Occ3D.mat", "Ori3D.mat"):
        shutil.copy(out / f, out2 / f)
    _run("HairGrow.py", grow + ["--name=t2", "--HairGenerate.scalp_samples=%s" % (out / "scalp_samples.npz")], env)
    assert not (out2 / "scalp_samples.npz").exists()
    for f in HAIR_FILES:
        assert (out2 / f).read_bytes() == first[f], f
    assert int(np.load(out2 / "num_root.npy")) == num_root

    # resumed after the first stage: num_root.npy is read, scalp_segment.hair stays, strands.hair comes out the same
    (out / "strands.hair").unlink()
    (out / "connected_strands.hair").unlink()
    stamp = os.stat(out / "scalp_segment.hair").st_mtime_ns
    r = _run("HairGrow.py", grow + ["--name=t1", "--HairGenerate.generate_segments="], env)
    T = json.loads(r.stdout.strip().splitlines()[-1])
    assert "generate_segments_s" not in T and "scalp_samples_s" not in T and "connect_segments_s" in T
    assert os.stat(out / "scalp_segment.hair").st_mtime_ns == stamp
    assert (out / "strands.hair").read_bytes() == first["strands.hair"]
    assert (out / "connected_strands.hair").read_bytes() == first["connected_strands.hair"]
