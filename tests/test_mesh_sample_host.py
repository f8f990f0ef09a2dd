"""CPU: the host side of the scalp sampler and of the HairGrow.py command -- the stratified allocation between the two
kernels of csrc/meshsample.hip (hairgrow.scalp_allocation) against a plain Python loop, pmvo_utils.read_obj_normals on
OBJ text written here, and the paths and defaults of HairGrow.config_parser."""
import math
import os

import numpy as np
import pytest
import yaml

from conftest import ROOT


# ------------------------------------------------------------------ allocation
def loop_allocation(area, n):
    """Open3D's SamplePointsUniformly loop over the triangles, without its random draws: (bounds, count per triangle,
    triangle of every sample).  The total is numpy's area.sum(), as the allocation is specified."""
    total = float(np.asarray(area, np.float64).sum())
    c, bounds = 0.0, []
    for a in area:
        c = c + float(a) / total
        bounds.append(int(math.floor(n * c + 0.5)))
    bounds[-1] = n
    counts, owner, i = [0] * len(bounds), [], 0
    for t, b in enumerate(bounds):
        while i < b:
            owner.append(t)
            counts[t] += 1
            i += 1
    return bounds, counts, owner


def allocation_cases():
    rng = np.random.default_rng(8)
    mid = rng.random(40) + 0.01
    mid[17] = 0.0
    end = rng.random(40) + 0.01
    end[-1] = 0.0
    return [("one", np.array([0.37]), 1), ("one_many", np.array([2.5]), 7), ("two", np.array([0.2, 0.5]), 9),
            ("two_one_sample", np.array([0.7, 0.1]), 1), ("sparse", rng.random(1000) + 1e-3, 65),
            ("zero_mid", mid, 1000), ("zero_end", end, 1000), ("zero_end_few", end, 65)]


@pytest.mark.parametrize("name,area,n", allocation_cases(), ids=[c[0] for c in allocation_cases()])
def test_allocation_matches_the_plain_loop(name, area, n):
    from monohair_amd.hairgrow import scalp_allocation

    B = scalp_allocation(area, n)
    bounds, counts, owner = loop_allocation(area, n)
    assert B.dtype == np.int64 and B.tolist() == bounds
    assert int(B[-1]) == n and (np.diff(B) >= 0).all() and B[0] >= 0
    got_counts = np.diff(np.concatenate([[0], B]))
    assert got_counts.tolist() == counts and int(got_counts.sum()) == n == len(owner)
    assert (got_counts[np.asarray(area) == 0] == 0).all()
    # sample i belongs to the first triangle whose bound exceeds i
    assert np.searchsorted(B, np.arange(n), side="right").tolist() == owner
    if name == "sparse":
        assert (got_counts == 0).sum() > 900


def test_allocation_refuses_what_has_no_answer():
    from monohair_amd._lib import MhError
    from monohair_amd.hairgrow import scalp_allocation

    for area in ([], [0.0, 0.0], [1.0, -0.5], [1.0, float("nan")]):
        with pytest.raises(MhError):
            scalp_allocation(np.array(area, np.float64), 5)


# ------------------------------------------------------------------ read_obj_normals
_V = ["v 0 0 0", "v 1 0 0", "v 0 1 0", "v 0 0 1"]
_VN = ["vn 0 0 2", "vn 0 3 0", "vn 1 0 0", "vn 0.6 0.8 0"]


def _write(tmp_path, lines):
    p = tmp_path / "m.obj"
    p.write_text("\n".join(lines) + "\n")
    return str(p)


def test_read_obj_normals_v_vn(tmp_path):
    from monohair_amd.pmvo_utils import read_obj, read_obj_normals

    path = _write(tmp_path, _V + _VN + ["f 1//1 2//2 3//3", "f 1//1 3//3 4//4"])
    v, f, n = read_obj_normals(path)
    v0, f0 = read_obj(path)
    assert np.array_equal(v, v0) and np.array_equal(f, f0) and v.dtype == np.float64
    assert np.array_equal(n, [[0, 0, 2], [0, 3, 0], [1, 0, 0], [0.6, 0.8, 0]])        # the file's records, not normalised


def test_read_obj_normals_v_vt_vn_with_their_own_indices(tmp_path):
    from monohair_amd.pmvo_utils import read_obj_normals

    # normal indices differ from the vertex indices; vertex 1 is given normal 4 and then normal 2: the last corner stays;
    # the second face is a quad (fan-triangulated) and uses a relative index
    path = _write(tmp_path, _V + ["vt 0 0", "vt 1 1"] + _VN + ["f 1/1/4 2/2/3 3/1/1", "f 1/1/2 3/2/1 4/1/-1 2/2/3"])
    v, f, n = read_obj_normals(path)
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 1]]
    assert np.array_equal(n, [[0, 3, 0], [1, 0, 0], [0, 0, 2], [0.6, 0.8, 0]])


def test_read_obj_normals_without_vn_falls_back_to_vertex_normals(tmp_path):
    from monohair_amd.pmvo_utils import read_obj_normals, vertex_normals

    faces = ["f 1 2 3", "f 1 3 4", "f 1 4 2"]
    v, f, n = read_obj_normals(_write(tmp_path, _V + faces))
    assert f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 1]]
    assert np.array_equal(n, vertex_normals(v, f)) and np.allclose(np.linalg.norm(n, axis=1), 1)
    # `vn` records, but a face corner that names none: the same fallback
    v2, f2, n2 = read_obj_normals(_write(tmp_path, _V + _VN + ["f 1//1 2//2 3//3", "f 1 3 4"]))
    assert np.array_equal(n2, vertex_normals(v2, f2))
    # a vertex no face uses does not matter: the file's normals are taken, that vertex keeps a zero normal
    v3, f3, n3 = read_obj_normals(_write(tmp_path, _V + _VN + ["f 1//2 2//3 3//4"]))
    assert np.array_equal(n3, [[0, 3, 0], [1, 0, 0], [0.6, 0.8, 0], [0, 0, 0]])


# ------------------------------------------------------------------ the command's configuration step
def _case_yaml(tmp_path, text):
    (tmp_path / "case.yaml").write_text(text)
    return ["--yaml=%s" % (tmp_path / "case"), "--data.root=%s" % (tmp_path / "data")]


def test_config_paths_refine_full_and_diffusion(tmp_path):
    import HairGrow

    base = _case_yaml(tmp_path, "_parent_: %s\nname: run\ndata: {case: head}\n"
                      % os.path.join(ROOT, "configs", "reconstruct", "base.yaml"))
    out = os.path.join(str(tmp_path), "data", "head", "output", "run")
    a = HairGrow.config_parser(base + ["--PMVO.infer_inner!"])
    assert a.output_path == out and a.save_path == os.path.join(out, "refine")
    assert a.data.Occ3D_path == os.path.join(out, "refine", "Occ3D.mat")
    assert a.data.Ori3D_path == os.path.join(out, "refine", "Ori3D.mat")
    assert a.data.scalp_path == os.path.join(str(tmp_path), "data", "head", "ours", "scalp_tsfm.obj")
    assert os.path.exists(os.path.join(out, "options.yaml"))
    b = HairGrow.config_parser(base + ["--PMVO.infer_inner", "--scalp_diffusion", "--seed=3"])
    out3 = out + "_seed3"
    assert b.save_path == os.path.join(out3, "full")
    assert b.data.Occ3D_path == os.path.join(out3, "full", "Occ3D_diffusion.mat")
    assert b.data.Ori3D_path == os.path.join(out3, "full", "Ori3D_diffusion.mat")
    c = HairGrow.config_parser(base + ["--PMVO.infer_inner!", "--scalp_diffusion"])
    assert c.data.Occ3D_path == os.path.join(out, "refine", "Occ3D_diffusion.mat")


def test_config_fills_the_reference_defaults_a_case_file_omits(tmp_path):
    import HairGrow

    text = yaml.safe_dump(dict(name="n", seed=0, gpu=0, cpu=None, output_root="output", image_camera_path="ours/c.json",
                               bbox_min=[-0.32, -0.32, -0.24], bust_to_origin=[0.0, 0.0, 0.0],
                               data=dict(root="data", case="k", image_size=[8, 8], strands_path="s", bust_path="b",
                                         scalp_path="ours/scalp_tsfm.obj"),
                               PMVO=dict(infer_inner=False), HairGenerate=dict(out_ratio=0.2, connect_scalp=None)))
    a = HairGrow.config_parser(_case_yaml(tmp_path, text))
    hg = a.HairGenerate
    assert (hg.connect_threshold, hg.grow_threshold, hg.connect_dot_threshold) == (0.005, 0.8, 0.7)
    assert hg.generate_segments is True and hg.connect_segments is True
    assert hg.connect_scalp is None and hg.out_ratio == 0.2                   # what the case file says stays
    assert hg.num_scalp_samples == 60000 and not hg.scalp_samples
    assert a.save_path.endswith(os.path.join("output", "n", "refine")) and a.data.Occ3D_path.endswith("Occ3D.mat")
    # the repository's own base file carries the same defaults
    d = yaml.safe_load(open(os.path.join(ROOT, "configs", "reconstruct", "base.yaml")))["HairGenerate"]
    assert d == HairGrow.HAIRGENERATE_DEFAULTS
