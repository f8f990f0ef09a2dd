"""CPU only: scalp diffusion with every decision ON its bound.  The numpy restatement (tests/scalp_diffusion_np.py) is
held to the reference's own run of the hand-written cases (tests/scalp_diffusion_bound_cases.py, recorded in
tests/golden/scalp_diffusion_bounds.npz by tools/gen_golden_diffusion_bounds.py), alone and tiled to 257 samples, on
every recorded quantity bit for bit -- the values torch.cosine_similarity returned to the reference included; every case's
own property is read from the record; every other form of a decision changes recorded rows, and only rows of the cases
built for that decision; the restatement's cosine equals the installed torch.cosine_similarity around 0.5 and on
degenerate rows."""
import json
import os

import numpy as np
import pytest
import torch

import scalp_diffusion_bound_cases as bc
import scalp_diffusion_np as rs
from conftest import GOLDEN

F32 = np.float32
TAGS = ("cases", "tiled")
RECORDED = ("status", "step", "restarts", "end_point", "first_normal", "last_normal", "total_sample", "total_normal", "voxel",
            "changed", "changed_ori", "changed_occ", "cos_values", "cos_offsets")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "scalp_diffusion_bounds.npz"))


@pytest.fixture(scope="module")
def case():
    return bc.build()


@pytest.fixture(scope="module")
def base(golden):
    return {tag: rs.diffusion_scalp(*bc.load(golden, tag)) for tag in TAGS}


def test_fixture_holds_the_cases_of_the_module(golden, case):
    pts, nrm, ori, occ = bc.load(golden, "cases")
    assert bc.same_bits(pts, case["points"]) and bc.same_bits(nrm, case["normals"])
    assert bc.same_bits(ori, case["ori"]) and bc.same_bits(occ, case["occ"])
    assert occ.shape[1:] == (bc.Z, bc.Y, bc.X) and bc.Z <= 16 and bc.Y <= 24 and bc.X <= 48
    assert json.loads(str(golden["info"])) == json.loads(json.dumps(case["info"]))
    for k, v in case["expect"].items():
        assert np.array_equal(golden["expect_" + k], v), k
    tp, tn, tori, tocc = bc.load(golden, "tiled")
    assert len(tp) == 257 and bc.same_bits(tp, bc.tiled(case, 257)[0]) and bc.same_bits(tn, bc.tiled(case, 257)[1])
    assert bc.same_bits(tori, ori) and bc.same_bits(tocc, occ)
    held = occ[0][occ[0].view(np.uint32) != 0]
    assert np.isnan(held).any() and (np.signbit(held) & (held == 0)).any() and (held == F32(1e-45)).any()
    assert (held == F32(1e-39)).any() and not np.isin(held[~np.isnan(held)], (0.0, 1.0)).all()


@pytest.mark.parametrize("tag", TAGS)
def test_restatement_reproduces_every_record(golden, base, tag):
    bc.check_record(golden, tag, base[tag])
    det = base[tag][2]
    assert (det["status"] != rs.LEFT).all() and det["total_normal"].any(1).all() and (det["voxel"] >= 0).all()


def test_every_case_reaches_its_bound_in_the_reference_run(golden, case):
    bc.assert_properties(case, {k: golden["cases_" + k] for k in RECORDED})
    info = case["info"]
    assert all(v >= 1 for v in info["bound_hits"].values()) and info["step_lands_on_integer"] is not None
    assert all(rows == bc.FORM_ROWS for rows, trials in info["form_trials"].values())
    assert info["param_steps_that_differ"] == [5, 6, 7, 9] and info["param_div_step"] in (5, 6, 7, 9)
    assert sorted(golden["cases_step"][golden["cases_status"] == 0].tolist())[-1] == 9
    assert set(range(1, 10)) <= set(golden["cases_step"][golden["cases_status"] == 0].tolist())


@pytest.mark.parametrize("name", sorted(bc.SWITCHES))
def test_every_other_form_changes_recorded_rows_of_its_own_cases(golden, case, base, name):
    rules, owners = bc.SWITCHES[name]
    pts, nrm, ori, occ = bc.load(golden, "cases")
    other = rs.diffusion_scalp(pts, nrm, ori, occ, rules=rules)
    with pytest.raises(AssertionError):
        bc.check_record(golden, "cases", other)
    names = bc.names_of(case["expect"], bc.differing_samples(base["cases"], other), len(pts))
    assert names and all(any(n.startswith(o) for o in owners) for n in names), names


@pytest.mark.parametrize("name", sorted(bc.UNREACHABLE))
def test_forms_the_cases_cannot_tell_apart_change_nothing(golden, base, name):
    rules, why = bc.UNREACHABLE[name]
    for tag in TAGS:
        pts, nrm, ori, occ = bc.load(golden, tag)
        assert not bc.differing_samples(base[tag], rs.diffusion_scalp(pts, nrm, ori, occ, rules=rules)), why


def cos_sweep(n=20000, seed=5):
    """-> (a [M,3], b [M,3]) float32: n pairs turned to acos(0.5) +- 2e-7 with random lengths and signs, then rows with
    components 0, -0, 1e-45, 1e-30, 1e-8 in either operand and as whole rows"""
    rng = np.random.default_rng(seed)
    b = rng.normal(size=(n, 3))
    b /= np.linalg.norm(b, axis=1, keepdims=True)
    a = bc.normals_at_60_degrees(rng, b, n).astype(np.float64) * rng.uniform(0.3, 3.0, (n, 1)) * rng.choice([-1.0, 1.0], (n, 1))
    b = b * rng.uniform(0.3, 3.0, (n, 1))
    xs, ys = [a.astype(F32)], [b.astype(F32)]
    plain = np.array([[0.3, -0.8, 0.52], [1.0, 0.0, 0.0], [-2.0, 1.0, 0.5], [0.0, 1.0, 0.0]], F32)
    da, db = [], []
    for v in (0.0, -0.0, 1e-45, -1e-45, 1e-30, -1e-30, 1e-8, -1e-8):
        whole = np.full(3, v, F32)
        for p in plain:
            for k in range(3):
                one = p.copy()
                one[k] = F32(v)
                da += [one, p, one, whole, p, -one]
                db += [p, one, one, p, whole, plain[1]]
        da.append(whole)
        db.append(whole)
    return np.concatenate([xs[0], np.array(da, F32)]), np.concatenate([ys[0], np.array(db, F32)])


def test_restated_cosine_equals_the_installed_torch_around_the_bound_and_on_degenerate_rows():
    a, b = cos_sweep()
    want = torch.cosine_similarity(torch.from_numpy(a), torch.from_numpy(b), dim=-1).numpy()
    got = rs.cosine32_rows(a, b)
    assert len(a) > 20000 and bc.same_bits(got, want)
    for v in (bc.HALF, bc.HALF_LO, bc.HALF_HI):
        assert (np.abs(want[:20000]) == v).sum() > 100
    assert not (np.signbit(want) & (want == 0)).any() and (want[20000:] == 0).sum() > 20
    one = np.array([torch.cosine_similarity(torch.from_numpy(a[k]), torch.from_numpy(b[k]), dim=-1).item()
                    for k in range(19990, len(a))], F32)           # called as the reference calls it: one pair
    assert bc.same_bits(one, want[19990:]) and bc.same_bits(np.array([rs.cosine32(a[k], b[k]) for k in range(19990, len(a))]), one)
    for form in bc.FORMS:                                           # and every other form IS another function
        assert not bc.same_bits(rs.cosine32_rows(a, b, form), want), form
