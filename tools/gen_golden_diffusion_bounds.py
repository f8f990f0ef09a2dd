"""Golden vectors of the scalp diffusion with every decision ON its bound (tests/golden/scalp_diffusion_bounds.npz): the
imported reference function diffusion_scalp (Utils/PMVO_utils.py:467-593) run on the hand-written cases of
tests/scalp_diffusion_bound_cases.py, once as they are ("cases") and once tiled to 257 samples ("tiled").

    python tools/gen_golden_diffusion_bounds.py

The reference is imported and traced from outside exactly as tools/gen_golden_diffusion.py does (its run_reference is
used as it is); in addition every value torch.cosine_similarity returns is recorded, call by call and per sample (the
calls of a sample follow from its restarts and its end: three per failed turn, then one or two).  Recorded sparse: the
voxels with any bit set, with their occupancies and orientations themselves, and the voxels the reference changed.

Asserted on the reference's output ALONE: every case reaches what it exists for, nothing raised, no row lies outside the
volume, no tangent has zero length.  Then: the numpy restatement (tests/scalp_diffusion_np.py) reproduces every record;
each other form of it (scalp_diffusion_bound_cases.SWITCHES) changes at least one record, and only records of the cases
built for that bound; the forms in UNREACHABLE change none.
"""
import json
import os
import shutil
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

from gen_golden_diffusion import run_reference  # noqa: E402
from ref_import import import_reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "scalp_diffusion_bounds.npz")
F32 = np.float32
TILED = 257


def run_recording_cosines(U, pts, nrm, ori, occ, tmp):
    """run_reference, with torch.cosine_similarity's returned values split per sample"""
    flat, orig = [], torch.cosine_similarity

    def cos(*a, **k):
        r = orig(*a, **k)
        assert r.dtype == torch.float32 and r.numel() == 1
        flat.append(r.numpy().reshape(()).copy())
        return r

    torch.cosine_similarity = cos
    try:
        rec = run_reference(U, pts, nrm, ori, occ, tmp)
    finally:
        torch.cosine_similarity = orig
    flat = np.array(flat, F32)
    offs, k = [0], 0
    for i in range(len(pts)):
        for _ in range(int(rec["restarts"][i])):
            assert flat[k] == flat[k + 2] and flat[k + 1] == -flat[k] and not flat[k] > 0.5 and not flat[k + 1] > 0.5
            k += 3
        if rec["status"][i] == 0:
            k += 1 if flat[k] > 0.5 else 2
            assert flat[k - 1] > 0.5
        offs.append(k)
    assert k == len(flat), (k, len(flat))
    rec["cos_values"], rec["cos_offsets"] = flat, np.array(offs, np.int32)
    rec["voxel"] = rec["voxel"].astype(np.int16)
    return rec


def main():
    import scalp_diffusion_bound_cases as bc
    import scalp_diffusion_np as rs
    import scipy

    U = import_reference()["PMVO_utils"]
    case = bc.build()
    print(json.dumps(case["info"]))
    m = len(case["points"])
    out = dict(meta=np.array("numpy %s, scipy %s, torch %s" % (np.__version__, scipy.__version__, torch.__version__)),
               info=np.array(json.dumps(case["info"])))
    for k, v in case["expect"].items():
        out["expect_" + k] = v
    tmp = tempfile.mkdtemp(prefix="mh_dfb_")
    ori, occ = case["ori"], case["occ"]
    runs = {}
    for tag, (pts, nrm) in (("cases", (case["points"], case["normals"])), ("tiled", bc.tiled(case, TILED))):
        rec = run_recording_cosines(U, pts, nrm, ori, occ, tmp)           # an IndexError of the reference ends it here
        runs[tag] = (pts, nrm, rec)
        bc.store_volume(out, tag, ori, occ)
        out[tag + "_points"], out[tag + "_normals"] = pts, nrm
        for k, v in rec.items():
            out["%s_%s" % (tag, k)] = v
    shutil.rmtree(tmp)
    bc.assert_properties(case, runs["cases"][2])

    base = {}
    for tag, (pts, nrm, rec) in runs.items():
        base[tag] = rs.diffusion_scalp(pts, nrm, ori, occ)
        bc.check_record(out, tag, base[tag])
        det = base[tag][2]
        print(tag, "status", np.bincount(det["status"], minlength=5).tolist(), "rows", len(det["total_sample"]),
              "changed", len(rec["changed"]), "cosine calls", len(rec["cos_values"]))
    pts, nrm, _ = runs["cases"]
    wrong = {}
    for name, (rules, owners) in bc.SWITCHES.items():
        d = bc.differing_samples(base["cases"], rs.diffusion_scalp(pts, nrm, ori, occ, rules=rules))
        names = bc.names_of(case["expect"], d, m)
        print("%-26s changes %2d samples: %s" % (name, len(d), ", ".join(names)))
        wrong.update({name: names} if not d or not all(any(n.startswith(o) for o in owners) for n in names) else {})
    assert not wrong, wrong
    for name, (rules, why) in bc.UNREACHABLE.items():
        for tag, (pts, nrm, _) in runs.items():
            assert not bc.differing_samples(base[tag], rs.diffusion_scalp(pts, nrm, ori, occ, rules=rules)), name
        print("%-26s changes nothing: %s" % (name, why))
    np.savez_compressed(OUT, **out)
    print("scalp_diffusion_bounds written: %.1f kB" % (os.path.getsize(OUT) / 1024))


if __name__ == "__main__":
    main()
