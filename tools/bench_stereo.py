"""Times of the photo-consistent carve (docs/PARITY.md f12): the default synthetic capture rendered as
photographs (24 views of 480 x 270, 2 000 strands), its silhouette hull on PMVO.py's candidate grid (512 x 512 x 384 at 1.25 mm)
refined at the defaults of monohair_amd.hairstereo, device events around each call, warm, the median of five --
mh_stereo_census, the compaction of the candidates (mh_select_rows), mh_stereo_winners, mh_stereo_agree, mh_stereo_refine.
Nothing is asserted on these numbers.  Prints one JSON line; profiles/stereo_timing.json is the record of a run.

    python tools/bench_stereo.py [--voxel-size 0.00125] [--rounds 5] [--out profiles/stereo_timing.json]"""
import argparse
import json
import os
import shutil
import sys
import tempfile

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from bench_carve import timed          # noqa: E402
from monohair_amd import gridviews, haircarve, hairstereo, synth_hair          # noqa: E402
from monohair_amd.camera import load_cam, parsing_camera          # noqa: E402
from monohair_amd.pmvo_utils import VOXEL_MIN, load_bust          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--voxel-size", type=float, default=haircarve.CARVE_VOXEL_SIZE)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the JSON line to this file")
    args = ap.parse_args()
    d = hairstereo.DEFAULTS
    data = tempfile.mkdtemp(prefix="bench_stereo_")
    try:
        base = synth_hair.write_case(data, "synthetic_hair", photo=True)
        images = os.path.join(base, "capture_images")
        camera = parsing_camera(load_cam(os.path.join(base, "ours", "cam_params.json")), images)
        masks = haircarve.load_masks(camera, os.path.join(base, "hair_mask"))
        gray = hairstereo.load_gray(camera, images)
        bv, bf, _ = load_bust(os.path.join(base, "ours", "bust_long_tsfm.obj"))
    finally:
        shutil.rmtree(data, ignore_errors=True)
    V, H, W = gray.shape
    pmvo = haircarve.mask_context(masks, camera, [H, W])
    dev = pmvo.device
    bust = gridviews.bust_planes(pmvo, (bv, bf))
    vmin, vs, dims = gridviews.grid(VOXEL_MIN, args.voxel_size, haircarve.carve_grid(args.voxel_size))
    flags = haircarve._inside_dev(pmvo, bust, vmin, vs, dims, 2, 0)
    nb = torch.from_numpy(hairstereo.neighbour_table(camera, d["neighbours"])).to(dev)
    cell = hairstereo.auto_cell(camera, vs, vmin, dims, (H, W))
    m255 = hairstereo.margin255(d["margin_vox"], vs)
    g = torch.from_numpy(gray).to(dev)
    out = dict(views=V, H=H, W=W, dims=[int(x) for x in dims], voxel_size=vs, cell=cell, radius=d["radius"],
               neighbours=d["neighbours"], keep=d["keep"], winners_form="one lane per candidate, every pair projected again")
    out["census"] = timed(lambda: hairstereo._census_dev(g, cell, d["radius"], dev), args.rounds)
    _, census = hairstereo._census_dev(g, cell, d["radius"], dev)
    out["compact"] = timed(lambda: hairstereo._candidates_dev(flags, dev), args.rounds)
    cand = hairstereo._candidates_dev(flags, dev)
    out["winners"] = timed(lambda: hairstereo._winners_dev(pmvo, bust, vmin, vs, dims, cand, census, nb, cell, d["radius"],
                                                           d["keep"]), args.rounds)
    keys = hairstereo._winners_dev(pmvo, bust, vmin, vs, dims, cand, census, nb, cell, d["radius"], d["keep"])
    out["agree"] = timed(lambda: hairstereo._agree_dev(pmvo, bust, vmin, vs, dims, flags, keys, cell, d["max_cost"], m255),
                         args.rounds)
    agree = hairstereo._agree_dev(pmvo, bust, vmin, vs, dims, flags, keys, cell, d["max_cost"], m255)
    out["refine"] = timed(lambda: hairstereo._refine_dev(pmvo, bust, vmin, vs, dims, flags, keys, agree, cell, d["max_cost"],
                                                         m255, d["min_agree"], d["min_through"]), args.rounds)
    refined, depth = hairstereo._refine_dev(pmvo, bust, vmin, vs, dims, flags, keys, agree, cell, d["max_cost"], m255,
                                            d["min_agree"], d["min_through"])
    out.update(n_inside=int(flags.sum(dtype=torch.int64).item()), n_candidates=int(cand.numel()),
               n_refined=int(refined.sum(dtype=torch.int64).item()), cells=int(depth.numel()),
               cells_with_key=int((keys != -1).sum().item()), cells_confirmed=int((depth != 255.0).sum().item()))
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
