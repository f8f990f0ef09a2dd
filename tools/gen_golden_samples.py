"""tests/golden/pmvo_samples.npz: the reference at sample counts other than 90.

The reference exposes the number of depth samples of its search as the default argument of PMVO.sample_next_3d_pos
(/root/reference/PMVO.py:263); forward() calls it without one (:54).  This generator sets that default to S in
{1, 16, 60, 100, 102} and records, for the points of two committed scenes, the reference's own forward() (PMVO.py:39-78) and,
from a direct call sample_next_3d_pos(points, base_view_indexs[0], S), the samples of the first 16 points.  With S = 1 it also
hands every fifth point to forward() ALONE: a batch of one candidate in all, whose [V, 1] tensors the reference projects and
sums in forms of their own (csrc/pmvo_search.hip: mh_search_one_column_kernel).  Only outputs are stored.  The offsets in the
file are NOT a recording: the reference forms them inside sample_next_3d_pos, and monohair_amd.pmvo.depth_offsets -- the
project's one restatement of those lines -- writes them here, so that a later change of that function shows; what pins them
to the reference is the recorded samples.

1: a search of one sample per rank; 16: fewer samples than ATen's 32 trailing columns; 60 and 100: the arange pieces have
exact lengths; 102: num_sample / 4 is not an integer.

The file is written with fixed zip time stamps, so that a second run reproduces it byte for byte.

    python tools/gen_golden_samples.py          (build container only: imports /root/reference)
"""
import io
import os
import sys
import zipfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(1, ROOT)
sys.path.insert(2, os.path.join(ROOT, "tests"))

import gen_golden as G  # noqa: E402
from ref_import import import_reference  # noqa: E402
from monohair_amd import synth  # noqa: E402
from monohair_amd.pmvo import depth_offsets  # noqa: E402

SAMPLE_COUNTS = (1, 16, 60, 100, 102)
THREADS = 8
HEAD = 16


def save_npz(path, arrays):
    """np.savez_compressed with a fixed time stamp per member (numpy stamps the members with the current time)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for key, val in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(val), allow_pickle=False)
            info = zipfile.ZipInfo(key + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main():
    from conftest import golden_scene, load_golden

    os.chdir("/tmp")
    torch.set_num_threads(THREADS)
    R = import_reference(gabor=False)
    cls = R["PMVO"].PMVO
    default = cls.sample_next_3d_pos.__defaults__
    out = {}
    try:
        for name in ("pmvo_small", "pmvo_quant"):
            case = G.PMVO_CASES[name]
            meta, z = load_golden(name)
            scene = golden_scene(meta)
            cams = G.ref_cameras(R, scene)
            depths, Ori, Conf, masks = synth.scene_to_reference_dicts(scene)
            pm = cls(cams, depths, Ori, Conf, masks, device="cpu", image_size=[case["H"], case["W"]],
                     patch_size=case["patch"], visible_threshold=case["vis_thr"], conf_threshold=case["thr"])
            pts = torch.from_numpy(z["points"]).type(torch.float)
            for S in SAMPLE_COUNTS:
                cls.sample_next_3d_pos.__defaults__ = (S,)
                _, so, ml, hc = pm.forward(z["points"])
                bidx, _ = pm.Find_max_conf_from_visible_view()      # (forward left the state of these points)
                assert np.array_equal(bidx.numpy(), z["base_idx"])
                samples, surface = pm.sample_next_3d_pos(pts, bidx[0], S)
                assert torch.equal(surface, pts) and samples.shape == (len(pts), S, 3)
                tag = "%s__S%d__" % (name, S)
                out.update({tag + "ori": so.numpy(), tag + "loss": ml.numpy(), tag + "hc": hc.numpy(),
                            tag + "samples": samples[:HEAD].numpy()})
                n90 = int(((ml.numpy() == z["fwd_loss"]) | (np.isnan(ml.numpy()) & np.isnan(z["fwd_loss"]))).sum())
                print("%-12s S = %3d: %d of %d finite losses, %d rows equal to S = 90" % (
                    name, S, int(np.isfinite(ml.numpy()).sum()), len(pts), n90))
            # S = 1, every fifth point alone: N * S = 1
            cls.sample_next_3d_pos.__defaults__ = (1,)
            pick = np.arange(0, len(pts), 5)
            alone = [pm.forward(z["points"][n:n + 1])[1:] for n in pick]
            tag = name + "__S1__alone_"
            out.update({tag + "pick": pick, tag + "ori": np.concatenate([a[0].numpy() for a in alone]),
                        tag + "loss": np.concatenate([a[1].numpy() for a in alone]),
                        tag + "hc": np.concatenate([a[2].numpy() for a in alone])})
            same = (out[tag + "loss"] == out[name + "__S1__loss"][pick]) | np.isnan(out[tag + "loss"])
            print("%-12s S =   1: %d points alone, %d finite, %d differ from their row in the batch" % (
                name, len(pick), int(np.isfinite(out[tag + "loss"]).sum()), int((~same).sum())))
    finally:
        cls.sample_next_3d_pos.__defaults__ = default
    for S in SAMPLE_COUNTS:        # (monohair_amd.pmvo.depth_offsets: see above)
        out["offsets__S%d" % S] = depth_offsets(S)
    meta = dict(torch=torch.__version__, threads=torch.get_num_threads(), sample_counts=SAMPLE_COUNTS, head=HEAD,
                what="the reference's forward() with sample_next_3d_pos.__defaults__ = (S,)")
    save_npz(os.path.join(G.OUT, "pmvo_samples.npz"), dict(meta=np.array(repr(meta)), **out))
    print("pmvo_samples.npz written")


if __name__ == "__main__":
    main()
