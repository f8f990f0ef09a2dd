#!/usr/bin/env python
"""Expected fall of the search's SQ_INSTS_VALU per launch with mh_key_walk (csrc/mh_key_blocks.h) from the list lengths of the bench
chunks -- pm.search_work as bench.py's kernel_rooflines reads it, one call per chunk -- and the per-path counts of
profiles/search_walk.txt (SAVE: VALU instructions a (wave, view) visit of a 49-tap list saves at KA item slices).  Prints bench.py's
result line, then the figures.
    python tools/exp_walk_valu.py"""
import os, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
import bench
from monohair_amd.pmvo import PMVO
SAVE = {4: 57, 3: 46, 2: 35, 1: 24, 0: 0}
rows = []
orig = PMVO.search_work
def wrapped(self, N, bval):
    cnt, nvalid = orig(self, N, bval)
    c, nv = cnt.cpu().numpy().astype(np.int64), nvalid.cpu().numpy().astype(np.int64)
    V = c.shape[0]
    n49 = (c == 49).sum(0)
    nact = nv * 90
    nrest = nact & 63
    nleft = np.where((nrest <= 16) & (nrest * V <= 544), nrest, 0)
    per = np.zeros_like(nact)
    for w in range(4):
        ka = sum(((j * 256 + 64 * w) < (nact - nleft)).astype(np.int64) for j in range(4))
        per += np.vectorize(SAVE.get)(ka)
    rows.append(dict(saved=int((n49 * per).sum()), lists=int((c > 0).sum()), lists49=int((c == 49).sum()), taps=int(c.sum()),
                     ranks=np.bincount(nv, minlength=11).tolist()))
    return cnt, nvalid
PMVO.search_work = wrapped
sys.argv = ["bench.py", "--gpus", "1", "--steps", "4", "--warmup", "1", "--no-cpu", "--no-secondary", "--streams", "1"]
bench.main()
print("chunks read: %d" % len(rows))
for k in ("saved", "lists", "lists49", "taps"):
    v = [r[k] for r in rows]
    print("%s per launch: mean %.1f min %d max %d" % (k, np.mean(v), min(v), max(v)))
print("share of 49-tap lists: %.4f" % (sum(r["lists49"] for r in rows) / sum(r["lists"] for r in rows)))
print("points by usable ranks 0..10 (all chunks): %s" % np.sum([r["ranks"] for r in rows], axis=0).tolist())
