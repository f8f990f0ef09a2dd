"""GPU: the hull mesh (csrc/haircarve.hip) on grids whose per-word counts do not fit one batch of mh_carve_scan_kernel.  The
kernel is one block of 1024 threads that walks the counts 1024 words (65 536 corners or voxels) at a time and carries the running
total from one batch into the next; on the grids of tests/test_hair_carve_gpu.py both scans end inside their first batch.  Here
the corner scan (int32) and the voxel scan (int64) cross one and two batch borders, end exactly on one and one word behind one,
with flags that put counts into every batch, into the first or the last batch alone, or one voxel into each.  Every mesh goes
through _check_flags of that file: both counts, vertices and faces bytewise against tests/hair_carve_np.py, guard rows, a guarded
scratch, check_mesh and the API twice."""
import numpy as np
import pytest

import hair_carve_np as R
from test_hair_carve_gpu import _check_flags

pytestmark = pytest.mark.gpu

BATCH = 1024 * 64          # the corners or voxels whose words make one batch of the scan
# dims -> (words of the voxel scan, words of the corner scan)
GRIDS = {
    "40x40x40": ((40, 40, 40), 1000, 1077),          # only the corner scan crosses a batch
    "64x32x32": ((64, 32, 32), 1024, 1107),          # the voxel scan ends exactly on a batch
    "41x41x39": ((41, 41, 39), 1025, 1103),          # one word into the second batch; both last words partial
    "64x64x33": ((64, 64, 33), 2112, 2245),          # three batches of both scans
}
PATTERNS = ["seeded", "full", "ends", "first_batch", "last_batch"]


def _words(dims):
    X, Y, Z = dims
    return -(-(X * Y * Z) // 64), -(-((X + 1) * (Y + 1) * (Z + 1)) // 64)


def _flags(dims, pattern):
    X, Y, Z = dims
    n = X * Y * Z
    lin = np.arange(n)
    if pattern == "seeded":
        density = 0.3 if n > 2 * BATCH else 0.5
        return (np.random.default_rng([29, X, Y, Z]).random(dims) < density).astype(np.uint8)
    if pattern == "full":
        return np.ones(dims, np.uint8)
    if pattern == "ends":          # two sparse totals carried through empty batches
        f = np.zeros(n, np.uint8)
        f[0] = f[n - 1] = 1
    elif pattern == "first_batch":
        f = (lin < BATCH).astype(np.uint8)
    elif pattern == "last_batch":
        f = (lin >= (_words(dims)[0] - 1) // 1024 * BATCH).astype(np.uint8)
    else:
        assert pattern == "one_per_batch"
        f = np.zeros(n, np.uint8)
        for b, offset in enumerate((12345, 1, 4000, 65535, 30000)[:-(-n // BATCH)]):
            f[min(b * BATCH + offset, n - 1)] = 1
    return f.reshape(dims)


def _loads(flags):
    """from the restatement alone: (the voxel words that hold an exposed face, the corner words that hold a used corner)"""
    X, Y, Z = flags.shape
    faces = R.exposed_faces(flags)
    vox = np.array([(x * Y + y) * Z + z for (x, y, z), _ in faces], np.int64)
    corners = np.array([[((x + di) * (Y + 1) + (y + dj)) * (Z + 1) + (z + dk) for di, dj, dk in R.CORNERS[d]]
                        for (x, y, z), d in faces], np.int64)
    return np.unique(vox // 64), np.unique(corners // 64)


def _run(grid, pattern):
    dims, wv, wc = GRIDS[grid]
    assert _words(dims) == (wv, wc)
    flags = _flags(dims, pattern)
    v, t = _check_flags(flags)
    return dims, wv, wc, flags, v, t


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("grid", sorted(GRIDS))
def test_mesh_scans_across_batches(grid, pattern):
    dims, wv, wc, flags, v, t = _run(grid, pattern)
    X, Y, Z = dims
    n = X * Y * Z
    if pattern in ("seeded", "full"):
        # the carry matters: every batch of either scan holds an exposed face or a used corner, and so does the last word
        vox_words, corner_words = _loads(flags)
        assert set(vox_words // 1024) == set(range(-(-wv // 1024))) and vox_words[-1] == wv - 1
        assert set(corner_words // 1024) == set(range(-(-wc // 1024))) and corner_words[-1] == wc - 1
    if pattern == "full":
        assert len(t) == 4 * (X * Y + Y * Z + X * Z)
        assert len(v) == (X + 1) * (Y + 1) * (Z + 1) - (X - 1) * (Y - 1) * (Z - 1)
        if grid == "64x64x33":
            assert (len(t), len(v)) == (33280, 16642)
    elif pattern == "ends":
        assert flags.reshape(-1)[[0, n - 1]].tolist() == [1, 1] and flags.sum() == 2 and len(v) == 16 and len(t) == 24
    elif pattern == "first_batch":
        assert int(flags.sum()) == min(n, BATCH) and len(t) > 0
    elif pattern == "last_batch":
        assert int(flags.sum()) == n - (wv - 1) // 1024 * BATCH and flags.reshape(-1)[-1] == 1 and len(t) > 0
    else:
        assert 0 < flags.sum() < n and len(t) > 0


def test_mesh_of_one_voxel_per_batch():
    dims, wv, wc, flags, v, t = _run("64x64x33", "one_per_batch")
    where = np.flatnonzero(flags.reshape(-1))
    assert (where // BATCH).tolist() == [0, 1, 2] == list(range(-(-wv // 1024)))
    assert len(v) == 24 and len(t) == 36
