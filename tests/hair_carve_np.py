"""The silhouette carve of include/mh_pmvo.h ("Silhouette carve") restated in numpy: what the HIP kernels of csrc/haircarve.hip
must equal on every quantity.  The votes are float32 comparisons on the oracle's projection of the float32 voxel centres, by
the view terms of tests/hair_fill_np.py (the abstention, `front` and `hair` are the same tests; the carve reads no depth map);
the mesh is a plain loop over the INSIDE voxels and the six directions with the corner table copied from the header.
tests/test_hair_carve_host.py holds this file to hand-computed cases."""
import numpy as np

import hair_fill_np as FILL

F = np.float32
centres, grid_voxels = FILL.centres, FILL.grid_voxels
DIRECTIONS = ((-1, 0, 0), (1, 0, 0), (0, -1, 0), (0, 1, 0), (0, 0, -1), (0, 0, 1))
# the four corners (di, dj, dk) of the face in each direction, in cyclic order
CORNERS = (((0, 0, 0), (0, 0, 1), (0, 1, 1), (0, 1, 0)), ((1, 0, 0), (1, 1, 0), (1, 1, 1), (1, 0, 1)),
           ((0, 0, 0), (1, 0, 0), (1, 0, 1), (0, 0, 1)), ((0, 1, 0), (0, 1, 1), (1, 1, 1), (1, 1, 0)),
           ((0, 0, 0), (0, 1, 0), (1, 1, 0), (1, 0, 0)), ((0, 0, 1), (1, 0, 1), (1, 1, 1), (0, 1, 1)))


# ------------------------------------------------------------------------------------------------- 1. votes
def votes(records, mask, bust, pts):
    """int32 [N,3] = n_in, n_free, n_miss over the views.  mask / bust: float32 [V,H,W]"""
    out = np.zeros((len(pts), 3), np.int32)
    nowhere = np.zeros(mask.shape[1:], F)      # (a depth plane for the term the carve does not have)
    for v in range(len(records)):
        inside, _, free, hair = FILL.view_terms(records[v], nowhere, mask[v], bust[v], pts)
        out[:, 0] += inside
        out[:, 1] += inside & free
        out[:, 2] += inside & free & ~hair
    return out


def inside_flags(counts, min_free=2, max_miss=0):
    c = np.asarray(counts).reshape(-1, 3)
    return ((c[:, 1] >= int(min_free)) & (c[:, 2] <= int(max_miss))).astype(np.uint8)


# ------------------------------------------------------------------------------------------------- 2. the mesh
def corner_position(corner, voxel_min, voxel_size):
    """float32 [3]: the world position of grid corner (i, j, k), float64 arithmetic rounded once"""
    m, vs = np.asarray(voxel_min, np.float64), np.float64(voxel_size)
    c = np.asarray(corner, np.float64) - 0.5
    return np.array([m[0] + c[0] * vs, -(m[1] + c[1] * vs), -(m[2] + c[2] * vs)]).astype(F)


def exposed_faces(flags):
    """[(voxel (x, y, z), direction index)] in the order of the rule"""
    f = np.asarray(flags) != 0
    X, Y, Z = f.shape
    out = []
    for x, y, z in np.argwhere(f).tolist():      # C order of [X,Y,Z]: ascending key
        for d, (dx, dy, dz) in enumerate(DIRECTIONS):
            nx, ny, nz = x + dx, y + dy, z + dz
            if not (0 <= nx < X and 0 <= ny < Y and 0 <= nz < Z) or not f[nx, ny, nz]:
                out.append(((x, y, z), d))
    return out


def mesh(flags, voxel_min, voxel_size):
    """-> (vertices float32 [Nv,3], faces int32 [Nt,3])"""
    X, Y, Z = np.asarray(flags).shape
    quads = []
    for (x, y, z), d in exposed_faces(flags):
        quads.append([((x + di) * (Y + 1) + (y + dj)) * (Z + 1) + (z + dk) for di, dj, dk in CORNERS[d]])
    quads = np.asarray(quads, np.int64).reshape(-1, 4)
    keys = np.unique(quads)                      # the used corners, ascending
    rank = np.searchsorted(keys, quads)
    faces = np.stack([rank[:, [0, 1, 2]], rank[:, [0, 2, 3]]], 1).reshape(-1, 3).astype(np.int32)
    ijk = np.stack([keys // ((Y + 1) * (Z + 1)), (keys // (Z + 1)) % (Y + 1), keys % (Z + 1)], 1).astype(np.float64) - 0.5
    m, vs = np.asarray(voxel_min, np.float64), np.float64(voxel_size)
    vertices = np.stack([m[0] + ijk[:, 0] * vs, -(m[1] + ijk[:, 1] * vs), -(m[2] + ijk[:, 2] * vs)], 1).astype(F)
    return vertices.reshape(-1, 3), faces


# ------------------------------------------------------------------------------------------------- what a closed mesh has
def signed_volume(vertices, faces):
    """float64: the sum over the triangles of a . (b x c) / 6 (positive for outward counter-clockwise faces)"""
    v = np.asarray(vertices, np.float64)
    a, b, c = v[faces[:, 0]], v[faces[:, 1]], v[faces[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def check_mesh(flags, vertices, faces, voxel_size):
    """asserts what the rule promises of any mesh (voxel_min and voxel_size dyadic, so that every figure is exact): two triangles
    per exposed face whose normals point from the INSIDE voxel to the neighbour in world coordinates (y and z negated), the
    signed volume, closedness"""
    want = exposed_faces(flags)
    assert len(faces) == 2 * len(want)
    v = np.asarray(vertices, np.float64)
    if len(faces):
        n = np.cross(v[faces[:, 1]] - v[faces[:, 0]], v[faces[:, 2]] - v[faces[:, 0]])
        world = np.array([(dx, -dy, -dz) for dx, dy, dz in DIRECTIONS], np.float64)
        out = np.repeat(world[[d for _, d in want]], 2, axis=0) * (np.float64(voxel_size) ** 2)
        assert np.array_equal(n, out)
    assert signed_volume(vertices, faces) == float(np.count_nonzero(flags)) * np.float64(voxel_size) ** 3
    assert odd_edges(faces) == 0


def odd_edges(faces):
    """the number of undirected edges used by an odd number of triangles (0 for a closed surface)"""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if not len(f):
        return 0
    e = np.sort(np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]]), axis=1)
    _, n = np.unique(e, axis=0, return_counts=True)
    return int((n % 2 == 1).sum())
