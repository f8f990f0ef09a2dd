"""GPU: the scalp sampler (csrc/meshsample.hip: mh_tri_area64, mh_mesh_sample, driven by hairgrow.sample_scalp) against a
float64 numpy restatement written here from the kernel's specification: the triangle of every sample and both float32
outputs element for element."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
VMIN64 = np.array([-0.32, -0.32, -0.24], np.float32).astype(np.float64)
BUST = np.array([0.006, -1.644, 0.010])
HI = np.nextafter(1.0, 0.0)


def np_sample(v, vn, f, u, bust):
    """areas, bounds, triangle per sample, voxel-space points and normals (float32), operation by operation in float64"""
    n = u.shape[0]
    a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
    e, g = b - a, c - a
    x = e[:, 1] * g[:, 2] - e[:, 2] * g[:, 1]
    y = e[:, 2] * g[:, 0] - e[:, 0] * g[:, 2]
    z = e[:, 0] * g[:, 1] - e[:, 1] * g[:, 0]
    area = 0.5 * np.sqrt((x * x + y * y) + z * z)
    C = np.cumsum(area / area.sum())
    B = np.floor(n * C + 0.5).astype(np.int64)
    B[-1] = n
    tri = np.searchsorted(B, np.arange(n), side="right")          # the first triangle t with B[t] > i
    r1, r2 = np.sqrt(u[:, 0]), u[:, 1]
    wa, wb, wc = (1.0 - r1)[:, None], (r1 * (1.0 - r2))[:, None], (r1 * r2)[:, None]
    ft = f[tri]
    p = (wa * v[ft[:, 0]] + wb * v[ft[:, 1]]) + wc * v[ft[:, 2]]
    q = (wa * vn[ft[:, 0]] + wb * vn[ft[:, 1]]) + wc * vn[ft[:, 2]]
    p = p + bust
    p[:, 1:] *= -1
    p = (p - VMIN64) / 0.0025
    q = q / np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])[:, None]
    q[:, 1:] *= -1
    return area, B, tri, p.astype(np.float32), q.astype(np.float32)


def random_mesh(rng, nv, nf, zero_area_at=()):
    """a cloud of head size around where a scalp lies before bust_to_origin is added; normals of lengths 0.1 .. 5"""
    v = rng.normal(size=(nv, 3)) * 0.05 + np.array([0.0, 1.7, 0.0])
    vn = rng.normal(size=(nv, 3))
    vn *= (rng.uniform(0.1, 5.0, size=(nv, 1)) / np.linalg.norm(vn, axis=1, keepdims=True))
    f = np.stack([rng.permutation(nv)[:3] for _ in range(nf)]).astype(np.int64)
    for t in zero_area_at:
        f[t, 1] = f[t, 0]                                          # a repeated vertex: the cross product is exactly 0
    return v, f, vn


def check(v, f, vn, u, bust):
    from monohair_amd.hairgrow import sample_scalp

    n = u.shape[0]
    pts, nrm, last = sample_scalp(None, bust, n, device=DEV, mesh=(v, f, vn), uniforms=u, return_details=True)
    area, B, tri, p, q = np_sample(v, vn, f, u, np.asarray(bust, np.float64))
    assert pts.dtype.is_floating_point and pts.element_size() == 4 and tuple(pts.shape) == (n, 3) == tuple(nrm.shape)
    assert np.array_equal(last["area"], area)
    assert np.array_equal(last["bounds"], B)
    got_tri = last["triangle"].cpu().numpy()
    assert np.array_equal(got_tri, tri)
    assert np.array_equal(np.bincount(got_tri, minlength=len(f)), np.diff(np.concatenate([[0], B])))
    assert np.array_equal(pts.cpu().numpy(), p)
    assert np.array_equal(nrm.cpu().numpy(), q)
    return got_tri, area


def test_one_triangle_one_sample():
    v = np.array([[0.01, 1.70, 0.02], [0.05, 1.71, 0.00], [0.02, 1.75, 0.03]])
    vn = np.array([[0.0, 2.0, 0.5], [0.3, 1.0, 0.0], [0.0, 0.2, 0.1]])
    f = np.array([[0, 1, 2]])
    check(v, f, vn, np.array([[0.25, 0.75]]), BUST)
    check(v, f, vn, np.array([[0.0, 0.0]]), np.zeros(3))           # the sample is vertex a itself, no offset


@pytest.mark.parametrize("nf,n", [(40, 65), (40, 1000), (1000, 65)])
def test_sizes_off_the_wave_and_the_block(nf, n):
    rng = np.random.default_rng(100 + nf + n)
    v, f, vn = random_mesh(rng, 60 if nf == 40 else 400, nf)
    tri, _ = check(v, f, vn, rng.random((n, 2)), BUST)
    if nf == 1000:
        assert len(np.unique(tri)) <= 65 < nf                      # most triangles receive nothing


@pytest.mark.parametrize("where", ["middle", "end"])
@pytest.mark.parametrize("n", [65, 1000])
def test_zero_area_triangle_receives_nothing(where, n):
    rng = np.random.default_rng(7)
    t = 17 if where == "middle" else 39
    v, f, vn = random_mesh(rng, 60, 40, zero_area_at=(t,))
    tri, area = check(v, f, vn, rng.random((n, 2)), BUST)
    assert area[t] == 0.0 and (tri != t).all() and (area[np.arange(40) != t] > 0).all()


def test_uniforms_at_both_ends_of_their_range():
    rng = np.random.default_rng(3)
    v, f, vn = random_mesh(rng, 60, 40)
    u = rng.random((1000, 2))
    corners = np.array([[0.0, 0.0], [0.0, HI], [HI, 0.0], [HI, HI]])
    u[:4] = corners                                                # first block, first triangles
    u[500:504] = corners
    u[-4:] = corners                                               # last block, last triangle
    check(v, f, vn, u, BUST)
    check(v, f, vn, u, np.array([-0.11, 0.37, 0.05]))


def test_seeded_draw_from_an_obj_file_repeats(tmp_path):
    """through the file reader and the seed: the uniforms are np.random.default_rng(seed).random((n, 2))"""
    from monohair_amd.hairgrow import sample_scalp

    rng = np.random.default_rng(12)
    v, f, vn = random_mesh(rng, 30, 50)
    f[:10] = np.arange(30).reshape(10, 3)                          # every vertex in a face: every vertex gets its `vn`
    with open(tmp_path / "scalp.obj", "w") as fh:
        for p in v:
            fh.write("v %r %r %r\n" % tuple(float(x) for x in p))
        for p in vn:
            fh.write("vn %r %r %r\n" % tuple(float(x) for x in p))
        for t in f:
            fh.write("f %d//%d %d//%d %d//%d\n" % tuple(int(i) + 1 for i in np.repeat(t, 2)))
    assert np.isin(np.arange(30), f).all()
    a = sample_scalp(str(tmp_path / "scalp.obj"), BUST, 300, seed=5, device=DEV)
    b = sample_scalp(str(tmp_path / "scalp.obj"), BUST, 300, seed=5, device=DEV)
    c = sample_scalp(str(tmp_path / "scalp.obj"), BUST, 300, seed=6, device=DEV)
    _, _, _, p, q = np_sample(v, vn, f, np.random.default_rng(5).random((300, 2)), BUST)
    assert np.array_equal(a[0].cpu().numpy(), p) and np.array_equal(a[1].cpu().numpy(), q)
    assert all(np.array_equal(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(a, b))
    assert not np.array_equal(a[0].cpu().numpy(), c[0].cpu().numpy())
