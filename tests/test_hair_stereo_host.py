"""CPU-only: the numpy restatement of the photo-consistent carve (tests/hair_stereo_np.py) held to the hand-computed values of
tests/hair_stereo_cases.py -- reduced images and census codes with windows clamped at all four borders, winner keys (padded
neighbour rows, fewer than `keep` neighbours, equal costs, flat images, no candidate), agreement and refinement on their bounds
-- and, on the textured sphere, shown to do what the rule is for: against a control whose views share no texture it confirms
more cells, its confirmed winners lie nearer the analytic depth, and it removes more of a hand-made spike than of the sphere.
The sphere's assertions fix no figures; the four shares are printed.  Neighbour tables of four and seven columns on the hand
cameras, with keys worked out by hand for keep up to 7, and tables of 3, 5 and 8 shuffled columns on the sphere; a thirteenth view
inside the sphere's grid, with voxel centres on its plane z' = 0 and behind it.  The fixtures `wide` and `inside` hold what the
GPU tests compare the kernels with."""
import numpy as np
import pytest

import hair_carve_np as CARVE
import hair_fill_cases as C
import hair_stereo_cases as S
import hair_stereo_np as R

F = np.float32


def records(cams):
    from monohair_amd.camera import camera_records, cameras_from_list

    return camera_records(cameras_from_list(cams))


def hand_terms(scene):
    return R.Terms(records(C.hand_cameras()), scene["mask"], scene["bust"], C.HAND_VMIN, C.HAND_VS, C.HAND_DIMS, scene["cell"])


# ------------------------------------------------------------------------------------------------- census
def test_reduced_image_and_census_codes_by_hand():
    gray, reduced, want = S.census_image()
    g = R.reduce_gray(gray, 2)
    assert g.dtype == np.uint8 and np.array_equal(g, reduced)
    code = R.census(g, 1)
    assert code.dtype == np.uint64 and code.shape == (1, 3, 4)
    for (i, j), c in want.items():
        assert code[0, i, j] == c, (i, j, bin(int(code[0, i, j])), bin(int(c)))
    # cell 1 leaves the image as it is; a flat image has the code 0 everywhere; radius 3 uses 48 bits
    assert np.array_equal(R.reduce_gray(gray, 1), gray)
    assert not R.census(np.full((2, 4, 5), 9, np.uint8), 3).any()
    ramp = np.arange(49, dtype=np.uint8).reshape(1, 7, 7)
    assert int(R.census(ramp, 3)[0, 3, 3]) == (1 << 24) - 1
    assert int(R.census(ramp, 3)[0, 6, 6]) == (1 << 48) - 1 - sum(1 << b for b in _self_bits(3))
    assert R.popcount(np.array([0, 1, 0xFF, 0xFFFFFFFFFFFFFFFF], np.uint64)).tolist() == [0, 1, 8, 64]


def _self_bits(radius):
    """the bits of the lower right corner pixel whose clamped neighbour lies in its own row or column or is itself: on a ramp
    that rises along rows and columns those neighbours are not smaller only where they clamp onto the pixel itself"""
    bits, b = [], 0
    for dy in range(-radius, radius + 1):
        for dx in range(-radius, radius + 1):
            if dy == 0 and dx == 0:
                continue
            if dy >= 0 and dx >= 0:          # clamps onto the corner pixel itself: equal, not smaller
                bits.append(b)
            b += 1
    return bits


# ------------------------------------------------------------------------------------------------- the hand-made scenes
def test_terms_of_the_hand_cameras():
    scene = S.hand_scene_one()
    t = hand_terms(scene)
    a, b = S.idx(3, 5, 0), S.idx(3, 5, 1)
    assert t.z255[0, a] == S.Z0 and t.z255[0, b] == S.Z1 and t.cell[0, a] == t.cell[0, b] == 5 * 8 + 3
    assert t.takes[:C.N_A, a].all() and not t.seen[C.N_A:, a].any()
    c0, c1 = S.idx(4, 4, 0), S.idx(4, 4, 1)
    assert t.seen[:, c0].all() and t.seen[:, c1].all() and t.cell[5, c0] == t.cell[5, c1] == 4 * 8 + 4
    assert t.z255[5, c0] == F(255.0 / 256.0) and F(t.z255[5, c1] - t.z255[5, c0]) == S.GAP
    assert not t.takes[2, S.idx(1, 6, 0)] and t.free[2, S.idx(1, 6, 0)]


@pytest.mark.parametrize("keep", [1, 2])
def test_winner_keys_by_hand(keep):
    scene = S.hand_scene_one()
    t = hand_terms(scene)
    codes = R.census(R.reduce_gray(scene["gray"], 1), 1)
    assert codes[0, 2, 2] == 0xFF and codes[2, 2, 2] == 0xFF and codes[1, 2, 2] == 0 and codes[3, 5, 5] == 7 and \
        codes[3, 3, 3] == 128 and codes[3, 4, 4] == 0
    keys = R.winners(t, codes, S.HAND_NB, 1, keep, np.flatnonzero(scene["flags"].reshape(-1)))
    assert keys.dtype == np.uint64 and keys.shape == (8, 8, 8)
    for (r, i, j), want in scene["keys"][keep].items():
        assert keys[r, i, j] == want, (r, i, j, hex(int(keys[r, i, j])), hex(int(want)))
    assert (keys[4] == S.NONE).all() and (keys[5:].reshape(3, -1) != S.NONE).sum(1).tolist() == ([1, 1, 1] if keep == 1 else
                                                                                                  [1, 0, 1])
    # two voxels of one cell with equal cost: the lower index, layer 0, wins every cell where it is a candidate
    won = keys[keys != S.NONE] & np.uint64(0xFFFFFFFF)
    assert (won % np.uint64(2) == 0).sum() == len(won) - (keys[:4, 6, 3] != S.NONE).sum()
    # flat images: every census 0, every cost 0
    flat = R.census(R.reduce_gray(np.full_like(scene["gray"], 77), 1), 1)
    kf = R.winners(t, flat, S.HAND_NB, 1, keep, np.flatnonzero(scene["flags"].reshape(-1)))
    assert not flat.any() and np.array_equal(kf == S.NONE, keys == S.NONE) and (kf[kf != S.NONE] >> np.uint64(32) == 0).all()
    # no candidate at all, and candidates outside the grid
    for cand in (np.zeros(0, np.int64), np.array([-1, 128, 1 << 30])):
        assert (R.winners(t, codes, S.HAND_NB, 1, keep, cand) == S.NONE).all()


@pytest.mark.parametrize("table,keep", [("keys4", 1), ("keys4", 2), ("keys4", 3), ("keys4", 4), ("keys7", 4), ("keys7", 7)])
def test_winner_keys_of_wide_tables_by_hand(table, keep):
    """tables of four and seven columns, keep 3, 4 and 7: distances that arrive ascending, descending and with an equal pair,
    exactly keep and keep - 1 neighbours taking part, a view named twice"""
    scene = S.hand_scene_wide()
    t = hand_terms(scene)
    codes = R.census(R.reduce_gray(scene["gray"], 1), 1)
    for (v, i, j), c in scene["codes"].items():
        assert codes[v, i, j] == c, (v, i, j, hex(int(codes[v, i, j])))
    nb = S.HAND_NB4 if table == "keys4" else S.HAND_NB7
    # the tables are what the docstring of the scene says of them
    assert all(sorted(S.HAND_NB4[r]) == sorted(set(range(C.N_A)) - {r}) for r in range(C.N_A))
    assert (S.HAND_NB4[C.N_A:] == -1).sum(1).tolist() == [2, 2, 1] and S.HAND_NB4[7].tolist().count(5) == 2
    assert all(sorted(S.HAND_NB7[r]) == sorted(set(range(8)) - {r}) for r in range(8))
    keys = R.winners(t, codes, nb, 1, keep, np.flatnonzero(scene["flags"].reshape(-1)))
    for (r, i, j), want in scene[table][keep].items():
        assert keys[r, i, j] == want, (r, i, j, hex(int(keys[r, i, j])), hex(int(want)))
    # the distances of P in the order of the rows of NB4, as the scene states them
    if table == "keys4" and keep == 4:
        arrive = [[int(R.popcount(codes[r, 1, 5] ^ codes[n, 1, 5])[0]) for n in S.HAND_NB4[r]] for r in range(C.N_A)]
        assert arrive == [[1, 3, 6, 8], [7, 1, 5, 2], [3, 2, 3, 5], [6, 5, 3, 2], [8, 7, 5, 2]]


def test_agreement_by_hand():
    scene = S.hand_scene_one()
    t = hand_terms(scene)
    codes = R.census(R.reduce_gray(scene["gray"], 1), 1)
    cand = np.flatnonzero(scene["flags"].reshape(-1))
    keys = {k: R.winners(t, codes, S.HAND_NB, 1, k, cand) for k in (1, 2)}
    for (keep, max_cost, m255), want in scene["agree"].items():
        a = R.agree(t, scene["flags"], keys[keep], max_cost, m255)
        assert a.dtype == np.int32 and a.shape == (128,)
        for (x, y, z), n in want.items():
            assert a[S.idx(x, y, z)] == n, (keep, max_cost, float(m255), (x, y, z), int(a[S.idx(x, y, z)]), n)
    none = R.agree(t, np.zeros_like(scene["flags"]), keys[1], 1024, S.GAP)
    assert not none.any()


def test_refinement_by_hand():
    scene = S.hand_scene_two()
    t = hand_terms(scene)
    codes = R.census(R.reduce_gray(scene["gray"], 2), 1)
    assert codes.shape == (8, 4, 4) and not codes.any()
    flags = scene["flags"]
    keys = R.winners(t, codes, S.HAND_NB, 1, 2, np.flatnonzero(flags.reshape(-1)))
    for (r, i, j), want in scene["keys"].items():
        assert keys[r, i, j] == want, (r, i, j)
    w, star, u = (S.idx(*scene[k]) for k in ("w", "star", "u"))
    m = scene["margins"]
    a = R.agree(t, flags, keys, 128, m["zero"])
    # w takes part nowhere; the winner agrees with itself in the three views that hold keys; u is a layer in front of it
    assert a[w] == 0 and a[star] == 3 and a[u] == 0 and a[S.idx(6, 6, 0)] == 3 and a[S.idx(6, 6, 1)] == 0
    assert R.agree(t, flags, keys, 128, m["on"])[u] == 3
    # through: w and u lie in front of the confirmed winner in views 0, 2 and 3 unless the margin reaches the gap
    for name, n in (("zero", 3), ("sum_below", 3), ("rounds_to_on", 0), ("on", 0), ("sum_above", 0)):
        th = R.through(t, flags, keys, a, 128, m[name], 3)
        assert th[w] == n and th[u] == n and th[star] == 0 and th[S.idx(6, 6, 0)] == 0 and th[S.idx(6, 6, 1)] == 0, name
    # agree exactly on min_agree confirms, one more does not; through exactly on min_through removes, one more does not
    for min_agree, min_through, gone in ((3, 3, True), (4, 3, False), (3, 4, False), (3, 1, True), (1, 3, True)):
        refined, depth = R.refine(t, flags, keys, a, 128, m["zero"], min_agree, min_through)
        assert refined.dtype == np.uint8 and depth.dtype == F and depth.shape == (8, 4, 4)
        assert refined[w] == refined[u] == (0 if gone else 1) and refined[star] == 1, (min_agree, min_through)
        assert refined.sum() == (3 if gone else 5)
        for r in range(8):
            on = r in (0, 2, 3) and min_agree <= 3
            assert depth[r, 0, 0] == (S.Z1 if on else F(255.0)) and depth[r, 3, 3] == (S.Z0 if on else F(255.0))
        assert (depth != 255.0).sum() == (6 if min_agree <= 3 else 0)
    # a cost above max_cost confirms nothing (every cost is 0 here: max_cost 0 still does)
    assert R.refine(t, flags, keys, a, 0, m["zero"], 3, 3)[0].sum() == 3
    empty = np.zeros_like(flags)
    k0 = R.winners(t, codes, S.HAND_NB, 1, 2, np.zeros(0, np.int64))
    r0, d0 = R.refine(t, empty, k0, R.agree(t, empty, k0, 128, m["zero"]), 128, m["zero"], 3, 3)
    assert not r0.any() and (d0 == 255.0).all()


def test_neighbour_table_and_auto_cell():
    from monohair_amd import hairstereo
    from monohair_amd.camera import cameras_from_list

    cams = cameras_from_list(C.hand_cameras())
    centres = hairstereo.camera_centres(cams)
    assert np.array_equal(centres[:C.N_A], [[0, 0, 1]] * C.N_A) and np.array_equal(centres[C.N_A:], [[0, 0, 0.5 + 1 / 128]] * C.N_B)
    # equal distances: the lower view index first; the view itself never
    nb = hairstereo.neighbour_table(cams, 3)
    assert nb.dtype == np.int32 and nb.tolist() == [[1, 2, 3], [0, 2, 3], [0, 1, 3], [0, 1, 2], [0, 1, 2], [6, 7, 0], [5, 7, 0],
                                                    [5, 6, 0]]
    assert hairstereo.neighbour_table(cams, 8)[:, 7].tolist() == [-1] * 8          # seven other views: padded
    ring = hairstereo.neighbour_table(cameras_from_list(S.sphere_cameras()), 2)
    assert np.array_equal(np.sort(ring, 1), np.sort(S.sphere_neighbours(2), 1))
    for k in (0, 9):
        with pytest.raises(ValueError):
            hairstereo.neighbour_table(cams, k)
    # camera A, focal 2 over 8 pixels, sees the grid's centre (0.5 - 1/32 below it ... at depth 0.53125): a voxel of 1/16 covers
    # (1/16) * 2 * 8 / (2 * 0.53125) = 0.94 pixels; camera B at depth 0.0390625: 12.8 pixels
    assert hairstereo.auto_cell(dict(list(cams.items())[:C.N_A]), C.HAND_VS, C.HAND_VMIN, C.HAND_DIMS, (8, 8)) == 1
    assert hairstereo.auto_cell(cams, C.HAND_VS, C.HAND_VMIN, C.HAND_DIMS, (8, 8)) == 13
    assert hairstereo.margin255(2.0, 1.0 / 128.0) == F(2.0 / 128.0 / 2.0 * 255.0)


# ------------------------------------------------------------------------------------------------- the textured sphere
SPHERE = dict(keep=2, max_cost=128, margin_vox=2.0, min_agree=3, min_through=2)
M255 = F(SPHERE["margin_vox"] * S.SPHERE_VS / 2.0 * 255.0)


@pytest.fixture(scope="module")
def sphere():
    """the restatement on the scene and on the control, for the hull and for the hull with the spike, computed once"""
    rec = records(S.sphere_cameras())
    nb = S.sphere_neighbours(2)
    out = {}
    for control in (False, True):
        gray, mask, z255 = S.sphere_views(control)
        bust = np.full(mask.shape, 255.0, F)
        pts = CARVE.centres(CARVE.grid_voxels(S.SPHERE_DIMS), S.SPHERE_VMIN, S.SPHERE_VS)
        hull = CARVE.inside_flags(CARVE.votes(rec, mask, bust, pts)).reshape(S.SPHERE_DIMS)
        spike = S.spike_voxels() & (hull == 0)
        for name, flags in (("hull", hull), ("spike", hull | spike.astype(np.uint8))):
            out[(control, name)] = R.stereo(rec, gray, mask, bust, S.SPHERE_VMIN, S.SPHERE_VS, S.SPHERE_DIMS, flags, nb,
                                            S.SPHERE_CELL, S.SPHERE_RADIUS, SPHERE["keep"], SPHERE["max_cost"], M255,
                                            SPHERE["min_agree"], SPHERE["min_through"])
            out[(control, name)].update(flags=flags, gray=gray, mask=mask, bust=bust, spike=spike, z255=z255)
    out["records"], out["neighbours"] = rec, nb
    return out


def analytic_cells(z255, cell):
    """the analytic depth per cell: the mean over the pixels of the block that see the sphere (NaN where none does)"""
    V, H, W = z255.shape
    Hc, Wc = -(-H // cell), -(-W // cell)
    out = np.full((V, Hc, Wc), np.nan)
    for i in range(Hc):
        for j in range(Wc):
            b = z255[:, i * cell:(i + 1) * cell, j * cell:(j + 1) * cell].reshape(V, -1).astype(np.float64)
            hit = b != 255.0
            n = hit.sum(1)
            out[:, i, j] = np.where(n > 0, (b * hit).sum(1) / np.maximum(n, 1), np.nan)
    return out


def shares(run):
    depth, truth = run["depth"], analytic_cells(run["z255"], S.SPHERE_CELL)
    confirmed = depth != 255.0
    with np.errstate(invalid="ignore"):
        near = confirmed & (np.abs(depth - truth) <= M255)
    return int(confirmed.sum()), float(near.sum()) / max(1, int(confirmed.sum()))


def test_the_rule_separates_the_scene_from_the_control(sphere):
    scene, control = sphere[(False, "hull")], sphere[(True, "hull")]
    assert scene["flags"].any() and np.array_equal(scene["flags"], control["flags"])          # the same silhouettes
    n_scene, near_scene = shares(scene)
    n_control, near_control = shares(control)
    print("confirmed cells: scene %d, control %d; within the margin of the analytic depth: scene %.4f, control %.4f"
          % (n_scene, n_control, near_scene, near_control))
    assert n_scene > 0 and n_control < n_scene
    assert near_scene > near_control


def test_the_spike_goes_before_the_sphere(sphere):
    run = sphere[(False, "spike")]
    flags, refined, spike = run["flags"].reshape(-1) != 0, run["refined"] != 0, run["spike"].reshape(-1)
    inside = (np.linalg.norm(S.sphere_world(), axis=-1) <= S.SPHERE_R).reshape(-1) & flags
    assert spike.sum() >= 4 and inside.sum() > 1000 and not (refined & ~flags).any()
    gone_spike = float((spike & ~refined).sum()) / spike.sum()
    gone_sphere = float((inside & ~refined).sum()) / inside.sum()
    print("removed: %.4f of the spike's %d voxels, %.4f of the sphere's own %d voxels"
          % (gone_spike, int(spike.sum()), gone_sphere, int(inside.sum())))
    assert gone_spike > gone_sphere


# ------------------------------------------------------------------------------------------------- tables of 3 to 8 columns
WIDE = [(K, keep) for K in (3, 5, 8) for keep in sorted({1, 3, K - 1, K})]
# the largest cost of a valid key per keep (the cost of a view grows with the number of distances it adds up): each leaves at
# least 300 cells valid and some not, which the test asserts of the restatement
WIDE_MAX_COST = {1: 64, 2: 64, 3: 96, 4: 96, 5: 128, 7: 192, 8: 192}


def stages(t, codes, flags, nb, radius, keep, max_cost, m255, min_agree, min_through):
    """the restatement's four stages on terms and census codes made once"""
    keys = R.winners(t, codes, nb, radius, keep, np.flatnonzero(np.asarray(flags).reshape(-1) != 0))
    a = R.agree(t, flags, keys, max_cost, m255)
    refined, depth = R.refine(t, flags, keys, a, max_cost, m255, min_agree, min_through)
    return dict(keys=keys, agree=a, refined=refined, depth=depth)


@pytest.fixture(scope="module")
def wide(sphere):
    """the restatement on the sphere's hull under the tables of S.sphere_table, computed once -> {(K, keep): dict(nb, max_cost,
    keys, agree, refined, depth)}"""
    run = sphere[(False, "hull")]
    out = {}
    for K, keep in WIDE:
        nb = S.sphere_table(K, keep)
        out[(K, keep)] = stages(run["terms"], run["census"], run["flags"], nb, S.SPHERE_RADIUS, keep, WIDE_MAX_COST[keep], M255,
                                SPHERE["min_agree"], SPHERE["min_through"])
        out[(K, keep)].update(nb=nb, max_cost=WIDE_MAX_COST[keep])
    return out


def insertion_positions(t, codes, row, r, cand):
    """int64 [8]: how often a distance of view r's candidates, arriving in the order of its neighbour row, has k of the earlier
    ones at or below it, k = 0..7 -- the slot of the ascending list it goes to, behind its equals"""
    codes = np.asarray(codes, np.uint64).reshape(t.V, -1)
    mine = codes[r][t.cell[r][cand]]
    earlier, count = [], np.zeros(8, np.int64)
    for n in row:
        if n < 0 or n == r:
            continue
        d, takes = R.popcount(mine ^ codes[n][t.cell[n][cand]]), t.takes[n][cand]
        pos = sum(((e_takes & (e_d <= d)).astype(np.int64) for e_d, e_takes in earlier), np.zeros(len(cand), np.int64))
        count += np.bincount(pos[takes & t.takes[r][cand]], minlength=8)
        earlier.append((d, takes))
    return count


def wide_conditions(run, w, K, keep):
    """what the restatement alone says of a table of S.sphere_table and its keys, for the tests on either side: the columns are
    out of the order of distance, one row has exactly keep entries and one keep - 1, at least 1 000 cells have a key, max_cost
    leaves at least 300 of them valid and some not; at K = keep = 8 the distances of one view take every slot of the list"""
    nb = w["nb"]
    assert nb.shape == (S.SPHERE_V, K) and np.array_equal(np.sort(nb[0]), np.sort(S.sphere_neighbours(K)[0]))
    assert (nb[3] >= 0).sum() == keep and (nb[8] >= 0).sum() == keep - 1 and ((nb >= 0).sum(1) == K).sum() >= S.SPHERE_V - 2
    assert any(not np.array_equal(nb[r], S.sphere_neighbours(K)[r]) for r in range(S.SPHERE_V))
    has = w["keys"] != S.NONE
    assert has.sum() >= 1000 and not has[8].any() and has[3].any()
    valid, _ = R.valid_keys(run["terms"], w["keys"], w["max_cost"])
    assert 300 <= valid.sum() < has.sum()
    if K == 8 and keep == 8:
        cand = np.flatnonzero(run["flags"].reshape(-1))[:2000]
        count = insertion_positions(run["terms"], run["census"], nb[0], 0, cand)
        print("insertion positions 0..7 of view 0 over %d candidates: %s" % (len(cand), count.tolist()))
        assert (count > 0).all()


@pytest.mark.parametrize("K,keep", WIDE)
def test_wide_tables_on_the_sphere(sphere, wide, K, keep):
    wide_conditions(sphere[(False, "hull")], wide[(K, keep)], K, keep)


# ------------------------------------------------------------------------------------------------- a view inside the grid
INSIDE_KEEPS = (2, 3)


@pytest.fixture(scope="module")
def inside():
    """the sphere's twelve views and the thirteenth inside the grid (S.inside_cameras): the restatement's votes, the hull they
    give, and the stereo stages on that hull under S.inside_table"""
    rec = records(S.inside_cameras())
    gray, mask = S.inside_views()
    bust = np.full(mask.shape, 255.0, F)
    pts = CARVE.centres(CARVE.grid_voxels(S.SPHERE_DIMS), S.SPHERE_VMIN, S.SPHERE_VS)
    votes = CARVE.votes(rec, mask, bust, pts)
    flags = CARVE.inside_flags(votes).reshape(S.SPHERE_DIMS)
    t = R.Terms(rec, mask, bust, S.SPHERE_VMIN, S.SPHERE_VS, S.SPHERE_DIMS, S.SPHERE_CELL)
    codes = R.census(R.reduce_gray(gray, S.SPHERE_CELL), S.SPHERE_RADIUS)
    nb = S.inside_table()
    runs = {keep: stages(t, codes, flags, nb, S.SPHERE_RADIUS, keep, SPHERE["max_cost"], M255, SPHERE["min_agree"],
                         SPHERE["min_through"]) for keep in INSIDE_KEEPS}
    return dict(records=rec, gray=gray, mask=mask, bust=bust, pts=pts, votes=votes, flags=flags, terms=t, nb=nb, runs=runs)


def test_view_inside_the_grid(inside):
    import oracle

    v = S.INSIDE_VIEW
    H = W = S.SPHERE_HW
    batch = np.concatenate([inside["pts"], np.zeros((1, 3), F)])          # (as view_terms projects: not a point alone)
    _, zp, oob, _ = (a[:-1] for a in oracle.project_points(inside["records"][v], batch, H, W))
    assert (zp == 0).sum() == 1024 and (zp < 0).sum() == 15360 and (zp > 0).sum() == 16384
    # behind the view and with an unclamped pixel inside the image: the sign of z' alone makes the view abstain
    assert ((zp < 0) & ~oob).sum() >= 1000
    t = inside["terms"]
    assert not t.seen[v][~(zp > 0)].any() and t.seen[v].sum() == 1496 and np.array_equal(t.seen[v], ~oob & (zp > 0))
    own = CARVE.votes(inside["records"][v:], inside["mask"][v:], inside["bust"][v:], inside["pts"])
    assert own[:, 0].sum() == 1496 and np.array_equal(own[:, 0], own[:, 1]) and not own[:, 2].any()
    # the hull holds candidates on the plane z' = 0, behind the view inside its image, and in front of it
    f = inside["flags"].reshape(-1) != 0
    assert (f & (zp == 0)).sum() > 100 and (f & (zp < 0) & ~oob).sum() > 100 and (f & t.takes[v]).sum() > 100
    nb = inside["nb"]
    assert nb.shape == (13, 3) and v in nb[0] and v in nb[6] and (nb[v] >= 0).all() and (nb[:v, :2] == S.sphere_neighbours(2)).all()
    for keep, run in inside["runs"].items():
        has = run["keys"] != S.NONE
        assert has[v].sum() > 50 and has[:v].sum() > 1000, keep
