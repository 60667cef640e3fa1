"""CPU: the generated marching-cubes table, the numpy restatement of the TSDF fusion (tests/fusion_ref.py) on analytic depth
maps of a sphere, the sampled cameras and the argument checks of the new entry points (no kernel is launched).  Also the
inputs tests/test_gpu_fusion.py feeds the kernels -- synthetic volumes, the skewed views -- with the conditions they have to
meet, and the restatement's integration against the rule in f64, voxel by voxel."""
import ctypes
import functools

import numpy as np
import pytest

import fusion_ref as fr

CENTRE, RADIUS = np.array([0.1, 1.2, -0.05]), 0.45
VOXEL, TRUNC = 0.02, 0.05
H = W = 200
INTR = (560.0, 560.0, (W - 1) / 2, (H - 1) / 2)

# The skewed fixture: the same sphere through views that are not symmetric -- H != W, neither a multiple of the touch stride,
# fx != fy, an off-centre principal point, random colours, punched pixels, cameras near, oblique and overlapping.
SK_H, SK_W = 150, 222
SK_INTR = (410.0, 395.0, 130.3, 61.7)
SK_WIDE = (205.0, 197.5, 130.3, 61.7)       # half the focal lengths: the subject whole in the frame from 1.2 m
SK_BOXES = {"full": (CENTRE - RADIUS, CENTRE + RADIUS),
            "half": (CENTRE - RADIUS, np.array([CENTRE[0], CENTRE[1] + RADIUS, CENTRE[2] + RADIUS])),
            # `half` still holds the whole sphere in its padding of one unit; this one ends a unit short of the surface at +x
            "clipped": (CENTRE - RADIUS, np.array([CENTRE[0] - 0.3, CENTRE[1] + RADIUS, CENTRE[2] + RADIUS]))}


def skewed_views():
    """[(intrinsic, extrinsic, depth [150,222] f32, rgb8 [150,222,3] uint8)]: eye, target - CENTRE, intrinsics per view."""
    rig = [((1.0, 0.0, 0.0), (0.0, 0.0, 0.0), SK_INTR),            # head-on at 1 m: the sphere overflows the frame's height
           ((0.52, 0.05, 0.0), (0.0, 0.0, 0.0), SK_INTR),          # 7 cm outside the surface: voxels behind the camera
           ((0.9, 0.5, 0.7), (0.1, 0.3, 0.2), SK_INTR),            # oblique, the target off the centre
           ((-0.6, -0.8, 0.9), (-0.2, 0.1, -0.25), SK_INTR),       # oblique from the other side
           ((1.2, 0.0, 0.0), (0.0, 0.0, 0.0), SK_WIDE),            # the first direction again, wider: weights above 1
           ((1.15, 0.2, 0.1), (0.0, 0.0, 0.0), SK_WIDE)]           # and next to it
    rng = np.random.default_rng(7)
    views = []
    for eye, target, intr in rig:
        E = fr.look_at_extrinsic(CENTRE + np.asarray(eye), CENTRE + np.asarray(target))
        depth, _ = fr.sphere_view(CENTRE, RADIUS, intr, E, SK_H, SK_W)
        depth[rng.random(depth.shape) < 0.03] = 0
        views.append((intr, E, depth, rng.integers(0, 256, size=(SK_H, SK_W, 3), dtype=np.uint8)))
    return views


def test_mc_table_uses_exactly_the_crossing_edges():
    from gaustar_amd import fusion
    table = fusion.mc_table()
    assert table.shape == (256, 16) and table.dtype == np.int32
    for case in range(256):
        crossing = {e for e in range(12) if ((case >> fusion.edge_corners(e)[0]) ^ (case >> fusion.edge_corners(e)[1])) & 1}
        row = table[case]
        n = int((row >= 0).sum())
        assert n % 3 == 0 and n // 3 <= 5 and (row[n:] == -1).all(), case
        assert set(row[:n].tolist()) == crossing, case
        tris = row[:n].reshape(-1, 3)
        assert all(len(set(t)) == 3 for t in tris.tolist()), case
    assert (table[0] == -1).all() and (table[255] == -1).all()
    # every edge joins two corners that differ in one coordinate, the lower one first
    for e in range(12):
        lo, hi = fusion.edge_corners(e)
        assert hi - lo == 1 << (e >> 2) and not lo & (1 << (e >> 2))


def full_weight_volume(seed):
    """One unit with every weight 1 and random f32 values: cubes up to the grid's wall, ambiguous faces included."""
    rng = np.random.default_rng(seed)
    return {"voxel": 0.1, "trunc": 0.3, "u0": np.array([-1, 0, 2]), "nu": np.array([1, 1, 1]),
            "tsdf": rng.normal(size=(16, 16, 16)).astype(np.float32), "weight": np.ones((16, 16, 16), np.float32),
            "color": rng.uniform(0, 255, size=(3, 16, 16, 16)).astype(np.float32)}


def interior_edges_closed(vol, verts, faces):
    """Asserts that no directed edge occurs twice, that every edge off the grid's wall has its reverse and that none on the wall
    has; returns the number of directed edges off the wall."""
    lo = np.array([fr._centres(vol, a)[0] for a in range(3)])
    hi = np.array([fr._centres(vol, a)[-1] for a in range(3)])
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    on_wall = lambda v: (verts[v] == lo) | (verts[v] == hi)
    boundary = (on_wall(d[:, 0]) & on_wall(d[:, 1])).any(1)        # both ends on the same outer plane of the grid
    key = d[:, 0] * len(verts) + d[:, 1]
    rev = d[:, 1] * len(verts) + d[:, 0]
    assert len(np.unique(key)) == len(key)                         # no directed edge twice
    interior = ~boundary
    assert np.isin(rev[interior], key).all()
    assert not np.isin(rev[boundary], key).any()
    return int(interior.sum())


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mc_table_closes_random_grids(seed):
    """All weights 1, random f32 values: every mesh edge that is not on the grid's boundary lies in exactly two triangles, which
    run through it in opposite directions -- the faces of neighbouring cubes agree, whatever the signs (ambiguous faces included)."""
    vol = full_weight_volume(seed)
    verts, faces, colors = fr.marching_cubes(vol)
    assert len(faces) > 1000 and faces.max() == len(verts) - 1 and len(np.unique(faces)) == len(verts)
    assert colors.min() >= 0 and colors.max() <= 1
    assert interior_edges_closed(vol, verts, faces) > 1000


@pytest.fixture(scope="module")
def sphere_volume():
    vol = fr.new_volume(CENTRE - RADIUS, CENTRE + RADIUS, VOXEL, TRUNC)
    for E in fr.sphere_rig(CENTRE):
        depth, rgb8 = fr.sphere_view(CENTRE, RADIUS, INTR, E, H, W)
        assert (depth > 0).sum() > 5000
        touched = fr.integrate(vol, depth, rgb8, INTR, E)
        assert touched.any()
    return vol


def test_restatement_fuses_an_analytic_sphere(sphere_volume):
    vol = sphere_volume
    verts, faces, colors = fr.marching_cubes(vol)
    closed, euler = fr.directed_edge_stats(faces)
    assert closed and euler == 2
    assert fr.signed_volume(verts, faces) > 0                      # triangles face positive tsdf: outward
    np.testing.assert_allclose(fr.signed_volume(verts, faces), 4 / 3 * np.pi * RADIUS ** 3, rtol=0.02)
    err = np.abs(np.linalg.norm(verts.astype(np.float64) - CENTRE, axis=1) - RADIUS)
    print("sphere: max |r - R| =", err.max(), "voxel =", VOXEL)
    assert err.max() < VOXEL
    np.testing.assert_allclose(colors * 255, np.broadcast_to([200, 120, 40], colors.shape), atol=1e-3)
    # the running means count views: integer weights, at most the number of views
    w = vol["weight"]
    assert (w == np.round(w)).all() and w.max() <= 14 and (np.abs(vol["tsdf"]) <= 1).all()


def test_touch_marks_the_units_around_the_surface(sphere_volume):
    vol = fr.new_volume(CENTRE - RADIUS, CENTRE + RADIUS, VOXEL, TRUNC)
    E = fr.sphere_rig(CENTRE)[0]
    depth, rgb8 = fr.sphere_view(CENTRE, RADIUS, INTR, E, H, W)
    touched = fr.integrate(vol, depth, rgb8, INTR, E)
    # weights appear in touched units only
    per_unit = vol["weight"].reshape(touched.shape[0], 16, touched.shape[1], 16, touched.shape[2], 16).max(axis=(1, 3, 5))
    assert (per_unit[~touched] == 0).all() and (per_unit[touched] > 0).any() and 0 < touched.sum() < touched.size


# ------------------------------------------------------------------------------------------------ synthetic volumes
def synthetic_volume(u0, nu, voxel, tsdf, weight, color):
    nz, ny, nx = (16 * int(n) for n in nu[::-1])
    assert tsdf.shape == weight.shape == color.shape[1:] == (nz, ny, nx)
    assert tsdf.dtype == weight.dtype == color.dtype == np.float32
    return {"voxel": float(voxel), "trunc": 2.5 * float(voxel), "u0": np.asarray(u0, np.int64), "nu": np.asarray(nu, np.int64),
            "tsdf": tsdf, "weight": weight, "color": color}


def random_holes_volume(seed):
    """3 x 1 x 2 units (nx, ny, nz all different) of N(0, 1) values, 5 % of them +0.0 and 2 % -0.0, weight 0 on 15 % of the
    voxels and 1..8 elsewhere, colours uniform in [0, 255)."""
    rng = np.random.default_rng(seed)
    shape = (32, 16, 48)
    tsdf = rng.normal(size=shape).astype(np.float32)
    pick = rng.random(shape)
    tsdf[pick < 0.05] = 0.0
    tsdf[(pick >= 0.05) & (pick < 0.07)] = -0.0
    weight = np.where(rng.random(shape) < 0.15, 0, rng.integers(1, 9, size=shape)).astype(np.float32)
    return synthetic_volume((-2, 1, -1), (3, 1, 2), 0.013, tsdf, weight, rng.uniform(0, 255, size=(3,) + shape).astype(np.float32))


def case_blocks_volume():
    """2 x 2 x 2 units whose weight is non-zero on 256 separate blocks of 2 x 2 x 2 voxels, on a pitch of 3: block c (its lowest
    voxel at 1 + 3 (c % 10, c // 10 % 10, c // 100)) is one cube of case c, +-(0.1 .. 1.0) per corner.
    -> (volume, flat index of every block's lowest voxel [256])."""
    rng = np.random.default_rng(11)
    shape = (32, 32, 32)
    tsdf = rng.normal(size=shape).astype(np.float32)               # (never read where the weight is 0)
    weight = np.zeros(shape, np.float32)
    at = np.zeros(256, np.int64)
    for c in range(256):
        x, y, z = 1 + 3 * (c % 10), 1 + 3 * (c // 10 % 10), 1 + 3 * (c // 100)
        at[c] = (z * 32 + y) * 32 + x
        for i in range(8):
            p = (z + (i >> 2), y + (i >> 1 & 1), x + (i & 1))
            weight[p] = rng.integers(1, 9)
            tsdf[p] = np.float32(rng.uniform(0.1, 1.0)) * (-1 if c >> i & 1 else 1)
    return synthetic_volume((-1, -1, 0), (2, 2, 2), 0.013, tsdf, weight, rng.uniform(0, 255, size=(3,) + shape).astype(np.float32)), at


def one_negative_voxel_volume():
    """One unit, all weights 1, tsdf 0.5 but for one voxel inside: an octahedron."""
    tsdf = np.full((16, 16, 16), 0.5, np.float32)
    tsdf[5, 9, 3] = -0.25
    return synthetic_volume((0, -3, 1), (1, 1, 1), 0.013, tsdf, np.ones((16, 16, 16), np.float32), np.full((3, 16, 16, 16), 100, np.float32))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_random_holes_volume_holds_every_cube_case(seed):
    """The conditions on the input of the GPU comparison: every one of the 256 cases among the valid cubes, exact zeros of
    both signs at cube corners, more than 10 000 vertices, every vertex used, everything finite."""
    vol = random_holes_volume(seed)
    verts, faces, colors, n = fr.marching_cubes(vol, counts=True)
    per_case = np.bincount(n["case"][n["valid"]], minlength=256)
    print(f"seed {seed}: valid cubes {n['valid'].mean():.3f}, fewest per case {per_case.min()}, Nv {len(verts)}, Nf {len(faces)}")
    assert per_case.min() >= 6 and 0.2 < n["valid"].mean() < 0.35
    assert len(verts) > 10000 and len(faces) > 10000 and len(np.unique(faces)) == len(verts)
    assert np.isfinite(verts).all() and np.isfinite(colors).all()
    zero = (vol["tsdf"] == 0) & (vol["weight"] != 0)
    assert (zero & np.signbit(vol["tsdf"])).sum() > 100 and (zero & ~np.signbit(vol["tsdf"])).sum() > 100
    assert (n["vert_count"] == [bin(m).count("1") for m in n["edge_mask"]]).all() and n["tri_count"].sum() == len(faces)
    assert n["vert_count"].sum() == len(verts)


def test_case_blocks_volume_isolates_every_case():
    from gaustar_amd import fusion
    vol, at = case_blocks_volume()
    verts, faces, colors, n = fr.marching_cubes(vol, counts=True)
    assert np.array_equal(np.nonzero(n["valid"])[0], np.sort(at))              # the blocks' own cubes and no other
    assert np.array_equal(n["case"][at], np.arange(256))
    want = (fusion.mc_table() >= 0).sum(1) // 3
    assert np.array_equal(n["tri_count"][at], want) and n["tri_count"].sum() == want.sum() == len(faces)


def test_one_negative_voxel_is_an_octahedron():
    verts, faces, colors = fr.marching_cubes(one_negative_voxel_volume())
    assert len(verts) == 6 and len(faces) == 8
    assert fr.directed_edge_stats(faces) == (True, 2) and fr.signed_volume(verts, faces) > 0


# ------------------------------------------------------------------------------------------------ the skewed fixture
@functools.lru_cache(maxsize=None)
def skewed_reference(box):
    """The skewed views through the restatement into the volume over SK_BOXES[box], computed once and shared (tests/
    test_gpu_fusion.py too): (volume, touched units after each view, census of each view).  Nobody changes it."""
    vol = fr.new_volume(*SK_BOXES[box], VOXEL, TRUNC)
    touched, census = [], []
    for intr, E, depth, rgb8 in skewed_views():
        census.append(fr.integration_census(vol, depth, intr, E))
        touched.append(fr.integrate(vol, depth, rgb8, intr, E))
    for a in (vol["tsdf"], vol["weight"], vol["color"]):
        a.setflags(write=False)
    return vol, touched, census


def test_skewed_views_reach_every_branch_of_the_integration():
    """Conditions on the inputs of the GPU comparison, so that it cannot pass by exercising nothing."""
    views = skewed_views()
    assert len(views) >= 6 and SK_H % 4 and SK_W % 4 and SK_H != SK_W
    for intr in (SK_INTR, SK_WIDE):
        fx, fy, cx, cy = intr
        assert fx != fy and cx != cy and abs(cx - (SK_W - 1) / 2) > 10 and abs(cy - (SK_H - 1) / 2) > 10
    for intr, E, depth, rgb8 in views:
        assert depth.shape == (SK_H, SK_W) and (depth > 0).sum() > 5000 and len(np.unique(rgb8)) == 256
    assert any((d[::4, ::4] == 0).any() and (d[::4, ::4] > 0).any() for _, _, d, _ in views)    # (touch meets holes too)
    vol, touched, census = skewed_reference("full")
    total = {k: sum(c[k] for c in census) for k in census[0]}
    print("census per view:", census)
    print("census:", total, " weights:", dict(zip(*np.unique(vol["weight"], return_counts=True))))
    for c in census:
        assert c["behind"] + c["outside"] + c["hole"] + c["beyond"] + c["updated"] == c["voxels"] and c["clamped"] <= c["updated"]
    assert all(total[k] > 0 for k in ("behind", "outside", "hole", "beyond", "clamped", "updated"))
    assert total["updated"] - total["clamped"] > 1000
    w = np.unique(vol["weight"])
    assert len(w[w > 0]) >= 3
    assert len({t.sum() for t in touched}) > 1 and all(0 < t.sum() < t.size for t in touched)

    border = lambda t: t[[0, -1]].any() or t[:, [0, -1]].any() or t[:, :, [0, -1]].any()
    assert not any(border(t) for t in touched)                    # the full box holds every view's units in its padding
    half, half_touched, _ = skewed_reference("half")
    assert any(border(t) for t in half_touched)
    # `half` ends at the centre, but its padding of one unit still holds the sphere: nothing is clamped there.  `clipped` ends a
    # unit short: its touched units are the full box's, cut off -- views whose points all lie beyond it touch nothing
    clipped, clipped_touched, _ = skewed_reference("clipped")
    assert (clipped["u0"] == vol["u0"]).all() and clipped["nu"][0] < half["nu"][0] < vol["nu"][0]
    nx = int(clipped["nu"][0])
    cut = [t[:, :, nx:].any() for t in touched]
    assert sum(cut) >= 3 and all(np.array_equal(c, t[:, :, :nx]) for c, t in zip(clipped_touched, touched))
    assert any(c.any() and border(c) for c in clipped_touched) and any(not c.any() for c in clipped_touched)
    assert (clipped["weight"] > 0).sum() > 1000


def test_restatement_follows_the_rule_voxel_by_voxel():
    """fr.integrate against fr.integrate_voxel_f64 (the rule of include/gsr.h in f64, one voxel at a time) on every voxel of the
    touched units, one skewed view into an empty volume at a time.

    The bound on |tsdf - f64|.  eps = 2^-24 (f32, round to nearest), M = max(d, Z), n = the depth-to-distance factor, D = d - Z
    (so |D| <= M, Z <= M); the f64 side's own roundings (2^-53) and terms of order eps^2 are left to the last unit below.
      (float) Z                      |Zf - Z| <= eps M
      d - Zf                         |Df - D| <= eps M + eps |D| <= 2 eps M
      a = (u - (float) cx) / (float) fx:  A = max(cx, W - cx) / fx bounds |a| and cx / fx, so |da| <= eps (cx + |u - cx|) / fx
                                     (rounding cx, the subtraction) + 2 eps |a| (rounding fx, the division) <= 4 eps A; c alike with C
      q = a a + c c + 1              |dq| <= (2 |a| |da| + eps a^2) + (the same in c) + 2 eps q (two additions)
                                          <= eps q (9 (A^2 + C^2) + 2)                                          as q >= 1
      nf = sqrt(q)                   |nf - n| <= n (|dq| / (2 q) + eps) = eps n G,   G = 4.5 (A^2 + C^2) + 2
      Df nf                          |sf - D n| <= n |Df - D| + |D| n G eps + eps |D| n <= eps M n (3 + G)
      sf / (float) trunc             two more roundings of a value of at most M n / trunc: + 2 eps M n / trunc
    min(1, .) moves nothing apart and the mean of one sample, (0 * 0 + t) / 1, is exact:
      |tsdf - f64| <= (6 + G) 2^-24 M n / trunc        (5 + G from the lines above, 1 for what was left out).
    The decision sdf > -trunc is compared where the f64 sdf + trunc is farther from 0 than that bound times trunc, plus eps
    trunc for (float) trunc; the pixel coordinates are f64 on both sides, and a voxel is compared where they are farther than
    1e-9 from an integer and from the frame's limits (and Z from 0).  At most 0.1 % of the voxels may be left out."""
    eps = 2.0 ** -24
    views = skewed_views()
    compared = skipped = updated = 0
    worst = 0.0
    for intr, E, depth, rgb8 in views[1:3]:                        # the near camera (voxels behind it) and an oblique one
        fx, fy, cx, cy = intr
        G = 4.5 * ((max(cx, SK_W - cx) / fx) ** 2 + (max(cy, SK_H - cy) / fy) ** 2) + 2
        vol = fr.new_volume(*SK_BOXES["full"], VOXEL, TRUNC)
        touched = fr.integrate(vol, depth, rgb8, intr, E)
        L = 16 * VOXEL
        u0 = [int(v) for v in vol["u0"]]
        depth_rows, rgb_rows, Erows = depth.tolist(), rgb8.tolist(), E.tolist()
        tsdf, weight, color = vol["tsdf"], vol["weight"], vol["color"]
        for uz, uy, ux in zip(*(a.tolist() for a in np.nonzero(touched))):
            for kz in range(16):
                z = (u0[2] + uz) * L + (kz + 0.5) * VOXEL
                for ky in range(16):
                    y = (u0[1] + uy) * L + (ky + 0.5) * VOXEL
                    for kx in range(16):
                        x = (u0[0] + ux) * L + (kx + 0.5) * VOXEL
                        r = fr.integrate_voxel_f64((x, y, z), depth_rows, rgb_rows, intr, Erows, TRUNC)
                        g = (uz * 16 + kz, uy * 16 + ky, ux * 16 + kx)
                        near = abs(r["Z"]) < 1e-9
                        if "uf" in r:
                            for p, n in ((r["uf"], SK_W), (r["vf"], SK_H)):
                                near |= min(abs(p - round(p)), abs(p - 1e-4), abs(p - (n - 1e-4))) < 1e-9
                        bound = None
                        if "sdf" in r:
                            bound = (6 + G) * eps * max(r["d"], r["Z"]) * r["norm"] / TRUNC
                            near |= abs(r["sdf"] + TRUNC) <= bound * TRUNC + eps * TRUNC
                        if near:
                            skipped += 1
                            continue
                        compared += 1
                        assert (weight[g] == 1) == r["updated"] and weight[g] in (0, 1), (g, r)
                        if r["updated"]:
                            updated += 1
                            assert tuple(int(color[ch][g]) for ch in range(3)) == r["color"], (g, r)
                            err = abs(float(tsdf[g]) - r["tsdf"])
                            worst = max(worst, err / bound)
                            assert err <= bound, (g, r, float(tsdf[g]), bound)
                        else:
                            assert tsdf[g] == 0 and not color[:, g[0], g[1], g[2]].any(), (g, r)
        # nothing outside the touched units
        per_unit = weight.reshape(touched.shape[0], 16, touched.shape[1], 16, touched.shape[2], 16).max(axis=(1, 3, 5))
        assert (per_unit[~touched] == 0).all()
    print(f"f64 cross-check: compared {compared}, updated {updated}, left out {skipped}, worst |tsdf - f64| / bound = {worst:.3f}")
    assert updated > 3000 and compared > 50000
    assert skipped <= 0.001 * (compared + skipped)


def test_sample_cameras():
    from gaustar_amd import fusion, harness, scene
    E = fusion.sample_extrinsics(dist=3, look_at_y=1.2)
    assert E.shape == (60, 4, 4) and E.dtype == np.float64
    at = np.array([0.0, 1.2, 0.0])
    for e in E:
        R = e[:3, :3]
        np.testing.assert_allclose(R @ R.T, np.eye(3), atol=1e-6)
        assert np.linalg.det(R) > 0
        np.testing.assert_allclose(R @ at + e[:3, 3], [0, 0, 3], atol=1e-12)      # refined_mesh.py:65-69: `at` sits on the axis at `dist`
        assert (e[3] == [0, 0, 0, 1]).all()
    # azimuth is the outer loop, elevation -40..40 the inner one: index 2 = (azim 0, elev 0) = diag(1, -1, -1) by the formula
    np.testing.assert_allclose(E[2][:3, :3], np.diag([1.0, -1.0, -1.0]), atol=1e-7)
    np.testing.assert_allclose(E[2][:3, 3], [0, 1.2, 3.0], atol=1e-7)
    # (azim 90, elev 0): C = at + (3, 0, 0); z = (-1, 0, 0), x = up x z = (0, 0, -1), y = z x x = (0, -1, 0), as columns
    np.testing.assert_allclose(E[3 * 5 + 2][:3, :3], np.array([[0, 0, -1.0], [0, -1, 0], [-1, 0, 0]]), atol=1e-6)
    assert len({e.tobytes() for e in E}) == 60
    cam0 = harness.nerf_camera_from_scene(scene.look_at_camera((0.0, 1.2, 3.0), (0.0, 1.2, 0.0), 64, 48, focal_px=60.0))
    cams = fusion.sample_cameras(cam0, dist=3, look_at_y=1.2)
    assert len(cams) == 60 and all(c.width == 64 and c.height == 48 and c.fx == cam0.fx for c in cams)
    intr, extr = fusion.open3d_camera(cam0)
    assert intr == (cam0.fx, cam0.fy, 31.5, 23.5) and extr.shape == (4, 4)
    np.testing.assert_allclose(extr[:3, :3] @ extr[:3, :3].T, np.eye(3), atol=1e-6)


def test_fusion_entry_points_validate_without_gpu(hip_lib):
    null = None
    grid = (ctypes.c_int * 6)(-2, 0, 1, 3, 4, 5)
    assert hip_lib.gsr_fusion_volume_bytes(grid) == 3 * 4 * 5 * 4096 * 20
    assert hip_lib.gsr_fusion_volume_bytes((ctypes.c_int * 6)(0, 0, 0, 0, 1, 1)) == 0
    assert hip_lib.gsr_fusion_volume_bytes((ctypes.c_int * 6)(0, 0, 0, 100, 100, 100)) == 0     # 2^31 voxels or more
    assert hip_lib.gsr_fusion_prep_workspace_bytes(1080, 1920) == 2 * 2048 * 4 + 1080 * 1920 * 4
    assert hip_lib.gsr_fusion_prep(8, 8, null, null, 1, 1, 6.0, null, null, null, null) != 0 and b"null" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_fusion_prep(0, 8, null, null, 1, 1, 6.0, null, null, null, null) != 0 and b"positive" in hip_lib.gsr_last_error()
    cam = (ctypes.c_double * 28)(*([1.0] * 28))
    assert hip_lib.gsr_fusion_touch(8, 8, null, cam, 0.01, 0.02, grid, null, null) != 0 and b"null" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_fusion_touch(8, 8, null, cam, 0.0, 0.02, grid, null, null) != 0 and b"positive" in hip_lib.gsr_last_error()
    bad = (ctypes.c_double * 28)(*([float("nan")] * 28))
    assert hip_lib.gsr_fusion_integrate(8, 8, null, null, bad, 0.01, 0.02, grid, *([null] * 5)) != 0 and b"camera" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_fusion_integrate(8, 8, null, null, cam, 0.01, 0.02, grid, *([null] * 5)) != 0 and b"null" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_fusion_count(grid, *([null] * 7)) != 0 and b"null" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_fusion_emit(null, 0.01, *([null] * 10)) != 0 and b"grid" in hip_lib.gsr_last_error()


def test_adapter_rejects_what_is_not_implemented():
    from gaustar_amd import fusion
    for kw in ({"save_dir": "out/"}, {"smooth": True}, {"simplify_face_num": 40000}):
        with pytest.raises(ValueError):
            fusion.extract_mesh_fusion(None, None, **kw)
