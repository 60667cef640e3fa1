"""CPU: the generated marching-cubes table, the numpy restatement of the TSDF fusion (tests/fusion_ref.py) on analytic depth
maps of a sphere, the sampled cameras and the argument checks of the new entry points (no kernel is launched)."""
import ctypes

import numpy as np
import pytest

import fusion_ref as fr

CENTRE, RADIUS = np.array([0.1, 1.2, -0.05]), 0.45
VOXEL, TRUNC = 0.02, 0.05
H = W = 200
INTR = (560.0, 560.0, (W - 1) / 2, (H - 1) / 2)


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


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_mc_table_closes_random_grids(seed):
    """All weights 1, random f32 values: every mesh edge that is not on the grid's boundary lies in exactly two triangles, which
    run through it in opposite directions -- the faces of neighbouring cubes agree, whatever the signs (ambiguous faces included)."""
    rng = np.random.default_rng(seed)
    vol = {"voxel": 0.1, "trunc": 0.3, "u0": np.array([-1, 0, 2]), "nu": np.array([1, 1, 1]),
           "tsdf": rng.normal(size=(16, 16, 16)).astype(np.float32), "weight": np.ones((16, 16, 16), np.float32),
           "color": rng.uniform(0, 255, size=(3, 16, 16, 16)).astype(np.float32)}
    verts, faces, colors = fr.marching_cubes(vol)
    assert len(faces) > 1000 and faces.max() == len(verts) - 1 and len(np.unique(faces)) == len(verts)
    assert colors.min() >= 0 and colors.max() <= 1
    lo = np.array([fr._centres(vol, a)[0] for a in range(3)])
    hi = np.array([fr._centres(vol, a)[-1] for a in range(3)])
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    on_wall = lambda v: (verts[v] == lo) | (verts[v] == hi)
    boundary = (on_wall(d[:, 0]) & on_wall(d[:, 1])).any(1)        # both ends on the same outer plane of the grid
    key = d[:, 0] * len(verts) + d[:, 1]
    rev = d[:, 1] * len(verts) + d[:, 0]
    assert len(np.unique(key)) == len(key)                         # no directed edge twice
    interior = ~boundary
    assert interior.sum() > 1000 and np.isin(rev[interior], key).all()
    assert not np.isin(rev[boundary], key).any()


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
