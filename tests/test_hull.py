"""Shape from silhouettes without a GPU: the numpy restatement tests/hull_ref.py against the definition, the properties the GPU
tests then ask of the kernels (checked here on the restatement first), and the argument checks of gaustar_amd.hull and of the
C entry points, which come before any launch."""
import ctypes
import warnings

import numpy as np
import pytest

import fusion_ref as fr
import hull_ref as hr


def _tiny_masks():
    rng = np.random.default_rng(3)
    out = [np.zeros((5, 7), np.uint8), np.full((4, 3), 255, np.uint8)]
    one = np.zeros((6, 9), np.uint8)
    one[2, 5] = 200
    out.append(one)
    for shape, dens in (((9, 13), 0.5), ((16, 5), 0.05), ((2, 2), 0.5), ((11, 12), 0.95)):
        out.append((rng.random(shape) < dens).astype(np.uint8) * 255)
    grey = rng.integers(0, 256, (8, 10)).astype(np.uint8)       # (the threshold is a comparison, not a test for 255)
    out.append(grey)
    return out


@pytest.mark.parametrize("radius", [1, 3, 127])
def test_restated_distance_equals_the_definition(radius):
    for m in _tiny_masks():
        got = hr.mask_distance(m, 128, radius)
        assert got.dtype == np.int16 and np.array_equal(got, hr.mask_distance_brute(m, 128, radius))
        assert (got != 0).all() and (np.abs(got.astype(int)) <= radius * radius).all()
    assert (hr.mask_distance(np.zeros((5, 7), np.uint8), 128, radius) == -radius * radius).all()
    assert (hr.mask_distance(np.full((5, 7), 255, np.uint8), 128, radius) == radius * radius).all()
    assert (hr.mask_distance(np.full((5, 7), 127, np.uint8), 128, radius) < 0).all()


@pytest.fixture(scope="module")
def sphere_hull():
    v, f = hr.sphere_mesh()
    rig = hr.ring_rig(12)
    vol, touched, masks, _ = hr.carved(v, f, rig, 12, radius=4)
    return v, f, rig, vol, touched, masks


@pytest.fixture(scope="module")
def torus_hull():
    v, f = hr.torus_mesh()
    rig = hr.torus_rig()
    vol, touched, masks, _ = hr.carved(v, f, rig, 9, radius=4)
    return v, f, rig, vol, touched, masks


def test_restated_hull_of_a_sphere_contains_the_sphere(sphere_hull):
    """Every voxel centre deeper inside the sphere than the silhouettes can err is inside the hull.  A centre at depth t below
    the surface projects at least t f / z pixels inside every true silhouette; the rasterised mask's zero contour lies midway
    between the last covered and the first uncovered pixel centre (0.5 pixels off the true edge at most) and the distance to
    the nearest pixel CENTRE of the other kind, minus 0.5, misses the distance to that contour by less than a pixel: 1.5
    pixels in all, 1.5 z_max / f in metres.  The icosphere's faces lie inside the sphere of its vertices; its inscribed radius
    is taken from the mesh."""
    v, f, _rig, vol, touched, _ = sphere_hull
    tri = v[f]
    n = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    r_in = float((np.einsum("ij,ij->i", tri[:, 0], n) / np.linalg.norm(n, axis=1)).min())
    slack = 1.5 * (hr.DIST + 0.1) / hr.FOCAL
    cz, cy, cx = np.meshgrid(hr.centres(vol, 2), hr.centres(vol, 1), hr.centres(vol, 0), indexing="ij")
    r = np.sqrt(cx * cx + cy * cy + cz * cz)
    deep = r <= r_in - slack
    assert deep.sum() > 5000 and (vol["weight"] == 1).all()
    assert (vol["tsdf"][deep] < 0).all()
    assert (vol["tsdf"][r >= 0.15] > 0).all()                  # and it is a hull of THIS sphere, not of the volume
    assert 0 < touched.sum() < touched.size
    V, F, _ = fr.marching_cubes(vol)
    closed, euler = fr.directed_edge_stats(F)
    assert closed and euler == 2 and fr.signed_volume(V, F) > 0


def test_restated_hull_of_a_torus_keeps_its_hole(torus_hull):
    """One camera looks along the torus' axis: the hole is carved, the hull's Euler characteristic is 0."""
    _v, _f, _rig, vol, _touched, _ = torus_hull
    V, F, _ = fr.marching_cubes(vol)
    closed, euler = fr.directed_edge_stats(F)
    assert closed and euler == 0 and fr.signed_volume(V, F) > 0


@pytest.mark.parametrize("which", ["sphere", "torus"])
def test_restated_hull_projects_back_into_its_masks(which, sphere_hull, torus_hull):
    """k = 2, confirmed here on the restatement: the hull's own silhouette lies within the input mask grown by 2 pixels and
    covers the input mask shrunk by 2 pixels, in every carving camera (a voxel's footprint is 0.96 pixels)."""
    _v, _f, rig, vol, _touched, masks = sphere_hull if which == "sphere" else torus_hull
    V, F, _ = fr.marching_cubes(vol)
    for got, want in zip(hr.render_masks(V.astype(np.float64), F, rig), masks):
        assert hr.mask_check(got, want, 2) == (0, 0)


def test_the_edge_rig_does_what_it_is_for():
    """The scene of the bit-for-bit GPU tests: cameras with voxels behind znear, off the image, at u = W - 1 exactly, and a
    region below min_views that leaves the surface open."""
    v, f = hr.sphere_mesh()
    rig = hr.edge_rig()
    vol, touched, masks, d2s = hr.carved(v, f, rig, hr.EDGE_MIN_VIEWS, True)
    assert tuple(vol["nu"]) == (4, 4, 4)
    cams = hr.rig_cameras(rig, d2s, True)
    cz, cy, cx = np.meshgrid(hr.centres(vol, 2), hr.centres(vol, 1), hr.centres(vol, 0), indexing="ij")
    p = [a.reshape(-1) for a in (cx, cy, cz)]
    qz7 = ((cams[7]["R"][2, 0] * p[0] + cams[7]["R"][2, 1] * p[1]) + cams[7]["R"][2, 2] * p[2]) + cams[7]["t"][2]
    assert (qz7 <= hr.ZNEAR).sum() > 1000 and (qz7 > hr.ZNEAR).sum() > 1000
    ok6 = hr.view_distance(cams[6], *p)[0]
    assert 1000 < ok6.sum() < ok6.size - 1000 and masks[6][:, -1].any()      # crops the object, loses voxels off the image
    X, Y = hr.centres(vol, 0)[hr.AXIS_VOXEL[0]], hr.centres(vol, 1)[hr.AXIS_VOXEL[1]]
    Z = hr.centres(vol, 2)
    c = cams[8]
    qx = ((c["R"][0, 0] * X + c["R"][0, 1] * Y) + c["R"][0, 2] * Z) + c["t"][0]
    u = c["fx"] * (qx / (Z + hr.DIST)) + c["cx"]
    assert (u == 127.0).all() and hr.view_distance(c, np.full_like(Z, X), np.full_like(Z, Y), Z)[0].all()
    assert (vol["weight"] == 0).sum() > 10000 and (vol["weight"] == 1).sum() > 10000
    V, F, _ = fr.marching_cubes(vol)
    assert len(F) > 1000 and not fr.directed_edge_stats(F)[0]               # no faces where the weight is 0: the surface is open
    assert 0 < touched.sum() < touched.size


def test_restated_bounds_hold_the_hull(sphere_hull):
    v, _f, rig, _vol, _touched, masks = sphere_hull
    lo, hi = hr.hull_bounds(rig, masks, np.full(3, -0.25), np.full(3, 0.25))
    assert (lo <= v.min(0)).all() and (hi >= v.max(0)).all() and (hi - lo < 0.2 + 6 * 0.032).all()


# ------------------------------------------------------------------------------------------------ argument checks
def test_host_argument_checks_raise():
    import torch

    from gaustar_amd import hull
    good = np.zeros((8, 8), np.uint8)
    for bad_radius in (0, 128, -3):
        with pytest.raises(ValueError):
            hull.mask_distance(good, radius=bad_radius)
    with pytest.raises(ValueError):
        hull.mask_distance(good, threshold=300)
    with pytest.raises(ValueError):
        hull.mask_distance(good.astype(np.float32))
    with pytest.raises(ValueError):
        hull.mask_distance(np.zeros((8, 1), np.uint8))
    with pytest.raises(ValueError):
        hull.mask_distance(np.zeros((1, 8), np.uint8))
    with pytest.raises(ValueError):
        hull.mask_distance(np.zeros((2, 8, 8), np.uint8))
    with pytest.raises(ValueError):
        hull.mask_distance(torch.zeros(8, 8, dtype=torch.uint8))             # a CPU tensor: the wrong device
    rig = hr.ring_rig(3)
    with pytest.raises(ValueError):
        hull.carve_views(object(), rig, [good] * 3)
    with pytest.raises(ValueError):
        hull.finish(object())
    with pytest.raises(ValueError):
        hull.radius_for({"intrinsics": rig["intrinsics"][:2], "extrinsics": rig["extrinsics"], "shape": rig["shape"]}, [0] * 3, [1] * 3, 0.02)
    with pytest.raises(ValueError):
        hull.radius_for(rig, [0] * 3, [1] * 3, 0.0)
    with pytest.raises(ValueError):
        hull.hull_mesh(rig, [good] * 3, taubin_iterations=-1)
    assert [hull.default_min_views(n) for n in (1, 2, 5, 12, 160)] == [1, 2, 2, 3, 40]


def test_radius_for_equals_the_restatement_and_warns_once_when_capped():
    from gaustar_amd import hull
    rig = hr.ring_rig(5)
    for half, trunc in ((0.1, 0.02), (0.256, 0.02), (0.5, 0.064), (1.0, 0.2)):
        lo, hi = np.full(3, -half), np.full(3, half)
        assert hull.radius_for(rig, lo, hi, trunc) == hr.radius_for(rig, lo, hi, trunc)
    assert hull.radius_for(rig, np.full(3, -0.256), np.full(3, 0.256), 0.02) == 4     # ceil(0.02 * 360 / (3 - 0.256 sqrt(3)...) + 0.5)
    hull._warned_radius = False
    with pytest.warns(UserWarning, match="capped"):
        assert hull.radius_for(rig, np.full(3, -4.0), np.full(3, 4.0), 0.02) == 127   # the box reaches behind the cameras
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert hull.radius_for(rig, np.full(3, -4.0), np.full(3, 4.0), 0.02) == 127   # once per process
    lo, hi = hull.rig_box(rig)                        # the cameras look at the origin from DIST
    assert np.allclose(lo, -0.35 * hr.DIST, atol=1e-9) and np.allclose(hi, 0.35 * hr.DIST, atol=1e-9)
    shifted = hr.look_at_rig(hr.ring_eyes(5, 2.0, centre=(0.5, 1.0, -0.25)), (0.5, 1.0, -0.25), 45, 67, 200.0)
    lo, hi = hull.rig_box(shifted, 0.25)
    assert np.allclose(0.5 * (lo + hi), (0.5, 1.0, -0.25), atol=1e-9) and np.allclose(hi - lo, 1.0, atol=1e-9)


def test_entry_points_check_their_arguments_before_any_launch(hip_lib):
    from gaustar_amd import hull
    assert hip_lib.gsr_hull_camera_bytes() == hull.CAMERA_DTYPE.itemsize == 144
    assert hip_lib.gsr_hull_mask_distance_workspace_bytes(96, 128) == 96 * 128 and hip_lib.gsr_hull_mask_distance_workspace_bytes(0, 5) == 0
    buf = (ctypes.c_char * 80)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16      # (the volume's arrays must be 16-byte aligned)
    p = ctypes.c_void_p(base)
    err = lambda: hip_lib.gsr_last_error()
    assert hip_lib.gsr_hull_mask_distance(1, 8, p, 128, 4, p, p, None) != 0 and b"2 x 2" in err()
    assert hip_lib.gsr_hull_mask_distance(8, 8, p, 128, 0, p, p, None) != 0 and b"radius" in err()
    assert hip_lib.gsr_hull_mask_distance(8, 8, p, 128, 128, p, p, None) != 0 and b"radius" in err()
    assert hip_lib.gsr_hull_mask_distance(8, 8, p, 257, 4, p, p, None) != 0 and b"threshold" in err()
    assert hip_lib.gsr_hull_mask_distance(8, 8, None, 128, 4, p, p, None) != 0 and b"null" in err()
    grid = (ctypes.c_int * 6)(0, 0, 0, 1, 1, 1)
    table = np.zeros(1, hull.CAMERA_DTYPE)
    table[0] = (np.eye(3).reshape(-1), np.zeros(3), 100.0, 100.0, 4.0, 4.0, base, 8, 8)
    host = lambda: ctypes.c_void_p(table.ctypes.data)
    assert hip_lib.gsr_hull_carve(-1, host(), p, 0.01, grid, p, p, None) != 0 and b"negative" in err()
    assert hip_lib.gsr_hull_carve(1, host(), p, 0.0, grid, p, p, None) != 0 and b"voxel_size" in err()
    assert hip_lib.gsr_hull_carve(1, host(), p, 0.01, None, p, p, None) != 0 and b"grid" in err()
    assert hip_lib.gsr_hull_carve(1, None, p, 0.01, grid, p, p, None) != 0 and b"null" in err()
    assert hip_lib.gsr_hull_carve(0, None, None, 0.01, grid, p, p, None) == 0                 # no camera: nothing to do
    for field, value, word in (("W", 1, b"2 x 2"), ("fx", 0.0, b"focal"), ("d2", 0, b"distance map"), ("cx", np.nan, b"finite")):
        bad = table.copy()
        bad[field] = value
        assert hip_lib.gsr_hull_carve(1, ctypes.c_void_p(bad.ctypes.data), p, 0.01, grid, p, p, None) != 0 and word in err(), field
    assert hip_lib.gsr_hull_finish(grid, p, p, 0, 0.02, p, p, p, None) != 0 and b"min_views" in err()
    assert hip_lib.gsr_hull_finish(grid, p, p, 1, 0.0, p, p, p, None) != 0 and b"sdf_trunc" in err()
    assert hip_lib.gsr_hull_finish(grid, p, None, 1, 0.02, p, p, p, None) != 0 and b"null" in err()
