"""GPU: TSDF fusion and mesh extraction (gaustar_amd.fusion, gsr_fusion.hip) against the numpy restatement
(tests/fusion_ref.py) on analytic images, the image preparation on real renders, an opaque sphere end to end, determinism,
touch semantics and the entry points.

Measured on an MI355X (printed by the tests, kept here for the record):
  integration vs restatement: weight, tsdf and colour bit-equal (14 analytic views);
  extraction vs restatement: vertex positions bit-equal (bound: 2 f32 ulps), triangle sets identical;
  end to end (icosphere level 5, radius 0.9, voxel 0.008, 8 + 60 cameras): see test_end_to_end_on_an_opaque_sphere's docstring."""
import numpy as np
import pytest
import torch

import fusion_ref as fr
from test_fusion import CENTRE, H, INTR, RADIUS, TRUNC, VOXEL, W

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _analytic_views():
    return [(E,) + fr.sphere_view(CENTRE, RADIUS, INTR, E, H, W) for E in fr.sphere_rig(CENTRE)]


@pytest.fixture(scope="module")
def analytic(hip_lib):
    """The same 14 analytic views through the kernels and through the restatement."""
    from gaustar_amd import fusion
    views = _analytic_views()
    ref = fr.new_volume(CENTRE - RADIUS, CENTRE + RADIUS, VOXEL, TRUNC)
    vol = fusion.TSDFVolume(CENTRE - RADIUS, CENTRE + RADIUS, VOXEL, TRUNC, DEV)
    assert (vol.u0 == ref["u0"]).all() and (vol.nu == ref["nu"]).all()
    for E, depth, rgb8 in views:
        touched = fr.integrate(ref, depth, rgb8, INTR, E)
        fusion.integrate_views(vol, torch.from_numpy(depth).to(DEV), torch.from_numpy(rgb8).to(DEV), INTR, E)
        assert np.array_equal(vol.touched.cpu().numpy().astype(bool), touched.reshape(-1))
    return vol, ref


def test_integration_is_bit_equal_to_the_restatement(analytic):
    vol, ref = analytic
    w, t, c = vol.weight.cpu().numpy(), vol.tsdf.cpu().numpy(), vol.color.cpu().numpy()
    assert (ref["weight"] > 0).sum() > 10000
    assert np.array_equal(w, ref["weight"])
    print("max |tsdf - ref| =", np.abs(t - ref["tsdf"]).max(), " max |color - ref| =", np.abs(c - ref["color"]).max())
    assert np.array_equal(t.view(np.uint32), ref["tsdf"].view(np.uint32))
    assert np.array_equal(c.view(np.uint32), ref["color"].view(np.uint32))


def _canonical(faces):
    f = np.asarray(faces, np.int64)
    k = f.argmin(1)
    rot = np.stack([np.take_along_axis(f, ((k + i) % 3)[:, None], 1)[:, 0] for i in range(3)], 1)
    return rot[np.lexsort(rot.T[::-1])]


def test_extraction_matches_the_restatement(analytic):
    from gaustar_amd import fusion
    vol, ref = analytic
    verts, faces, colors = (x.cpu().numpy() for x in fusion.extract_triangle_mesh(vol))
    rv, rf, rc = fr.marching_cubes(ref)
    assert verts.shape[0] == rv.shape[0] > 1000 and faces.shape[0] == rf.shape[0] > 2000
    # one division and one multiply-add in f32: 2 ulps at the largest coordinate
    bound = 2 * np.spacing(np.float32(np.abs(rv).max()))
    print("max |verts - ref| =", np.abs(verts - rv).max(), "bound", bound, " max |colors - ref| =", np.abs(colors - rc).max())
    assert np.abs(verts.astype(np.float64) - rv).max() <= bound
    assert np.abs(colors - rc).max() <= 2 * np.spacing(np.float32(1))
    # vertices are the same ones in the same order (above), so a triangle of positions is a triangle of ids
    assert np.array_equal(_canonical(faces), _canonical(rf))
    closed, euler = fr.directed_edge_stats(faces)
    assert closed and euler == 2 and fr.signed_volume(verts, faces) > 0


def test_touch_semantics(hip_lib):
    """A unit that a view did not touch keeps its bits through that view."""
    from gaustar_amd import fusion
    views = _analytic_views()
    vol = fusion.TSDFVolume(CENTRE - RADIUS, CENTRE + RADIUS, VOXEL, TRUNC, DEV)
    up = lambda a: torch.from_numpy(a).to(DEV)
    for E, depth, rgb8 in views[:3]:
        fusion.integrate_views(vol, up(depth), up(rgb8), INTR, E)
    before = (vol.tsdf.clone(), vol.weight.clone(), vol.color.clone())
    E, depth, rgb8 = views[3]
    fusion.integrate_views(vol, up(depth), up(rgb8), INTR, E)
    nz, ny, nx = (int(v) for v in vol.nu[::-1])
    touched = vol.touched.view(nz, ny, nx).bool()
    assert 0 < int(touched.sum()) < touched.numel()
    per_voxel = touched.repeat_interleave(16, 0).repeat_interleave(16, 1).repeat_interleave(16, 2)
    changed = (vol.weight != before[1]) | (vol.tsdf != before[0]) | (vol.color != before[2]).any(0)
    assert changed.any() and not (changed & ~per_voxel).any()
    assert (before[1][~per_voxel] > 0).any()        # (units of the earlier views that this one left alone)


# ---------------------------------------------------------------------------------------------------- renders of a model
def _model(level):
    from gaustar_amd import harness, scene
    from test_gpu_topology import _opaque
    v, f = scene.icosphere(level, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    m = _opaque(harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), sh_levels=2))
    g = torch.Generator().manual_seed(0)
    with torch.no_grad():
        m._sh_coordinates_dc.copy_(torch.rand(m._sh_coordinates_dc.shape, generator=g) * 2 - 0.5)
        m._sh_coordinates_rest.copy_(torch.rand(m._sh_coordinates_rest.shape, generator=g) * 0.4 - 0.2)
    return m


def _cams():
    """8 cameras of test_gpu_topology._small_cams' size (480 x 270, focal 300, 3 m away), four at +65 and four at -65 degrees
    of elevation.  The sampled cameras stop at +-40 degrees and see the poles at 50 degrees of incidence; a cube corner
    sqrt(3) voxels = 1.39 cm below the surface is then 1.39 / cos(50) = 2.16 cm along the ray, beyond sdf_trunc = 2 cm: it
    keeps weight 0 and its cubes stay invalid.  Below acos(1.39 / 2) = 46 degrees of incidence every corner is reached, and
    with these eight no point of the sphere is farther than that from its nearest camera."""
    from gaustar_amd import harness, scene
    c = np.asarray(scene.SUBJECT_CENTER)
    el = np.deg2rad(65.0)
    eyes = [c + 3.0 * np.array([np.cos(el) * np.cos(a), s * np.sin(el), np.cos(el) * np.sin(a)])
            for s in (1.0, -1.0) for a in np.deg2rad([0.0, 90.0, 180.0, 270.0])]
    return [harness.nerf_camera_from_scene(scene.look_at_camera(tuple(e), scene.SUBJECT_CENTER, 480, 270, focal_px=300.0)) for e in eyes]


@pytest.fixture(scope="module")
def sphere_model(hip_lib):
    return _model(5), _cams()


def test_renders_are_the_reference_calls_and_prep_matches(sphere_model):
    from gaustar_amd import fusion
    model, cams = sphere_model
    renders = fusion.FusionRenders(model)
    sampled = fusion.sample_cameras(cams[0])
    for cam in (cams[0], cams[3], sampled[7]):
        rgb, da = renders(cam)
        with torch.no_grad():
            a = model.render_image_gaussian_rasterizer(cam, bg_color=[0.0, 1.0, 0.0], sh_deg=model.sh_levels - 1,
                                                       compute_color_in_rasterizer=True, compute_covariance_in_rasterizer=True)
            b = model.render_image_gaussian_rasterizer(cam, bg_color=[0.0, 0.0, 0.0], sh_deg=0, compute_color_in_rasterizer=False,
                                                       use_solid_surface=False, point_colors=renders.depth_alpha_colors(cam))
        assert torch.equal(rgb.permute(1, 2, 0), a) and torch.equal(da.permute(1, 2, 0), b)
        assert torch.equal(da[0], da[1]) and float(da[2].max()) > 0.9
        for flags in ((True, True), (False, True), (True, False)):
            depth, rgb8 = fusion.prepare_images(rgb, da, 6.0, *flags)
            want_d, want_c = fr.prep(a.cpu().numpy(), b.cpu().numpy(), 6.0, *flags)
            assert np.array_equal(depth.cpu().numpy().view(np.uint32), want_d.view(np.uint32)), flags
            assert np.array_equal(rgb8.cpu().numpy(), want_c)
        depth, rgb8 = fusion.fusion_inputs(model, cam)
        want_d, want_c = fr.prep(a.cpu().numpy(), b.cpu().numpy())
        assert np.array_equal(depth.cpu().numpy(), want_d) and np.array_equal(rgb8.cpu().numpy(), want_c)
        assert (want_d > 0).sum() > 1000 and ((want_d == 0) & (b.cpu().numpy()[..., 2] >= 0.5)).sum() > 0     # (edge pixels went)
        trunc_d, _ = fusion.prepare_images(rgb, da, 2.9)
        assert float(trunc_d.max()) < 2.9 and (trunc_d > 0).any()
    # sampled views look at the subject through with_extrinsic
    assert float(renders(sampled[0])[1][2].max()) > 0.9


def test_end_to_end_on_an_opaque_sphere(sphere_model):
    """Icosphere level 5 (radius 0.9), opaque as test_gpu_topology._opaque makes it, 8 cameras + the 60 sampled ones, defaults
    (voxel 0.008, sdf_trunc 0.02): closed, Euler characteristic 2, every vertex within 1.5 voxels of radius 0.9 (one voxel of
    discretisation plus the splat thickness)."""
    from gaustar_amd import scene
    model, cams = sphere_model
    res = model.extract_mesh_fusion(cams, return_volume=True)
    assert res.n_views == 68 and res.n_blocks > 100
    verts, faces = res.verts.cpu().numpy(), res.faces.cpu().numpy()
    assert res.colors.shape == res.verts.shape and float(res.colors.min()) >= 0 and float(res.colors.max()) <= 1
    assert res.faces.dtype == torch.int32 and res.verts.dtype == torch.float32 and len(faces) > 100000
    closed, euler = fr.directed_edge_stats(faces)
    err = np.abs(np.linalg.norm(verts.astype(np.float64) - np.asarray(scene.SUBJECT_CENTER), axis=1) - scene.SUBJECT_RADIUS)
    print(f"end to end: Nv={len(verts)} Nf={len(faces)} closed={closed} euler={euler} max|r-R|={err.max():.5f} "
          f"({err.max() / 0.008:.3f} voxels) mean={err.mean():.5f} blocks={res.n_blocks}")
    d = np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]).astype(np.int64)
    und, cnt = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    odd = und[cnt != 2]
    if len(odd):
        p = verts[odd.reshape(-1)]
        lat = np.degrees(np.arcsin(np.clip((p[:, 1] - scene.SUBJECT_CENTER[1]) / scene.SUBJECT_RADIUS, -1, 1)))
        print(f"edges not in two triangles: {len(odd)} (counts {np.unique(cnt[cnt != 2])}), latitude histogram (15-degree bins from -90): "
              f"{np.histogram(lat, bins=12, range=(-90, 90))[0].tolist()}")
    signed = np.linalg.norm(verts.astype(np.float64) - np.asarray(scene.SUBJECT_CENTER), axis=1) - scene.SUBJECT_RADIUS
    print(f"signed r - R: mean {signed.mean():.5f} min {signed.min():.5f} max {signed.max():.5f}; weight max {float(res.weight.max())}")
    assert closed and euler == 2
    assert err.max() <= 1.5 * 0.008
    assert fr.signed_volume(verts, faces) > 0
    assert tuple(res.tsdf.shape) == res.dims[::-1] and res.origin.shape == (3,)


def test_bit_reproducible_across_calls_and_views_in_flight(sphere_model):
    model, cams = sphere_model
    kw = dict(voxel_size=0.016, sdf_trunc=0.04, return_volume=True)
    a = model.extract_mesh_fusion(cams, **kw)
    b = model.extract_mesh_fusion(cams, **kw)
    c = model.extract_mesh_fusion(cams, views_in_flight=1, **kw)
    d = model.extract_mesh_fusion(cams, views_in_flight=3, **kw)
    assert a.verts.shape[0] > 1000
    for x in (b, c, d):
        for k in ("tsdf", "weight", "color", "verts", "faces", "colors"):
            assert torch.equal(getattr(a, k), getattr(x, k)), k
        assert x.n_blocks == a.n_blocks and x.n_views == a.n_views


def test_entry_points_and_errors(sphere_model):
    from gaustar_amd import formats, fusion
    model, cams = sphere_model
    kw = dict(voxel_size=0.03, sdf_trunc=0.075)

    class Nerf:
        cameras = cams

    a = fusion.extract_mesh_fusion(model, Nerf, depth_trunc=6, mask_backgrond=True, remove_depth_edge=True, smooth=False,
                                   simplify_face_num=0, save_dir=None, **kw)
    b = fusion.fuse_mesh(model, cams, **kw)
    assert torch.equal(a.verts, b.verts) and torch.equal(a.faces, b.faces) and torch.equal(a.colors, b.colors)
    only_rig = fusion.fuse_mesh(model, cams, sample_cameras=False, **kw)
    assert only_rig.n_views == 8 and a.n_views == 68
    for bad in ({"save_dir": "out/"}, {"smooth": True}, {"simplify_face_num": 40000}):
        with pytest.raises(ValueError):
            fusion.extract_mesh_fusion(model, Nerf, **bad)
    with pytest.raises(ValueError):
        fusion.TSDFVolume([0, 0, 0], [100, 100, 100], 0.008, 0.02, DEV)     # a dense volume of 2^31 voxels or more
    import os
    import tempfile
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "fusion.obj")
        formats.save_obj(path, a.verts.cpu().numpy(), a.faces.cpu().numpy(), a.colors.cpu().numpy())
        lines = open(path).read().splitlines()
    assert sum(l.startswith("v ") for l in lines) == a.verts.shape[0] and len(lines[0].split()) == 7
    assert sum(l.startswith("f ") for l in lines) == a.faces.shape[0]
