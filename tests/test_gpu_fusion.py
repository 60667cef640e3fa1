"""GPU: TSDF fusion and mesh extraction (gaustar_amd.fusion, gsr_fusion.hip) against the numpy restatement
(tests/fusion_ref.py) on analytic images, the image preparation on real renders, an opaque sphere end to end, determinism,
touch semantics and the entry points.  Beyond the sphere seen whole: the extraction on synthetic volumes (all 256 cube cases,
weight holes, exact zeros, the grid's wall, empty totals), the integration of tests/test_fusion.py's skewed views (H != W, fx !=
fy, holes, cameras near and oblique, boxes that cut the surface off) and the image preparation's degenerate branches.

Measured on an MI355X (printed by the tests, kept here for the record):
  integration vs restatement: weight, tsdf and colour bit-equal (14 analytic views);
  extraction vs restatement: vertex positions bit-equal (bound: 2 f32 ulps), triangle sets identical;
  end to end (icosphere level 5, radius 0.9, voxel 0.008, 8 + 60 cameras): see test_end_to_end_on_an_opaque_sphere's docstring."""
import numpy as np
import pytest
import torch

import fusion_ref as fr
import test_fusion as tf
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


# ---------------------------------------------------------------------------------------------------- synthetic volumes
def _upload(ref):
    """A restatement volume (tests/test_fusion.py's builders) as a TSDFVolume of the same directory."""
    from gaustar_amd import fusion
    vol = fusion.TSDFVolume.from_units(ref["u0"], ref["nu"], ref["voxel"], ref["trunc"], DEV)
    assert (vol.u0 == ref["u0"]).all() and (vol.nu == ref["nu"]).all() and (vol.u0 < 0).any() and vol.voxel_size == ref["voxel"]
    for k in ("tsdf", "weight", "color"):
        getattr(vol, k).copy_(torch.from_numpy(ref[k]))
    return vol


def _count(hip_lib, vol):
    """gsr_fusion_count's own outputs (extract_triangle_mesh keeps only their scans): edge_mask, vert_count, tri_count."""
    from gaustar_amd import _lib, fusion
    n = vol.tsdf.numel()
    mask = torch.full((n,), 0xAA, dtype=torch.uint8, device=DEV)
    vcnt, tcnt = (torch.full((n,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    table = torch.from_numpy(fusion.mc_table()).to(DEV)
    _lib.check(hip_lib.gsr_fusion_count(vol.grid, _lib.ptr(vol.tsdf), _lib.ptr(vol.weight), _lib.ptr(table), _lib.ptr(mask),
                                        _lib.ptr(vcnt), _lib.ptr(tcnt), torch._C._cuda_getCurrentRawStream(mask.device.index)), "gsr_fusion_count")
    return mask.cpu().numpy(), vcnt.cpu().numpy(), tcnt.cpu().numpy()


def _extraction_matches(hip_lib, vol, ref, what):
    """The kernels' mesh and counts of `vol` against fr.marching_cubes(ref), as test_extraction_matches_the_restatement compares
    them; -> (verts, faces, colors, the restatement's counts)."""
    from gaustar_amd import fusion
    rv, rf, rc, n = fr.marching_cubes(ref, counts=True)
    mask, vcnt, tcnt = _count(hip_lib, vol)
    assert np.array_equal(mask, n["edge_mask"]) and np.array_equal(vcnt, n["vert_count"]), what
    differ = np.nonzero(tcnt != n["tri_count"])[0]
    assert len(differ) == 0, f"{what}: tri_count differs at voxels {differ[:8]} (cases {n['case'][differ[:8]]})"
    verts, faces, colors = (x.cpu().numpy() for x in fusion.extract_triangle_mesh(vol))
    assert verts.shape == rv.shape and faces.shape == rf.shape and colors.shape == rc.shape, what
    assert verts.dtype == np.float32 and faces.dtype == np.int32 and colors.dtype == np.float32
    if len(rv):
        # one division and one multiply-add in f32: 2 ulps at the largest coordinate
        bound = 2 * np.spacing(np.float32(np.abs(rv).max()))
        print(f"{what}: Nv={len(rv)} Nf={len(rf)} max |verts - ref| =", np.abs(verts - rv).max(), "bound", bound,
              " max |colors - ref| =", np.abs(colors - rc).max())
        assert np.abs(verts.astype(np.float64) - rv).max() <= bound, what
        assert np.abs(colors - rc).max() <= 2 * np.spacing(np.float32(1)), what
        assert np.array_equal(_canonical(faces), _canonical(rf)), what
    return verts, faces, colors, n


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_extraction_on_random_volumes_with_holes(hip_lib, seed):
    """All 256 cube cases, ambiguous faces, +0.0 and -0.0, weight holes, nx != ny != nz."""
    ref = tf.random_holes_volume(seed)
    rv, _, _, n = fr.marching_cubes(ref, counts=True)                          # the input is what it claims to be, first
    assert np.bincount(n["case"][n["valid"]], minlength=256).min() >= 1 and len(rv) > 10000
    verts, faces, colors, _ = _extraction_matches(hip_lib, _upload(ref), ref, f"random with holes, seed {seed}")
    assert len(np.unique(faces)) == len(verts) and np.isfinite(verts).all() and np.isfinite(colors).all()


def test_extraction_of_one_isolated_cube_per_case(hip_lib):
    from gaustar_amd import fusion
    ref, at = tf.case_blocks_volume()
    vol = _upload(ref)
    want = (fusion.mc_table() >= 0).sum(1) // 3
    tcnt = _count(hip_lib, vol)[2]
    for case in range(256):
        assert tcnt[at[case]] == want[case], f"case {case}: {tcnt[at[case]]} triangles, the table's row has {want[case]}"
    assert tcnt.sum() == want.sum()
    verts, faces, colors, n = _extraction_matches(hip_lib, vol, ref, "one cube per case")
    assert np.array_equal(n["case"][at], np.arange(256)) and len(faces) == want.sum()


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_extraction_closes_full_weights_up_to_the_wall(hip_lib, seed):
    """tests/test_fusion.py::test_mc_table_closes_random_grids' property, of the kernels' faces."""
    ref = tf.full_weight_volume(seed)
    verts, faces, colors, _ = _extraction_matches(hip_lib, _upload(ref), ref, f"full weights, seed {seed}")
    assert len(faces) > 1000 and faces.max() == len(verts) - 1 and len(np.unique(faces)) == len(verts)
    assert colors.min() >= 0 and colors.max() <= 1
    assert tf.interior_edges_closed(ref, verts, faces) > 1000


def test_extraction_of_degenerate_totals(hip_lib):
    ref = tf.one_negative_voxel_volume()
    verts, faces, colors, _ = _extraction_matches(hip_lib, _upload(ref), ref, "one negative voxel")
    assert len(verts) == 6 and len(faces) == 8
    assert fr.directed_edge_stats(faces) == (True, 2) and fr.signed_volume(verts, faces) > 0
    np.testing.assert_allclose(colors, 100 / 255, rtol=1e-6)
    nothing = dict(ref, weight=np.zeros_like(ref["weight"]))                 # no cube is valid: the emit call gets null outputs
    outside = dict(ref, tsdf=np.abs(ref["tsdf"]))                            # every cube is valid and none is crossed
    outside["tsdf"][0, 0, 0] = 0.0
    for r, what in ((nothing, "all weights 0"), (outside, "all tsdf >= 0")):
        verts, faces, colors, n = _extraction_matches(hip_lib, _upload(r), r, what)
        assert verts.shape == (0, 3) and faces.shape == (0, 3) and colors.shape == (0, 3)
        assert n["valid"].any() == (what == "all tsdf >= 0")


# ---------------------------------------------------------------------------------------------------- the skewed views
def _skewed_on_device():
    up = lambda a: torch.from_numpy(a).to(DEV)
    return [(intr, E, up(depth), up(rgb8)) for intr, E, depth, rgb8 in tf.skewed_views()]


@pytest.fixture(scope="module", params=list(tf.SK_BOXES))
def skewed(hip_lib, request):
    """tests/test_fusion.py's skewed views through the kernels, into each of its boxes; the touched units are compared here,
    after every view."""
    from gaustar_amd import fusion
    ref, touched, _ = tf.skewed_reference(request.param)
    vol = fusion.TSDFVolume(*tf.SK_BOXES[request.param], VOXEL, TRUNC, DEV)
    assert (vol.u0 == ref["u0"]).all() and (vol.nu == ref["nu"]).all()
    for (intr, E, depth, rgb8), want in zip(_skewed_on_device(), touched):
        fusion.integrate_views(vol, depth, rgb8, intr, E)
        assert np.array_equal(vol.touched.cpu().numpy().astype(bool), want.reshape(-1)), request.param
    return vol, ref, request.param


def test_skewed_integration_is_bit_equal_to_the_restatement(skewed):
    vol, ref, box = skewed
    w, t, c = vol.weight.cpu().numpy(), vol.tsdf.cpu().numpy(), vol.color.cpu().numpy()
    assert (ref["weight"] > 0).sum() > 1000
    assert np.array_equal(w, ref["weight"])
    print(f"{box}: max |tsdf - ref| =", np.abs(t - ref["tsdf"]).max(), " max |color - ref| =", np.abs(c - ref["color"]).max(),
          " weights", np.unique(w).tolist())
    assert np.array_equal(t.view(np.uint32), ref["tsdf"].view(np.uint32))
    assert np.array_equal(c.view(np.uint32), ref["color"].view(np.uint32))


def test_skewed_extraction_matches_the_restatement(hip_lib, skewed):
    vol, ref, box = skewed
    verts, faces, colors, _ = _extraction_matches(hip_lib, vol, ref, f"skewed views, {box} box")
    assert len(verts) > 500 and len(faces) > 500


def test_a_stack_of_views_is_the_loop_over_them(skewed):
    """integrate_views with [V,H,W], [V,H,W,3], V intrinsics and V extrinsics: the bits of the view-by-view calls."""
    from gaustar_amd import fusion
    one_by_one, _, box = skewed
    views = _skewed_on_device()
    vol = fusion.TSDFVolume(*tf.SK_BOXES[box], VOXEL, TRUNC, DEV)
    fusion.integrate_views(vol, torch.stack([v[2] for v in views]), torch.stack([v[3] for v in views]), [v[0] for v in views],
                           np.stack([v[1] for v in views]))
    assert vol.n_views == one_by_one.n_views == len(views)
    for k in ("touched", "weight"):
        assert torch.equal(getattr(vol, k), getattr(one_by_one, k)), k
    for k in ("tsdf", "color"):
        assert torch.equal(getattr(vol, k).view(torch.int32), getattr(one_by_one, k).view(torch.int32)), k
    # one intrinsic for all views is taken for each of them
    a, b = (fusion.TSDFVolume(*tf.SK_BOXES[box], VOXEL, TRUNC, DEV) for _ in range(2))
    fusion.integrate_views(a, torch.stack([v[2] for v in views[:4]]), torch.stack([v[3] for v in views[:4]]), tf.SK_INTR,
                           [v[1] for v in views[:4]])
    for intr, E, depth, rgb8 in views[:4]:
        fusion.integrate_views(b, depth, rgb8, intr, E)
    assert torch.equal(a.tsdf.view(torch.int32), b.tsdf.view(torch.int32)) and torch.equal(a.weight, b.weight)
    assert torch.equal(a.color.view(torch.int32), b.color.view(torch.int32))


# ---------------------------------------------------------------------------------------------------- image preparation's edges
def _prep_cases(Hp, Wp):
    """(name, rgb [3,H,W], depth_alpha [3,H,W], depth_trunc): the special values tiled over the image."""
    n = Hp * Wp
    f32 = np.float32
    rng = np.random.default_rng(Hp * 1000 + Wp)
    tile = lambda vals, count=n: np.asarray(vals, f32)[np.arange(count) % len(vals)]
    unit = f32(1) / f32(255)
    rgb = tile([-0.5, 0.0, np.nextafter(unit, f32(0)), unit, np.nextafter(unit, f32(1)), 1.0, 1.5, 0.5, 254.5 / 255, 0.999999],
               3 * n).reshape(3, Hp, Wp)
    rnd = rng.uniform(0, 1, size=(3, Hp, Wp)).astype(f32)

    def da(ch0, alpha=1.0):
        out = np.zeros((3, Hp, Wp), f32)
        out[0] = out[1] = np.broadcast_to(np.asarray(ch0, f32), (n,) if np.ndim(ch0) == 1 else (Hp, Wp)).reshape(Hp, Wp)
        out[2] = np.broadcast_to(np.asarray(alpha, f32), (n,) if np.ndim(alpha) == 1 else (Hp, Wp)).reshape(Hp, Wp)
        return out

    step = np.where(np.arange(Wp) < Wp // 2, 2.0, 4.0)[None].repeat(Hp, 0)
    six = f32(6)
    return [("far", rnd, da(rng.uniform(10, 20, size=(Hp, Wp))), 100.0),
            ("flat", rnd, da(2.5), 6.0),
            ("step", rnd, da(step), 6.0),
            ("trunc", rnd, da(tile([six, np.nextafter(six, f32(0)), np.nextafter(six, f32(7)), 3.0])), 6.0),
            ("alpha", rnd, da(tile([2.0, 1.0, 1.5, 2.5, 0.0]), tile([0.0, 0.5, np.nextafter(f32(0.5), f32(0)), 1.0])), 6.0),
            ("rgb", rgb, da(rng.uniform(1, 3, size=(Hp, Wp))), 6.0)]


@pytest.mark.parametrize("shape", [(37, 53), (2, 3)])
def test_prep_at_its_edges(hip_lib, shape):
    """fusion_prep_kernel's degenerate branches, bit-equal to fr.prep: nothing below 10, a flat map, a step, depth_trunc and its
    f32 neighbours, alpha at 0 and around 0.5, rgb outside [0, 1] and around 1 / 255."""
    from gaustar_amd import fusion
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    seen = set()
    for name, rgb, da, trunc in _prep_cases(*shape):
        d0 = da[0] / (da[2] + np.float32(1e-8))
        assert np.isfinite(d0).all() and np.isfinite(rgb).all()
        for mask_background in (True, False):
            for remove_edge in (True, False):
                what = (name, mask_background, remove_edge)
                depth, rgb8 = (x.cpu().numpy() for x in fusion.prepare_images(up(rgb), up(da), trunc, mask_background, remove_edge))
                want_d, want_c = fr.prep(rgb.transpose(1, 2, 0), da.transpose(1, 2, 0), trunc, mask_background, remove_edge)
                assert np.array_equal(depth.view(np.uint32), want_d.view(np.uint32)), what
                assert np.array_equal(rgb8, want_c), what
                # what each case is about, on the expected side: the kernel equals it bit for bit
                if name == "far":
                    assert fr.tr.depth_edge(d0, 10.0) is None and np.array_equal(want_d, d0) and (want_d >= 10).all()
                elif name == "flat":
                    assert fr.tr.depth_edge(d0, 10.0).max() == 0 and (want_d == np.float32(2.5)).all()
                elif name == "step":
                    lost = want_d == 0
                    assert lost.any() == remove_edge and not lost.all()
                    if remove_edge and shape[1] > 4:
                        assert lost[:, shape[1] // 2 - 1: shape[1] // 2 + 1].all() and not lost[:, 0].any() and not lost[:, -1].any()
                elif name == "trunc" and not remove_edge:
                    flat = want_d.reshape(-1)[:4]
                    assert flat.tolist() == [0.0, float(np.nextafter(np.float32(6), np.float32(0))), 0.0, 3.0]
                elif name == "alpha" and not remove_edge:
                    # pixels 0..4: alpha 0, 0.5, just below 0.5, 1, 0 over ch0 2, 1, 1.5, 2.5, 0
                    flat = want_d.reshape(-1)[:5].tolist()
                    below = float(np.float32(1.5) / (np.nextafter(np.float32(0.5), np.float32(0)) + np.float32(1e-8)))
                    assert flat == [0.0, 2.0, 0.0 if mask_background else below, 2.5, 0.0] and below > 3.0
                elif name == "rgb":
                    # -0.5, 0, 1/255 less an ulp, 1/255, 1/255 plus an ulp, 1, 1.5, 0.5, 254.5/255, 0.999999 (channel-major)
                    first = want_c.transpose(2, 0, 1).reshape(-1)[:10].tolist()
                    assert first[:3] == [0, 0, 0] and first[3] in (0, 1) and first[4:] == [1, 255, 255, 127, 254, 254]
                seen.add(name)
    assert seen == {"far", "flat", "step", "trunc", "alpha", "rgb"}


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
