"""gaustar_amd.evaluate on the GPU against the numpy restatement tests/eval_ref.py (itself pinned by tests/test_evaluate.py).
Faces, barycentrics, closest points, distances, sample ids, counts and maxima are compared bit for bit: they use only IEEE
add, multiply, divide and square root of float64 in a stated order.  Sums are fixed-order on the device and pairwise in numpy:
those are held to the worst case of reordering a sum of n non-negative terms, n 2^-52 relative."""
import functools
import math

import numpy as np
import pytest
import torch

import eval_ref as ref
import tracking_ref
from loss_cases import LOSS_TOL

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _n(t):
    return t.cpu().numpy()


def _same(got, want):
    got, want = _n(got) if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _ev():
    from gaustar_amd import evaluate
    return evaluate


def _consts():
    from gaustar_amd import _lib
    lib = _lib.load()
    return int(lib.gsr_eval_tile()), int(lib.gsr_eval_queries())


def _check_hit(hit, points, verts, faces):
    dist, face, bary, closest = ref.surface_distance(points, verts, faces)
    assert hit.face.dtype == torch.int32 and hit.dist.dtype == torch.float64
    assert np.array_equal(_n(hit.face), face), np.nonzero(_n(hit.face) != face)[0][:10]
    assert _same(hit.dist, dist) and _same(hit.bary, bary) and _same(hit.closest, closest)
    return dist, face, bary, closest


# ---------------------------------------------------------------------------------------------------- 1 closest point
def test_hand_cases_on_the_device():
    pts = np.array([c[0] for c in ref.HAND_CASES], np.float64)
    hit = _ev().surface_distance(_t(pts), _t(ref.TRIANGLE), _t(np.array([[0, 1, 2]], np.int32)))
    _check_hit(hit, pts, ref.TRIANGLE, [[0, 1, 2]])
    assert np.array_equal(_n(hit.dist), np.sqrt([float(c[1]) for c in ref.HAND_CASES]))
    assert np.array_equal(_n(hit.bary), np.array([c[2] for c in ref.HAND_CASES], np.float64))


def test_mirror_tie_on_the_device():
    verts, faces, p = ref.MIRROR
    for f in (faces, faces[::-1].copy()):
        hit = _ev().surface_distance(_t(p), _t(verts), _t(f))
        assert int(hit.face[0]) == 0 and float(hit.dist[0]) == math.sqrt(5.0)


@functools.lru_cache(maxsize=None)
def _soup_case():
    T, Q = _consts()
    verts, faces = ref.triangle_soup(2 * T + 3, seed=11)
    pts = np.random.default_rng(12).uniform(-1.3, 1.3, size=(2 * Q + 1, 3))
    return T, Q, verts, faces, pts


F_CASES = ("1", "2", "T-1", "T", "T+1", "2*T+3")
K_CASES = ("1", "Q-1", "Q", "Q+1", "2*Q+1")


@pytest.mark.parametrize("k_case", K_CASES)
@pytest.mark.parametrize("f_case", F_CASES)
def test_sizes_around_the_tile_and_the_workgroup(f_case, k_case):
    T, Q, verts, faces, pts = _soup_case()
    F = eval(f_case, {"T": T})
    K = eval(k_case, {"Q": Q})
    f, p = faces[:F], pts[:K]
    hit = _ev().surface_distance(_t(p), _t(verts), _t(f))
    _check_hit(hit, p, verts, f)


def test_a_duplicated_face_gives_the_lower_index():
    """Face i copied to j > i, the two in different slices of a tile (j - i not a multiple of 16), in different waves (slices
    of different quarters), in different tiles: a query just above face i is equally far from both."""
    T, Q, verts, faces, _ = _soup_case()
    for i, j in ((1, 2), (1, 9), (1, T + 1), (1, T + 9), (T - 1, 2 * T + 2), (17, 33)):
        f = faces.copy()
        f[j] = f[i]
        tri = verts[f[i]]
        n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
        p = (tri.mean(0) + 1e-3 * n / np.linalg.norm(n))[None]
        want = ref.surface_distance(p, verts, f)
        both = ref.closest_pairs(p[0], *verts[f[i]])[0], ref.closest_pairs(p[0], *verts[f[j]])[0]
        assert both[0] == both[1] and want[1][0] == i
        hit = _ev().surface_distance(_t(np.repeat(p, Q + 1, 0)), _t(verts), _t(f))
        assert (_n(hit.face) == i).all() and (_n(hit.dist) == want[0][0]).all()


@functools.lru_cache(maxsize=None)
def _sphere():
    return ref.icosphere(2)


def test_icosphere_inside_on_and_outside():
    verts, faces = _sphere()
    assert len(faces) == 320
    dirs = np.random.default_rng(5).normal(size=(40, 3))
    dirs /= np.linalg.norm(dirs, axis=-1, keepdims=True)
    pts = np.concatenate([0.5 * dirs, np.zeros((1, 3)), verts[:30], verts[faces[:30]].mean(1), 1.5 * dirs, 40.0 * dirs[:3]])
    hit = _ev().surface_distance(_t(pts), _t(verts), _t(faces))
    dist, face, bary, closest = _check_hit(hit, pts, verts, faces)
    assert (dist[41:71] < 1e-15).all() and (dist[:40] > 0.4).all() and (np.abs(dist[101:141] - 0.5) < 0.03).all()
    assert (bary >= 0).all() and np.abs(bary.sum(-1) - 1).max() < 1e-15


def test_f32_vertices_are_widened():
    verts, faces = _sphere()
    v32 = verts.astype(np.float32)
    pts = np.random.default_rng(6).uniform(-1.2, 1.2, size=(50, 3))
    hit = _ev().surface_distance(_t(pts), _t(v32), _t(faces.astype(np.int64)))
    _check_hit(hit, pts, v32.astype(np.float64), faces)


def test_subset_and_live_count():
    T, Q, verts, faces, pts = _soup_case()
    f = faces[:T + 1]
    want = ref.surface_distance(pts, verts, f)
    subset = np.array([2 * Q, 0, 5, 5, Q, 3, 1], np.int32)
    hit = _ev().surface_distance(_t(pts), _t(verts), _t(f), subset=_t(subset))
    assert np.array_equal(_n(hit.face), want[1][subset]) and _same(hit.dist, want[0][subset])
    assert _same(hit.bary, want[2][subset]) and _same(hit.closest, want[3][subset])
    live = torch.tensor([4], dtype=torch.int32, device=DEV)
    hit = _ev().surface_distance(_t(pts), _t(verts), _t(f), subset=_t(subset), n_live=live)
    assert np.array_equal(_n(hit.face)[:4], want[1][subset[:4]]) and (_n(hit.face)[4:] == -1).all()
    assert _same(hit.closest[:4], want[3][subset[:4]]) and np.isinf(_n(hit.dist)[4:]).all() and np.isnan(_n(hit.bary)[4:]).all()
    with pytest.raises(ValueError):
        _ev().surface_distance(_t(pts), _t(verts), _t(f), subset=_t(np.array([0, len(pts)], np.int32)))


def test_closest_point_errors():
    ev = _ev()
    verts, faces = _sphere()
    pts = np.zeros((3, 3))
    bad = pts.copy()
    bad[1, 2] = np.nan
    with pytest.raises(ValueError):
        ev.surface_distance(_t(bad), _t(verts), _t(faces))
    v = verts.copy()
    v[faces[7, 1], 0] = np.nan
    with pytest.raises(ValueError):
        ev.surface_distance(_t(pts), _t(v), _t(faces))
    f = faces.copy()
    f[100, 2] = len(verts)
    with pytest.raises(ValueError):
        ev.surface_distance(_t(pts), _t(verts), _t(f))
    f[100, 2] = -1
    with pytest.raises(ValueError):
        ev.surface_distance(_t(pts), _t(verts), _t(f))
    with pytest.raises(ValueError):
        ev.surface_distance(_t(pts), _t(verts), _t(np.zeros((0, 3), np.int32)))
    hit = ev.surface_distance(_t(np.zeros((0, 3))), _t(verts), _t(faces))
    assert tuple(hit.dist.shape) == (0,) and tuple(hit.bary.shape) == (0, 3)


# ---------------------------------------------------------------------------------------------------- 2 sampler
WIDE = (np.array([[0, 0, 0], [2.0 ** -9, 0, 0], [0, 2.0 ** -9, 0], [0, 0, 1], [2, 0, 1], [0, 2, 1]], np.float64),
        np.array([[0, 1, 2], [3, 4, 5]], np.int32))          # areas 2^-19 : 2 = 1 : 2^20


@pytest.mark.parametrize("mesh", ("icosphere", "wide"))
def test_samples_bit_for_bit(mesh):
    verts, faces = _sphere() if mesh == "icosphere" else WIDE
    F = len(faces)
    if mesh == "wide":
        a = ref.face_areas(verts, faces)
        assert a[1] / a[0] == 2.0 ** 20
    for n, seed in ((1, 0), (F, 0), (F + 1, 3), (1000, 2 ** 63 + 5)):
        smp = _ev().sample_surface(_t(verts), _t(faces), n, seed=seed)
        ids, bary, points = ref.sample_surface(verts, faces, n, seed=seed)
        assert smp.face_ids.dtype == torch.int32 and np.array_equal(_n(smp.face_ids), ids)
        assert _same(smp.bary, bary) and _same(smp.points, points)
        assert (np.diff(ids) >= 0).all() and (bary >= 0).all() and (bary.sum(-1) == 1.0).all()
    if mesh == "wide":
        n = 1 << 21
        ids = _n(_ev().sample_surface(_t(verts), _t(faces), n).face_ids)
        assert int((ids == 0).sum()) in (1, 2)                # its share of 2^21 samples is 2^21 / (2^20 + 1)


def test_sampler_errors():
    ev = _ev()
    verts, faces = _sphere()
    flat = np.zeros_like(verts)
    with pytest.raises(ValueError):
        ev.sample_surface(_t(flat), _t(faces), 10)
    with pytest.raises(ValueError):
        ev.sample_surface(_t(verts * 1e200), _t(faces), 10)                  # areas overflow
    with pytest.raises(ValueError):
        ev.sample_surface(_t(verts), _t(np.zeros((0, 3), np.int32)), 10)
    with pytest.raises(ValueError):
        ev.sample_surface(_t(verts), _t(faces), 0)
    f = faces.copy()
    f[3, 0] = len(verts)
    with pytest.raises(ValueError):
        ev.sample_surface(_t(verts), _t(f), 10)


# ---------------------------------------------------------------------------------------------------- 3 mesh against mesh
SQUARE = (np.array([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0]], np.float64), np.array([[0, 1, 2], [0, 2, 3]], np.int32))


def test_lifted_square_is_exactly_its_height_away():
    """Dyadic coordinates and barycentrics: the samples lie exactly in their plane, the closest points' in-plane rounding
    is far below half an ulp of h^2, so every distance is exactly h = 0.25 and every sum of them exact."""
    ev = _ev()
    v, f = SQUARE
    h, n = 0.25, 3000
    up = v + np.array([0, 0, h])
    md, ab, ba = ev.mesh_distance((_t(v), _t(f)), (_t(up), _t(f)), n_samples=n, thresholds=(h, h + 2.0 ** -40), return_samples=True)
    assert (_n(ab.dist) == h).all() and (_n(ba.dist) == h).all()
    assert md.a_to_b.counts == (0, n) and md.b_to_a.counts == (0, n)
    assert md.precision == (0.0, 1.0) and md.recall == (0.0, 1.0) and md.fscore == (0.0, 1.0)
    assert md.chamfer == 0.5 and md.chamfer_sq == 0.125 and md.a_to_b.max == h and md.b_to_a.mean == h
    assert md.n_samples == n and md.thresholds == (h, h + 2.0 ** -40)
    plain = ev.mesh_distance((_t(v), _t(f)), (_t(up), _t(f)), n_samples=n, thresholds=(h, h + 2.0 ** -40))
    assert plain == md


def test_a_mesh_against_itself():
    """A sample is bary_to_point's rounding away from its own face: three products and two sums per coordinate."""
    verts, faces = _sphere()
    n = 5000
    md, ab, ba = _ev().mesh_distance((_t(verts), _t(faces)), (_t(verts), _t(faces)), n_samples=n, return_samples=True)
    bound = 8 * 2.0 ** -53 * np.abs(verts).max()
    print("self distance: max", md.a_to_b.max, md.b_to_a.max, "bound", bound)
    assert md.a_to_b.max <= bound and md.b_to_a.max <= bound
    assert md.precision == (1.0, 1.0) and md.fscore == (1.0, 1.0)


def test_means_maxima_and_counts_against_numpy():
    verts, faces = _sphere()
    other = verts * np.array([1.02, 0.97, 1.0]) + np.array([0.004, 0.0, -0.003])
    n, taus = 20000, (0.004, 0.01, 0.03)
    md, ab, ba = _ev().mesh_distance((_t(verts), _t(faces)), (_t(other), _t(faces)), n_samples=n, thresholds=taus, seed=9,
                                     return_samples=True)
    smp_a = ref.sample_surface(verts, faces, n, seed=9)
    smp_b = ref.sample_surface(other, faces, n, seed=10)
    rows = np.arange(0, n, 97)                                                  # (the whole search in numpy takes too long)
    assert _same(_n(ab.dist)[rows], ref.surface_distance(smp_a[2][rows], other, faces)[0])
    assert _same(_n(ba.dist)[rows], ref.surface_distance(smp_b[2][rows], verts, faces)[0])
    for got, hit in ((md.a_to_b, ab), (md.b_to_a, ba)):
        d = _n(hit.dist)
        s, s2, mx, counts = ref.distance_stats(d, taus)
        print("mean", got.mean, s / n, "mean_sq", got.mean_sq, s2 / n)
        assert abs(got.mean - s / n) <= n * 2.0 ** -52 * (s / n)
        assert abs(got.mean_sq - s2 / n) <= n * 2.0 ** -52 * (s2 / n)
        assert got.max == mx and list(got.counts) == counts
    assert md.chamfer == md.a_to_b.mean + md.b_to_a.mean
    p, r = md.a_to_b.counts[1] / n, md.b_to_a.counts[1] / n
    assert 0 < p < 1 and md.fscore[1] == 2 * p * r / (p + r)


def test_score_frame_and_the_model(tmp_path):
    from gaustar_amd import formats, harness
    verts, faces = _sphere()
    v32 = verts.astype(np.float32)
    formats.save_obj(str(tmp_path / "a.obj"), v32, faces)
    formats.save_obj(str(tmp_path / "b.obj"), v32 * np.float32(1.01), faces)
    md = _ev().score_frame(str(tmp_path / "a.obj"), str(tmp_path / "b.obj"), device=DEV, n_samples=2000, thresholds=(0.02,))
    assert 0.005 < md.a_to_b.mean < 0.011 and md.fscore == (1.0,)
    model = harness.SurfaceGaussians(_t(v32), _t(faces, torch.long), n_gaussians_per_surface_triangle=1, sh_levels=1)
    pts = np.random.default_rng(8).uniform(-1.2, 1.2, size=(20, 3))
    _check_hit(model.surface_distance(_t(pts)), pts, v32.astype(np.float64), faces)
    md2 = model.mesh_distance_to(_t(v32 * np.float32(1.01)), _t(faces), n_samples=2000, thresholds=(0.02,))
    assert md2.n_samples == 2000 and 0.005 < md2.chamfer / 2 < 0.011


# ---------------------------------------------------------------------------------------------------- 4 images
def _pair(shape, seed=0):
    rng = np.random.default_rng(seed)
    return rng.uniform(-0.2, 1.2, size=shape).astype(np.float32), rng.uniform(0, 1, size=shape).astype(np.float32)


@pytest.mark.parametrize("shape", ((3, 1, 1), (3, 7, 5), (3, 64, 64), "strided"))
def test_image_metrics_shapes(shape):
    ev = _ev()
    from gaustar_amd import losses
    if shape == "strided":
        big_p, big_g = _pair((48, 40, 3), seed=3)
        tp, tg = _t(big_p)[5:37, 2:35:2].permute(2, 0, 1), _t(big_g)[5:37, 2:35:2].permute(2, 0, 1)     # [3,32,17], strides (1, 120, 6)
        pred, gt = big_p[5:37, 2:35:2].transpose(2, 0, 1), big_g[5:37, 2:35:2].transpose(2, 0, 1)
        assert not tp.is_contiguous() and tp.stride(2) != 1
    else:
        pred, gt = _pair(shape, seed=sum(shape))
        tp, tg = _t(pred), _t(gt)
    n = pred.size
    for clamp in (False, True):
        im = ev.image_metrics(tp, tg, clamp=clamp)
        sse, count = ref.image_sse(pred, gt, clamp01=clamp)
        print(shape, clamp, "mse", im.mse, sse / n, "psnr", im.psnr)
        assert im.n == count == n
        assert abs(im.mse * n - sse) <= n * 2.0 ** -52 * sse
        assert abs(im.psnr - ref.psnr(sse, n)) <= 1e-9
        want_ssim = float(losses.ssim(tp.clamp(0, 1) if clamp else tp, tg))
        assert im.ssim == want_ssim
    assert ev.image_metrics(tp, tg, clamp=True).mse <= ev.image_metrics(tp, tg, clamp=False).mse


def test_image_metrics_known_values():
    ev = _ev()
    gt = np.full((3, 7, 5), 0.25, np.float32)
    im = ev.image_metrics(_t(gt + np.float32(0.5)), _t(gt))
    assert im.mse == 0.25 and im.psnr == 20 * math.log10(2.0) and im.n == 105
    same = ev.image_metrics(_t(gt), _t(gt))
    assert same.mse == 0.0 and same.psnr == float("inf") and abs(same.ssim - 1.0) <= LOSS_TOL
    # clamp: 1.75 and -3 count as 1 and 0
    hi = ev.image_metrics(_t(gt + np.float32(1.5)), _t(gt))
    assert hi.mse == 0.5625
    lo = ev.image_metrics(_t(gt - np.float32(3.25)), _t(gt), clamp=True)
    assert lo.mse == 0.0625 and ev.image_metrics(_t(gt - np.float32(3.25)), _t(gt), clamp=False).mse == 3.25 ** 2


def test_psnr_against_torch_in_f32():
    """The reference's expression, 20 log10(1 / sqrt(mean((a - b)^2))), in f32 on the host: its sum of n = 3 64 64 terms errs
    by at most (n - 1) 2^-24 relative, which is (10 / ln 10) (n - 1) 2^-24 = 3.2e-3 dB."""
    pred, gt = _pair((3, 64, 64), seed=21)
    im = _ev().image_metrics(_t(pred), _t(gt), clamp=False)
    a, b = torch.from_numpy(pred), torch.from_numpy(gt)
    want = float(20 * torch.log10(1.0 / torch.sqrt(((a - b) ** 2).mean())))
    print("psnr", im.psnr, "torch f32", want)
    assert abs(im.psnr - want) <= 4e-3


def test_image_metrics_mask():
    ev = _ev()
    pred, gt = _pair((3, 64, 64), seed=22)
    mask = np.zeros((64, 64), bool)
    mask[:, ::2] = True
    for m in (_t(mask), _t(mask.astype(np.uint8))):
        im = ev.image_metrics(_t(pred), _t(gt), mask=m)
        sse, count = ref.image_sse(pred, gt, mask=mask, clamp01=True)
        assert im.n == count == 3 * 32 * 64 and im.ssim is None
        assert abs(im.mse * count - sse) <= count * 2.0 ** -52 * sse
    with pytest.raises(ValueError):
        ev.image_metrics(_t(pred), _t(gt), mask=_t(np.zeros((64, 64), bool)))
    with pytest.raises(ValueError):
        ev.image_metrics(_t(pred), _t(gt[:, :32]))


# ---------------------------------------------------------------------------------------------------- 5 binding, views
def test_bind_points_exact_and_default():
    from gaustar_amd import tracking
    verts, faces = _sphere()
    pts = np.random.default_rng(31).uniform(-1.2, 1.2, size=(70, 3))
    ids, bary = tracking.bind_points(_t(verts), _t(faces), _t(pts), exact=True)
    hit = _ev().surface_distance(_t(pts), _t(verts), _t(faces))
    assert torch.equal(ids, hit.face) and _same(bary, _n(hit.bary)) and (_n(bary) >= 0).all()
    want_ids, want_bary = tracking_ref.bind_points(verts, faces, pts)
    for got in (tracking.bind_points(_t(verts), _t(faces), _t(pts)), tracking.bind_points(_t(verts), _t(faces), _t(pts), exact=False)):
        assert np.array_equal(_n(got[0]), want_ids) and _same(got[1], want_bary)
    assert (want_bary < 0).any()                     # the reference's binding is beside its face somewhere; the exact one never


def test_evaluate_views_against_its_own_renders():
    from gaustar_amd import harness, scene
    ev = _ev()
    v, f = scene.icosphere(2, 0.12)
    model = harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), sh_levels=2)
    with torch.no_grad():
        model._sh_coordinates_dc.add_(torch.linspace(-1.0, 1.5, model._sh_coordinates_dc.numel(), device=DEV).view_as(model._sh_coordinates_dc))
    eyes = ((0.0, 0.1, 0.45), (0.45, 0.0, 0.05), (-0.3, 0.2, -0.3), (0.05, -0.42, 0.1))
    cams = [harness.nerf_camera_from_scene(scene.look_at_camera(e, (0.0, 0.0, 0.0), 64, 48, focal_px=60.0)) for e in eyes]
    with torch.no_grad():
        gt = torch.stack([model.render_image_gaussian_rasterizer(c, bg_color=(1.0, 1.0, 1.0)).permute(2, 0, 1).clamp(0, 1) for c in cams])
    assert tuple(gt.shape) == (4, 3, 48, 64) and float(gt.min()) < 0.9
    one = ev.evaluate_views(model, cams, gt, views_in_flight=1)
    two = ev.evaluate_views(model, cams, lambda i: gt[i], views_in_flight=2)
    assert one.psnr.dtype == np.float64 and one.ssim.dtype == np.float32 and one.psnr.shape == one.ssim.shape == (4,)
    assert np.isposinf(one.psnr).all() and one.mean_psnr == float("inf")
    assert np.abs(one.ssim - 1.0).max() <= LOSS_TOL and abs(one.mean_ssim - 1.0) <= LOSS_TOL
    assert np.array_equal(one.psnr, two.psnr) and np.array_equal(one.ssim, two.ssim)
    # against another ground truth: a finite score per view, equal to image_metrics' of the same pair
    grey = torch.full_like(gt, 0.5)
    vm = ev.evaluate_views(model, cams, grey)
    for i in range(4):
        im = ev.image_metrics(gt[i], grey[i])
        assert vm.psnr[i] == im.psnr and abs(float(vm.ssim[i]) - im.ssim) <= LOSS_TOL
    assert np.isfinite(vm.psnr).all() and vm.mean_psnr == float(vm.psnr.mean())
