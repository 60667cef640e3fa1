"""GPU: the density field (gaustar_amd.density, gsr_density.hip) against the numpy restatement (tests/density_ref.py) to at most
1 f32 ulp -- the exponent's argument is the same bits on both sides, both exponentials are within 1 ulp of f64 and the terms
are not negative, so the two f64 sums differ by a few 2^-53 relative and round to equal or adjacent floats --, and what is
built on it: SurfaceGaussians.postprocess_mesh against the restated peel and restore, get_covariance, export_ply."""
import numpy as np
import pytest
import torch

import density_ref as dr
import knn_ref as kr
from gaustar_amd import density, formats, scene
from gaustar_amd.harness import SurfaceGaussians
from gaustar_amd.sweep import ForwardSweep

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
P_ALL = 4096


def _t(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else x, np.float32).view(np.int32)


def _cloud():
    gs = scene.random_gaussians(P_ALL, np.random.default_rng(7))
    return gs.means3D, gs.scales, gs.rotations, gs.opacities[:, 0].copy()


CLOUD = _cloud()


def _gpu(x, P, idx=None, K=16, factor=1.0, cloud=CLOUD):
    pts, s, q, w = (_t(a[:P]) for a in cloud)
    d, t = density.compute_density(_t(x), pts, s, q, w, closest_gaussians_idx=idx, K=K, density_factor=factor,
                                   return_closest_gaussian_opacities=True)
    assert d.dtype == torch.float32 and t.dtype == torch.float32 and tuple(d.shape) == (len(x),) and t.shape[0] == len(x)
    return d.cpu().numpy(), t.cpu().numpy()


def _within_one_ulp(got, want, what):
    u = dr.ulp_diff(got, want)
    print(f"{what}: {int((u != 0).sum())} of {u.size} values differ from the restatement, the largest by {int(u.max()) if u.size else 0} ulp")
    assert u.size == 0 or u.max() <= 1, (what, int(u.max()), np.argwhere(u > 1)[:5])


@pytest.mark.parametrize("K", [1, 15, 16, 17, 32])
def test_sizes(hip_lib, K):
    QW, QG = hip_lib.gsr_density_queries_per_wave(), hip_lib.gsr_density_queries_per_workgroup()
    assert QW == 4 and QG % QW == 0
    rng = np.random.default_rng(100 + K)
    pts, s, q, w = CLOUD
    Qs = [1, QW - 1, QW, QW + 1, QG - 1, QG + 1, 3 * QG + 5]
    for P in sorted({1, K - 1, P_ALL}):
        x = (pts[rng.integers(0, max(P, 1), max(Qs))] + 0.03 * rng.normal(size=(max(Qs), 3))).astype(np.float32)
        if P == 0:
            with pytest.raises(ValueError, match="no Gaussians"):
                _gpu(x[:1], 0, K=K)
            continue
        idx = kr.knn(x, pts[:P], K)[0]
        assert ((idx == -1).sum(1) == max(0, K - P)).all()
        want_d, want_t = dr.density(x, idx, pts[:P], s[:P], q[:P], w[:P])
        if P == P_ALL and K == 16:
            n = (want_t > 0).sum(1)
            print(f"K=16: {n.min()} to {n.max()} of 16 neighbours contribute, densities {want_d.min():.1e} to {want_d.max():.2g}")
        for Q in Qs:
            d, t = _gpu(x[:Q], P, K=K)
            _within_one_ulp(d, want_d[:Q], f"density K={K} P={P} Q={Q}")
            _within_one_ulp(t, want_t[:Q], f"opacities K={K} P={P} Q={Q}")
            assert (t[idx[:Q] == -1] == 0).all()
            # the search's indices and given ones, int64 and int32: the same bits
            for given in (_t(idx[:Q], np.int64), _t(idx[:Q], np.int32)):
                d2, t2 = _gpu(x[:Q], P, idx=given)
                assert np.array_equal(_bits(d), _bits(d2)) and np.array_equal(_bits(t), _bits(t2)), (K, P, Q)
            # and again: bit-reproducible across calls
            d3, t3 = _gpu(x[:Q], P, K=K)
            assert np.array_equal(_bits(d), _bits(d3)) and np.array_equal(_bits(t), _bits(t3))


def test_density_only_equals_the_first_of_the_pair():
    pts, s, q, w = CLOUD
    x = (pts[:37] + np.float32(0.02)).astype(np.float32)
    d_only = density.compute_density(_t(x), _t(pts), _t(s), _t(q), _t(w)[:, None])          # strengths [P,1], K = 16
    assert isinstance(d_only, torch.Tensor) and np.array_equal(_bits(d_only), _bits(_gpu(x, P_ALL)[0]))


def test_values():
    one = [1, 0, 0, 0]
    # Gaussian 0: a scale of 0, 1: a scale of 1e-9, 2: plain, 3: strength 0, 4: an all-zero quaternion, 5: thin, for the far query
    pts = np.float32([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 0], [5, 5, 5]])
    s = np.float32([[0, 0.2, 0.2], [1e-9, 0.2, 0.2], [0.1, 0.2, 0.3], [0.1, 0.1, 0.1], [0.1, 0.1, 0.1], [0.01, 1, 1]])
    q = np.float32([one, one, [0.3, -0.5, 0.7, 0.2], one, [0, 0, 0, 0], one])
    w = np.float32([0.9, 0.8, 0.7, 0.0, 0.6, 0.5])
    cloud = (pts, s, q, w)
    x = np.float32([[1e-8, 0.05, 0], [1 + 2e-8, 0, 0.05], [0.05, 1.02, 0.01], [0, 0, 1.01], [1, 1, 0.01], [1005, 5, 5],
                    [np.nan, 0, 0], [0.5, 0.5, 0.5]])
    idx = np.array([[0, -1, -1], [1, -1, -1], [2, -1, -1], [3, -1, -1], [4, -1, -1], [5, -1, -1], [2, 0, -1], [2, 0, 1]])
    for factor in (1.0, 0.5):
        want_d, want_t = dr.density(x, idx, pts, s, q, w, factor)
        d, t = _gpu(x, 6, idx=_t(idx, np.int64), factor=factor, cloud=cloud)
        _within_one_ulp(d, want_d, f"values, factor {factor}: density")
        _within_one_ulp(t, want_t, f"values, factor {factor}: opacities")
        assert d[3] == 0 and d[5] == 0 and t[5, 0] == 0          # strength 0; m at 1e8: exactly 0
        assert np.isnan(d[4]) and np.isnan(d[6]) and np.isnan(t[6, 0]) and np.isnan(t[6, 1]) and t[6, 2] == 0
        assert d[0] > 0 and d[1] > 0 and np.isfinite(d[:4]).all()
    d1, d5 = _gpu(x, 6, idx=_t(idx, np.int64), cloud=cloud)[0], _gpu(x, 6, idx=_t(idx, np.int64), factor=0.5, cloud=cloud)[0]
    assert np.array_equal(d5[[0, 1, 2, 7]], np.float32(0.5) * d1[[0, 1, 2, 7]])      # (halving is exact)
    # without given indices a query that is not finite has an empty row, as the search gives it: nothing is summed
    want_idx = kr.knn(x, pts, 3)[0]
    assert (want_idx[6] == -1).all()
    want_d, want_t = dr.density(x, want_idx, pts, s, q, w)
    d, t = _gpu(x, 6, K=3, cloud=cloud)
    _within_one_ulp(d, want_d, "values, searched: density")
    _within_one_ulp(t, want_t, "values, searched: opacities")
    assert d[6] == 0 and (t[6] == 0).all()


def test_what_is_refused():
    pts, s, q, w = (_t(a[:50]) for a in CLOUD)
    x = pts[:5].clone()
    for bad in (50, -2, 2 ** 32 + 3):
        idx = torch.zeros(5, 4, dtype=torch.int64, device=DEV)
        idx[3, 2] = bad
        with pytest.raises(ValueError, match="outside"):
            density.compute_density(x, pts, s, q, w, closest_gaussians_idx=idx)
    with pytest.raises(ValueError, match="K = 33"):
        density.compute_density(x, pts, s, q, w, K=33)
    with pytest.raises(ValueError, match="K = 33"):
        density.compute_density(x, pts, s, q, w, closest_gaussians_idx=torch.zeros(5, 33, dtype=torch.int32, device=DEV))
    with pytest.raises(ValueError, match="float32"):
        density.compute_density(x.double(), pts, s, q, w)
    with pytest.raises(ValueError, match="strengths"):
        density.compute_density(x, pts, s, q, w[:49])
    empty = density.compute_density(x[:0], pts, s, q, w)
    assert tuple(empty.shape) == (0,)


# ------------------------------------------------------------------------------------------------ the model's methods
def _shell(level, cut, G=6, loose=False, seed=0):
    """An icosphere without the faces whose centre is above y = 1.2 + cut (cut=None: closed), with G Gaussians per face, faint
    opacities and parameters that differ from row to row."""
    v, f = scene.icosphere(level, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    v = v.astype(np.float32)
    if cut is not None:
        f = f[v[f].mean(1)[:, 1] <= 1.2 + cut]
    rng = np.random.default_rng(seed)
    m = SurfaceGaussians(_t(v), _t(f, np.int64), n_gaussians_per_surface_triangle=G, loose_bind=loose)
    N = len(f) * G
    op = rng.uniform(0.001, 0.1, (N, 1))
    with torch.no_grad():
        m.all_densities.copy_(_t(np.log(op / (1 - op))))
        m._scales.add_(_t(0.05 * rng.normal(size=(N, 2))))
        a = rng.uniform(-0.3, 0.3, N)
        m._quaternions.copy_(_t(np.stack([np.cos(a), np.sin(a)], 1)))
        m._sh_coordinates_dc.copy_(_t(rng.normal(size=(N, 1, 3))))
        m._sh_coordinates_rest.copy_(_t(rng.normal(size=(N, 15, 3))))
        if loose:
            m._delta_t.copy_(_t(1e-3 * rng.normal(size=(N, 3))))
    return m, v, f


def _restated(m, v, f, iterations, threshold, K=16):
    n = lambda t: t.detach().cpu().numpy()
    return dr.postprocess(v, f, n(m.points), n(m.scaling), n(m.quaternions), n(m.strengths), iterations, threshold, K,
                          lambda q, c, K: kr.knn(q, c, K)[0])


def _check_postprocess(m, v, f, res, want):
    mask, kept, restored, _ = want
    G, F = m.n_gaussians_per_surface_triangle, len(f)
    assert res.face_mask.dtype == torch.bool and np.array_equal(res.face_mask.cpu().numpy(), mask)
    assert res.kept_per_iteration == kept and res.restored == restored
    new = res.model
    assert torch.equal(new._points, m._points) and torch.equal(new._surface_mesh_faces, m._surface_mesh_faces[res.face_mask])
    for name in ("_scales", "_quaternions", "all_densities", "_sh_coordinates_dc", "_sh_coordinates_rest"):
        old = getattr(m, name).detach()
        rows = old.reshape(F, G, *old.shape[1:])[res.face_mask].reshape(-1, *old.shape[1:])
        assert getattr(new, name).shape == rows.shape and np.array_equal(_bits(getattr(new, name)), _bits(rows)), name
    assert new.n_gaussians_per_surface_triangle == G and new.sh_levels == m.sh_levels and not new.is_loose_bind()
    assert torch.equal(new.surface_mesh_thickness, m.surface_mesh_thickness)
    assert (new.min_gaussian_scale, new.max_gaussian_scale) == (m.min_gaussian_scale, m.max_gaussian_scale)


@pytest.mark.parametrize("level,cut", [(2, 0.3), (3, 0.5)])
def test_thin_shell(level, cut):
    m, v, f = _shell(level, cut)
    want = _restated(m, v, f, 5, 0.1)
    mask, kept, restored, dens = want
    removed = int((~dr.peel(f, 5)[0]).sum())
    margin = np.abs(dens.astype(np.float64) - 0.1).min() / 0.1
    print(f"level {level}: {len(f)} faces, {removed} removed, {restored} restored, kept {kept}, closest density {margin:.1e} relative")
    assert margin > 1e-5                     # the condition: no removed centre decides within rounding of the threshold
    assert 0 < restored < removed            # both outcomes occur
    _check_postprocess(m, v, f, m.postprocess_mesh(5, 0.1), want)
    # the model's own compute_density at the removed centres, with and without given indices
    c = dr.face_centres(v, f)[~dr.peel(f, 5)[0]]
    got = m.compute_density(_t(c))
    _within_one_ulp(got.cpu().numpy(), dens, "removed centres")
    assert m.knn_to_track == 16
    idx = m.get_gaussians_closest_to_samples(_t(c))
    assert idx.dtype == torch.int64 and np.array_equal(idx.cpu().numpy(), kr.knn(c, m.points.detach().cpu().numpy(), 16)[0])
    assert np.array_equal(_bits(m.compute_density(_t(c), closest_gaussians_idx=idx)), _bits(got))
    # the reference's own f32 composition (sugar_model.py:1024-1035) agrees to f32 rounding.  The thin axis divides by the
    # thickness, 1e-6: the f32 rounding of a shift of 0.02 and of its rotation, some 1e-9, becomes 1e-3 in w, which is below
    # 0.1 there, so 2e-4 in m and 1e-4 relative in a term; the in-plane axes add 1e-6 relative per operation
    with torch.no_grad():
        x = _t(c)
        inv = m.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)[idx]
        shift = x[:, None] - m.points[idx]
        ws = (inv.transpose(-1, -2) @ shift[..., None])[..., 0]
        comp = (m.strengths[idx][..., 0] * torch.exp(-0.5 * (ws * ws).sum(-1).clamp(min=0., max=1e8))).sum(-1)
    torch.testing.assert_close(got, comp, rtol=1e-3, atol=1e-6)


def test_postprocess_edge_cases():
    m, v, f = _shell(2, 0.3)
    res = m.postprocess_mesh(0, 0.1)                                  # no peel: nothing removed
    assert res.face_mask.all() and res.kept_per_iteration == [] and res.restored == 0
    _check_postprocess(m, v, f, res, (np.ones(len(f), bool), [], 0, None))
    m, v, f = _shell(2, None)                                         # closed: no border
    res = m.postprocess_mesh(5, 0.1)
    assert res.face_mask.all() and res.kept_per_iteration == [len(f)] * 5 and res.restored == 0
    m, v, f = _shell(2, 0.3, G=1, seed=1)                             # one Gaussian per triangle
    _check_postprocess(m, v, f, m.postprocess_mesh(3, 0.05), _restated(m, v, f, 3, 0.05))
    _check_postprocess(m, v, f, m.postprocess_mesh(2, 0.05, K=4), _restated(m, v, f, 2, 0.05, K=4))
    m, v, f = _shell(2, 0.3, loose=True, seed=2)                      # loose-bound in, bound out
    assert m.is_loose_bind()
    res = m.postprocess_mesh(5, 0.1)
    _check_postprocess(m, v, f, res, _restated(m, v, f, 5, 0.1))
    assert getattr(res.model, "_delta_t", None) is None
    with pytest.raises(ValueError, match="no face is left"):          # a threshold nothing passes, a peel that takes all
        tri = SurfaceGaussians(_t(v[f[0]]), _t([[0, 1, 2]], np.int64))
        tri.postprocess_mesh(1, 1e9)


def test_get_covariance_forms():
    m, _, _ = _shell(2, 0.3)
    from gaustar_amd import producers
    with torch.no_grad():
        s, R = m.scaling, producers.quaternion_to_matrix(m.quaternions)
        for inverse in (False, True):
            sc = 1. / s.clamp(min=1e-8) if inverse else s
            sr = R * sc[:, None]
            full = sr @ sr.transpose(-1, -2)
            assert torch.equal(m.get_covariance(return_sqrt=True, inverse_scales=inverse), sr)
            assert torch.equal(m.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=inverse), sr)
            got = m.get_covariance(return_full_matrix=True, inverse_scales=inverse)
            torch.testing.assert_close(got, full, rtol=1e-6, atol=0)
            six = m.get_covariance(inverse_scales=inverse)
            assert tuple(six.shape) == (m.n_points, 6)
            torch.testing.assert_close(six, torch.stack([full[:, 0, 0], full[:, 0, 1], full[:, 0, 2], full[:, 1, 1], full[:, 1, 2],
                                                         full[:, 2, 2]], -1), rtol=1e-6, atol=0)
        # the columns are the scaled axes: the form compute_density's (R diag(1 / s))^T d stands for
        assert torch.equal(m.get_covariance(return_sqrt=True)[:, :, 1], R[:, :, 1] * s[:, 1:2])


def test_export_ply(tmp_path):
    m, _, _ = _shell(2, 0.3)
    path = str(tmp_path / "point_cloud.ply")
    m.export_ply(path)
    cloud = formats.load_ply(path)
    with torch.no_grad():
        for got, want in ((cloud.xyz, m.points), (cloud.opacity, m.all_densities), (cloud.features_dc, m._sh_coordinates_dc),
                          (cloud.features_rest, m._sh_coordinates_rest), (cloud.rotation, m.quaternions),
                          (cloud.scaling, torch.log(m.scaling))):
            assert got.shape == tuple(want.shape) and np.array_equal(_bits(got), _bits(want))
    assert cloud.sh_degree == m.sh_levels - 1
    ri = cloud.rasterizer_inputs()
    sweep = ForwardSweep(_t(ri["means3D"]), _t(ri["opacities"]), _t(ri["scales"]), _t(ri["rotations"]), sh=_t(ri["shs"]),
                         sh_levels=m.sh_levels)
    cam = scene.look_at_camera((0.5, 1.6, 3.0), scene.SUBJECT_CENTER, 64, 64, focal_px=60.0)
    rgb, depth = sweep.render_rgb_depth(cam)
    assert tuple(rgb.shape) == (64, 64, 3) and tuple(depth.shape) == (64, 64) and torch.isfinite(rgb).all()
