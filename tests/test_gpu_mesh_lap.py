"""GPU: the fused mesh Laplacian-smoothing loss and small-area regulariser (gsr_mesh_lap_forward / _backward,
losses.mesh_smoothness_loss, meshes.mesh_laplacian_smoothing, SurfaceGaussians.rgbd_step(mesh_reg=dict(laplacian_factor=...)))
against closed forms, an f64 torch restatement of the definitions in include/gsr.h (tests/mesh_lap_ref.py) run on the device
with the same f32 positions, invariances of the gradient, and the autograd composition of a refinement iteration."""
import math

import numpy as np
import pytest
import torch

import mesh_lap_ref as ml
import mesh_reg_ref as mr
from gaustar_amd.losses import mesh_smoothness_loss          # noqa: F401  (the op under test)
from gaustar_amd.meshes import mesh_laplacian_smoothing      # noqa: F401

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")

MESHES = {"icosphere2": lambda: mr.icosphere(2, noise=0.2), "grid": lambda: mr.grid(6, noise=0.05),
          "non_manifold": mr.non_manifold, "degenerate": mr.degenerate,
          "icosphere4": lambda: mr.icosphere(4, noise=0.3)}
TETRAHEDRON = {"uniform": 4.0 * math.sqrt(3.0) / 3.0, "cot": 4.0 * math.sqrt(3.0) / 3.0, "cotcurv": math.sqrt(3.0) / 9.0}
_CACHE = {}


def _mesh(name):
    """(f32 positions, faces) of a named mesh on the device, made once."""
    if ("mesh", name) not in _CACHE:
        v, f = MESHES[name]() if name in MESHES else name()
        _CACHE[("mesh", name)] = (torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).to(DEV))
    return _CACHE[("mesh", name)]


def _restated(name, lap, method, areg):
    """The f64 restatement on the device over the same f32 positions, computed once per case and left unchanged."""
    key = ("ref", name, lap, method, areg)
    if key not in _CACHE:
        v, f = _mesh(name)
        _CACHE[key] = ml.smoothness(v.double(), f, lap, method, areg)
    return _CACHE[key]


def _fused(v32, f, lap=1.0, method="uniform", areg=0.0, upstream=1.0):
    from gaustar_amd import losses, meshes
    topo = meshes.MeshTopology.of(f, v32.shape[0])
    x = v32.detach().clone().requires_grad_(True)
    loss, parts = losses.mesh_smoothness_loss(x, topo, lap, method, areg, return_parts=True)
    loss.backward(torch.tensor(upstream, device=DEV))
    return loss.detach(), parts, x.grad


def _grad_err(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.abs().max()), 1e-30))


@pytest.mark.parametrize("method", ml.METHODS)
def test_tetrahedron_closed_forms(method, hip_lib):
    v, f = mr.tetrahedron()
    v, f = torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).to(DEV)
    factor = 3.0
    loss, parts, grad = _fused(v, f, factor, method)
    p = parts.cpu().tolist()
    want = factor * TETRAHEDRON[method]
    print(method, p, want)
    assert abs(p[0] - want) <= 2e-6 * want and p[1] == 0.0 and p[2] == p[0] and float(loss) == p[2], (p, want)
    assert torch.isfinite(grad).all()


@pytest.mark.parametrize("name", sorted(MESHES))
@pytest.mark.parametrize("method", ml.METHODS)
def test_against_f64_restatement(method, name, hip_lib):
    """Value within 1e-5 relative, gradient within 1e-4 of its largest magnitude (the bounds of tests/test_gpu_mesh_reg.py).
    The small meshes: one workgroup, boundary edges with one face, an edge with three faces, an unreferenced vertex, clamped
    Heron areas; icosphere4 (V = 2 562): several workgroups and partials."""
    v, f = _mesh(name)
    loss, parts, g = _fused(v, f, 1.0, method)
    want, gw = _restated(name, 1.0, method, 0.0)
    print(name, method, "value rel err", abs(float(loss) - float(want)) / abs(float(want)), "grad err", _grad_err(g, gw))
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    assert torch.isfinite(g).all()
    assert _grad_err(g, gw) <= 1e-4, _grad_err(g, gw)


def test_value_beyond_the_grid_stride_cap(hip_lib):
    """icosphere(8): V = 655 362 vertices, more than the 2 048 workgroups of 256 of the vertex pass take in one stride."""
    v, f = _mesh(lambda: mr.icosphere(8, noise=0.2))
    assert v.shape[0] == 655362 > 2048 * 256
    from gaustar_amd import losses, meshes
    loss = losses.mesh_smoothness_loss(v, meshes.MeshTopology.of(f, v.shape[0]), 1.0, "uniform")
    want = float(ml.laplacian_loss(v.double(), f, "uniform"))
    print("icosphere8 value rel err", abs(float(loss) - want) / want)
    assert abs(float(loss) - want) <= 1e-5 * want, (float(loss), want)


@pytest.mark.parametrize("name", ["non_manifold", "degenerate"])
def test_unreferenced_vertex(name, hip_lib):
    """Vertex 6 has no edge: l = -v, so the loss holds |v| / V and the gradient is (1 / V) d u = (1 / V) v / |v| (d = -1,
    u = -v / |v|): the vertex is pulled to the origin, as in pytorch3d.  cotcurv gives it the weight 0: exactly no gradient."""
    v, f = _mesh(name)
    V = v.shape[0]
    want = v[6].double() / v[6].double().norm() / V
    for method in ("uniform", "cot"):
        g = _fused(v, f, 1.0, method)[2][6].double()
        assert float((g - want).abs().max()) <= 2.0 ** -23 * float(want.abs().max()), (method, g, want)
    assert torch.equal(_fused(v, f, 1.0, "cotcurv")[2][6], torch.zeros(3, device=DEV))


@pytest.mark.parametrize("name", ["icosphere2", "icosphere4"])
def test_area_regulariser_against_f64_restatement(name, hip_lib):
    v, f = _mesh(name)
    loss, parts, g = _fused(v, f, 0.0, "uniform", 1.0)
    want, gw = _restated(name, 0.0, "uniform", 1.0)
    p = parts.cpu().tolist()
    print(name, "area_reg", float(loss), float(want), "grad err", _grad_err(g, gw))
    assert float(want) > 0.0                                   # some faces are below half the mean area
    assert p[0] == 0.0 and p[1] == p[2] == float(loss)
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    assert _grad_err(g, gw) <= 1e-4, _grad_err(g, gw)


def _two_flat_faces():
    """`degenerate` with one more collinear face, (1, 7, 8): vertex 8 is touched by a zero-area face only."""
    v, f = mr.degenerate()
    v[5] = 0.5 * (v[1] + v[2]) + [0.05, 0.05, 0.02]     # face (1, 5, 2) becomes a sliver: below half the mean area
    return np.vstack([v, [[3, 0, 0]]]), np.vstack([f, [[1, 7, 8]]])


def test_area_regulariser_on_zero_area_faces(hip_lib):
    v, f = _mesh("degenerate")
    loss, _, g = _fused(v, f, 0.0, "uniform", 1.0)
    assert float(loss) == math.inf and torch.isfinite(g).all()
    assert _grad_err(g, ml.area_reg_grad(v.double(), f)) <= 1e-4      # (no other face is below half the mean: all 0)
    v, f = _mesh(_two_flat_faces)
    loss, _, g = _fused(v, f, 0.0, "uniform", 1.0)
    assert float(loss) == math.inf and torch.isfinite(g).all()
    assert torch.equal(g[8], torch.zeros(3, device=DEV))        # touched only by a zero-area face: exactly 0
    gw = ml.area_reg_grad(v.double(), f)
    assert float(gw.abs().max()) > 0.0 and _grad_err(g, gw) <= 1e-4, _grad_err(g, gw)


def test_gradient_invariances(hip_lib):
    """cotcurv and the area regulariser are translation invariant (uniform and cot carry -v_i and are not); the area
    regulariser is rotation invariant too."""
    v, f = _mesh("icosphere4")
    x = v.double()
    for kw in (dict(lap=1.0, method="cotcurv"), dict(lap=0.0, areg=1.0)):
        g = _fused(v, f, **kw)[2].double()
        tot = float(g.abs().sum())
        assert tot > 0.0
        assert float(g.sum(0).abs().max()) <= 1e-5 * tot, kw
        if kw["lap"] == 0.0:
            assert float(torch.linalg.cross(x, g, dim=1).sum(0).abs().max()) <= 1e-5 * tot      # |x| ~ 1


@pytest.mark.parametrize("method", ml.METHODS)
def test_backward_is_deterministic_accumulates_and_scales_on_device(method, hip_lib):
    from gaustar_amd import harness, losses, meshes
    v, f = _mesh("icosphere4")
    topo = meshes.MeshTopology.of(f, v.shape[0])
    ctx = harness._PlainCtx((True,) + (False,) * 4)
    l0, p0 = losses._MeshSmoothnessLoss.forward(ctx, v, topo, 5.0, method, 0.1)
    one = torch.ones((), device=DEV)
    a = losses._MeshSmoothnessLoss.grad_into(ctx, one, torch.empty_like(v), 0).clone()
    b = losses._MeshSmoothnessLoss.grad_into(ctx, one, torch.full_like(v, float("nan")), 0)
    assert torch.equal(a, b) and float(a.abs().max()) > 0.0
    ctx2 = harness._PlainCtx((True,) + (False,) * 4)
    l1, p1 = losses._MeshSmoothnessLoss.forward(ctx2, v, topo, 5.0, method, 0.1)
    assert torch.equal(p0, p1) and torch.equal(l0, l1)
    assert torch.equal(losses._MeshSmoothnessLoss.grad_into(ctx2, one, torch.empty_like(v), 0), a)
    X = torch.randn(v.shape, device=DEV)
    acc = losses._MeshSmoothnessLoss.grad_into(ctx, one, X.clone(), 1)
    assert torch.equal(acc, X + a)
    s = torch.tensor(-0.5, device=DEV)                 # a power of two: exact
    assert torch.equal(losses._MeshSmoothnessLoss.grad_into(ctx, s, torch.empty_like(v), 0), a * s)
    # through autograd: the upstream gradient is the device scale
    _, parts, g = _fused(v, f, 5.0, method, 0.1, upstream=-0.5)
    assert torch.equal(g, a * s) and torch.equal(parts, p0)
    # the parts: each term alone gives its part, and a term whose factor is 0 is 0.0
    only_lap = _fused(v, f, 5.0, method, 0.0)[1].cpu().tolist()
    only_areg = _fused(v, f, 0.0, method, 0.1)[1].cpu().tolist()
    p = p0.cpu().tolist()
    assert only_lap == [p[0], 0.0, p[0]] and only_areg == [0.0, p[1], p[1]]
    assert p[2] == float(np.float32(p[0]) + np.float32(p[1]))


@pytest.mark.parametrize("method", ml.METHODS)
def test_meshes_shim_equals_fused_call(method, hip_lib):
    """refine.py:681-683 after the import swap: meshes.mesh_laplacian_smoothing(Meshes([v], [f]), method)."""
    from gaustar_amd import meshes
    v, f = _mesh("icosphere2")
    points = v.clone().requires_grad_(True)
    loss = meshes.mesh_laplacian_smoothing(meshes.Meshes(verts=[points], faces=[f]), method)
    loss.backward()
    fused, _, g = _fused(v, f, 1.0, method)
    assert torch.equal(loss.detach(), fused) and torch.equal(points.grad, g)


def _small_model():
    from gaustar_amd import harness, scene
    v, f = scene.icosphere(3, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    model = harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), 6, 3).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(4)
    with torch.no_grad():
        model._sh_coordinates_dc.copy_(torch.rand(model.n_points, 1, 3, device=DEV, generator=g) * 2 - 1)
        model._sh_coordinates_rest.copy_(torch.randn(model._sh_coordinates_rest.shape, device=DEV, generator=g) * 0.1)
    ref_mesh = model.surface_mesh
    ve = ref_mesh.verts_packed().detach()[ref_mesh.edges_packed()]
    ref_edge_len = (ve[:, 0] - ve[:, 1]).norm(dim=1) * 0.98
    ref_area = ref_mesh.faces_areas_packed().detach() * 0.95
    with torch.no_grad():
        model._points.add_(0.01 * torch.randn(model._points.shape, device=DEV, generator=g))
    cam = harness.nerf_camera_from_scene(scene.ring_cameras(5, 32, 320, 240, focal_px=200.0)[37])
    bg4 = torch.tensor([0.0, 1.0, 0.0, 10.0], device=DEV)
    gt_rgb = torch.rand(3, 240, 320, device=DEV, generator=g)
    gt_d = torch.rand(240, 320, device=DEV, generator=g) * 12.0
    reg = dict(nc_factor=0.5, ref_edge_len=ref_edge_len, edge_factor=1000.0, ref_area=ref_area, area_factor=5000.0)
    return model, cam, bg4, gt_rgb, gt_d, reg


SMOOTH = dict(laplacian_factor=5.0, laplacian_method="uniform", area_reg_factor=0.1)


def test_rgbd_step_with_smoothness_equals_the_autograd_iteration(hip_lib):
    """rgbd_step(mesh_reg=dict(..., laplacian_factor=..., area_reg_factor=...)) = (rgb_depth_loss(render_channels(...)) +
    surface_mesh_loss(...) + mesh_smoothness_loss(...)).backward(): the loss bit for bit, gradients up to the order of the
    rasterizer backward's float atomics (as tests/test_gpu_mesh_reg.py)."""
    from gaustar_amd import losses
    model, cam, bg4, gt_rgb, gt_d, reg = _small_model()
    params = [p for p in model.parameters() if p.requires_grad]
    topo = model.mesh_topology()
    img = model.render_channels(cam, bg4, depth_channels=1)[0]
    smooth = losses.mesh_smoothness_loss(model._points, topo, 5.0, "uniform", 0.1)
    loss = losses.rgb_depth_loss(img, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5) + losses.surface_mesh_loss(
        model._points, topo, **reg) + smooth
    loss.backward()
    ref = [None if p.grad is None else p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    loss2, img2, _ = model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=dict(reg, **SMOOTH))
    assert float(smooth.detach()) > 0.0
    assert float(loss2) == float(loss.detach()) and torch.equal(img2, img.detach())
    for p, r in zip(params, ref):
        assert (p.grad is None) == (r is None)
        if r is not None and r.numel():
            assert torch.allclose(p.grad, r, rtol=2e-4, atol=1e-4 * float(r.abs().max()) + 1e-9), float((p.grad - r).abs().max())
    # the new terms' share of the vertex gradient is there: without them, _points.grad differs by the fused node's gradient
    g_with = model._points.grad.clone()
    for p in params:
        p.grad = None
    loss3, _, _ = model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=reg)
    _, _, g_smooth = _fused(model._points.detach(), model._surface_mesh_faces, 5.0, "uniform", 0.1)
    assert float(loss2) > float(loss3) and float(g_smooth.abs().max()) > 0.0
    g_without = model._points.grad
    # (two renders: their vertex gradients differ by the backward blend's float-atomic order, 1e-4 of the largest each)
    assert torch.allclose(g_with - g_without, g_smooth, rtol=1e-3, atol=2e-4 * float(g_without.abs().max()) + 1e-9)
    # a device scale reaches the new terms' gradient too
    for p in params:
        p.grad = None
    model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, grad_scale=torch.tensor(-0.5, device=DEV),
                    mesh_reg=dict(reg, **SMOOTH))
    assert torch.allclose(model._points.grad, -0.5 * g_with, rtol=2e-4, atol=1e-4 * float(g_with.abs().max()) + 1e-9)


def test_rgbd_step_without_the_new_keys_is_the_step_as_it_was(hip_lib, monkeypatch):
    """Without laplacian_factor / area_reg_factor (or with both 0) the step launches nothing of the new op and returns the
    same loss and image bit for bit.  The parameter gradients pass through the backward blend's float atomics, whose order
    differs from one run to the next, so they are compared as tests/test_gpu_mesh_reg.py compares two runs of the step."""
    from gaustar_amd import losses
    calls = []
    fwd = losses._MeshSmoothnessLoss.forward
    monkeypatch.setattr(losses._MeshSmoothnessLoss, "forward", staticmethod(lambda *a, **k: (calls.append(1), fwd(*a, **k))[1]))
    model, cam, bg4, gt_rgb, gt_d, reg = _small_model()
    params = [p for p in model.parameters() if p.requires_grad]
    out = []
    for mesh_reg in (reg, dict(reg, laplacian_factor=0.0, area_reg_factor=0.0), None):
        for p in params:
            p.grad = None
        loss, img, _ = model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=mesh_reg)
        out.append((loss, img, [None if p.grad is None else p.grad.clone() for p in params]))
    assert not calls
    (l0, i0, g0), (l1, i1, g1), (l2, i2, _g2) = out
    assert torch.equal(l0, l1) and torch.equal(i0, i1) and torch.equal(i0, i2) and float(l0) > float(l2)
    for a, b in zip(g0, g1):
        assert (a is None) == (b is None)
        if a is not None and a.numel():
            assert torch.allclose(a, b, rtol=2e-4, atol=1e-4 * float(a.abs().max()) + 1e-9)
    # with a key on, the op runs once per step
    model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=dict(reg, **SMOOTH))
    assert len(calls) == 1
    with pytest.raises(ValueError, match="Method should be one of"):
        model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=dict(reg, laplacian_factor=1.0, laplacian_method="cotan"))
