"""GPU: the fused surface-mesh regularisers (gsr_mesh_reg_forward / _backward, losses.surface_mesh_loss, meshes.Meshes /
mesh_normal_consistency, SurfaceGaussians.rgbd_step(mesh_reg=...)) against closed forms, invariances of the gradient, an f64
torch restatement of pytorch3d's algorithm (tests/mesh_reg_ref.py) and the autograd composition refine.py:681-706 builds."""
import math

import numpy as np
import pytest
import torch

import mesh_reg_ref as mr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTORS = dict(nc_factor=0.5, edge_factor=1000.0, area_factor=5000.0)   # train_seq.py:108-110


def _mesh(mk):
    v, f = mk()
    return torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)


def _refs(v64, f, seed=0):
    """Reference edge lengths / areas: the mesh's own, each scaled by a random factor in [0.8, 1.2]."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    edges, _ = mr.p3d_edges(f, v64.shape[0])
    ve = v64[edges]
    re = (ve[:, 0] - ve[:, 1]).norm(dim=1) * (0.8 + 0.4 * torch.rand(len(edges), generator=g, dtype=torch.float64)).to(DEV)
    fv = v64[f]
    ra = 0.5 * torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1)
    ra = ra * (0.8 + 0.4 * torch.rand(len(f), generator=g, dtype=torch.float64)).to(DEV)
    return re, ra


def _fused(v32, f, re=None, ra=None, nc_factor=0.5, edge_factor=1000.0, area_factor=5000.0, upstream=1.0):
    from gaustar_amd import losses, meshes
    topo = meshes.MeshTopology.of(f, v32.shape[0])
    x = v32.detach().clone().requires_grad_(True)
    loss, parts = losses.surface_mesh_loss(x, topo, nc_factor, None if re is None else re.float(), edge_factor,
                                           None if ra is None else ra.float(), area_factor, return_parts=True)
    loss.backward(torch.tensor(upstream, device=DEV))
    return loss.detach(), parts, x.grad


def _restated(v64, f, re=None, ra=None, nc_factor=0.5, edge_factor=1000.0, area_factor=5000.0):
    x = v64.detach().clone().requires_grad_(True)
    t = mr.ref_terms(x, f, re, ra)
    loss = nc_factor * mr.p3d_normal_consistency(x, f)
    if re is not None:
        loss = loss + edge_factor * t["edge"]
    if ra is not None:
        loss = loss + area_factor * t["area"]
    loss.backward()
    return loss.detach(), x.grad


def _grad_err(a, b):
    return float((a.double() - b.double()).abs().max() / max(float(b.abs().max()), 1e-30))


@pytest.mark.parametrize("name", sorted(mr.CLOSED_FORM_NC))
def test_normal_consistency_closed_forms(name, hip_lib):
    mk, want = mr.CLOSED_FORM_NC[name]
    v, f = _mesh(mk)
    loss, parts, grad = _fused(v.float(), f, nc_factor=1.0)
    p = parts.cpu().tolist()
    assert abs(p[0] - want) <= 2e-6 and p[1] == 0.0 and p[2] == 0.0 and abs(float(loss) - want) <= 2e-6, (p, want)
    assert torch.isfinite(grad).all()


def test_edge_and_area_terms_exact_on_a_scaled_tetrahedron(hip_lib):
    v, f = _mesh(mr.tetrahedron)
    edges, _ = mr.p3d_edges(f, 4)
    re = (v[edges[:, 0]] - v[edges[:, 1]]).norm(dim=1)               # 2 sqrt(2)
    fv = v[f]
    ra = 0.5 * torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1)   # 2 sqrt(3)
    s = 1.5
    loss, parts, _ = _fused((s * v).float(), f, re, ra, nc_factor=0.25, edge_factor=3.0, area_factor=7.0)
    p = parts.cpu().tolist()
    want = [0.25 * 4.0 / 3.0, 3.0 * 8.0 * (s - 1) ** 2, 7.0 * 2.0 * math.sqrt(3.0) * (s * s - 1)]
    for got, w in zip(p[:3], want):
        assert abs(got - w) <= 2e-6 * abs(w), (p, want)
    assert abs(p[3] - sum(want)) <= 4e-6 * sum(want) and float(loss) == p[3]


def test_gradient_invariances_config_c_mesh(hip_lib):
    v0, f = _mesh(lambda: mr.icosphere(6))
    re, ra = _refs(v0, f, seed=1)
    v, _ = _mesh(lambda: mr.icosphere(6, noise=0.3, seed=2))
    assert v.shape[0] == 40962
    for kw in (dict(FACTORS), dict(nc_factor=1.0, edge_factor=0.0, area_factor=0.0)):
        _, _, g = _fused(v.float(), f, re, ra, **kw)
        g, x = g.double(), v.float().double()
        tot = float(g.abs().sum())
        assert float(g.sum(0).abs().max()) <= 1e-5 * tot                                     # translation
        assert float(torch.linalg.cross(x, g, dim=1).sum(0).abs().max()) <= 1e-5 * tot      # rotation (|x| ~ 1)
        if kw["edge_factor"] == 0.0:
            assert abs(float((x * g).sum())) <= 1e-5 * tot                                  # scale: NC alone


def _twice(mk):
    """Two disjoint copies of a mesh, the second's vertex indices offset."""
    v, f = mk()
    return np.concatenate([v, v]), np.concatenate([f, f + len(v)])


@pytest.mark.parametrize("name", ["icosphere2", "grid", "non_manifold", "degenerate", "noisy_level6", "two_noisy_level6"])
def test_against_f64_restatement(name, hip_lib):
    """two_noisy_level6: Q + E + F = 655 360 elements, a second trip of 131 072 behind gsr_reduce.h's capped grid."""
    level6 = lambda: mr.icosphere(6, noise=0.3, seed=3)
    mk = {"icosphere2": lambda: mr.icosphere(2, noise=0.2), "grid": lambda: mr.grid(6, noise=0.05),
          "non_manifold": mr.non_manifold, "degenerate": mr.degenerate,
          "noisy_level6": level6, "two_noisy_level6": lambda: _twice(level6)}[name]
    v, f = _mesh(mk)
    v = v.float().double()                       # the same f32 positions on both sides
    if name == "two_noisy_level6":               # each copy with the single mesh's references
        V1, F1 = v.shape[0] // 2, f.shape[0] // 2
        re, ra = _refs(v[:V1], f[:F1], seed=4)
        e1, e2 = mr.p3d_edges(f[:F1], V1)[0], mr.p3d_edges(f, 2 * V1)[0]
        assert torch.equal(e2, torch.cat([e1, e1 + V1]))              # the edges of the copies, in the single mesh's order
        Q = mr.p3d_pair_index(f, 2 * V1)[2].shape[0]
        assert Q + e2.shape[0] + f.shape[0] == 655_360
        re, ra = torch.cat([re, re]), torch.cat([ra, ra])
    else:
        re, ra = _refs(v, f, seed=4)
    re, ra = re.float().double(), ra.float().double()
    loss, parts, g = _fused(v.float(), f, re, ra, **FACTORS)
    want, gw = _restated(v, f, re, ra, **FACTORS)
    assert abs(float(loss) - float(want)) <= 1e-5 * abs(float(want)), (float(loss), float(want))
    nc_only, _, g_nc = _fused(v.float(), f, nc_factor=1.0)
    want_nc = float(mr.p3d_normal_consistency(v, f))
    assert abs(float(nc_only) - want_nc) <= 1e-5 * max(abs(want_nc), 1e-6)
    assert torch.isfinite(g).all() and torch.isfinite(g_nc).all()
    assert _grad_err(g, gw) <= 1e-4, _grad_err(g, gw)
    if name in ("non_manifold", "degenerate"):
        assert torch.equal(g[6], torch.zeros(3, device=DEV))     # referenced by no face: exactly 0
    if name == "two_noisy_level6":
        # Q, E and F doubled: every term's coefficient is exactly half the single mesh's, so is each copy's gradient, bit for bit
        _, _, g1 = _fused(v[:V1].float(), f[:F1], re[:len(re) // 2], ra[:F1], **FACTORS)
        _, _, g1_nc = _fused(v[:V1].float(), f[:F1], nc_factor=1.0)
        for got, one in ((g, g1), (g_nc, g1_nc)):
            assert torch.equal(got[:V1], 0.5 * one) and torch.equal(got[V1:], 0.5 * one)


def test_backward_is_deterministic_accumulates_and_scales_on_device(hip_lib):
    from gaustar_amd import harness, losses, meshes
    v, f = _mesh(lambda: mr.icosphere(6, noise=0.3, seed=5))
    re, ra = _refs(v, f, seed=6)
    v = v.float()
    topo = meshes.MeshTopology.of(f, v.shape[0])
    ctx = harness._PlainCtx((True,) + (False,) * 6)
    losses._SurfaceMeshLoss.forward(ctx, v, topo, 0.5, re.float(), 1000.0, ra.float(), 5000.0)
    one = torch.ones((), device=DEV)
    a = losses._SurfaceMeshLoss.grad_into(ctx, one, torch.empty_like(v), 0).clone()
    b = losses._SurfaceMeshLoss.grad_into(ctx, one, torch.full_like(v, float("nan")), 0)
    assert torch.equal(a, b)
    X = torch.randn(v.shape, device=DEV)
    acc = losses._SurfaceMeshLoss.grad_into(ctx, one, X.clone(), 1)
    assert torch.equal(acc, X + a)
    s = torch.tensor(-3.7, device=DEV)
    assert torch.equal(losses._SurfaceMeshLoss.grad_into(ctx, s, torch.empty_like(v), 0), a * s)
    # through autograd: the upstream gradient is the device scale
    _, _, g = _fused(v, f, re, ra, **FACTORS, upstream=-3.7)
    assert torch.equal(g, a * s)


def test_meshes_shim_composition_equals_fused_call(hip_lib):
    """refine.py:681-706 on meshes.Meshes / meshes.mesh_normal_consistency vs the one fused node."""
    from gaustar_amd import losses, meshes
    v, f = _mesh(lambda: mr.icosphere(5, noise=0.3, seed=7))
    re, ra = _refs(v, f, seed=8)
    re, ra = re.float(), ra.float()
    points = v.float().clone().requires_grad_(True)
    surface_mesh = meshes.Meshes(verts=[points], faces=[f])
    loss = 0.5 * meshes.mesh_normal_consistency(surface_mesh)
    verts_edges = surface_mesh.verts_packed()[surface_mesh.edges_packed()]
    v0, v1 = verts_edges.unbind(1)
    edge_len = (v0 - v1).norm(dim=1, p=2)
    loss = loss + 1000.0 * ((edge_len - re) ** 2).mean()
    face_area = surface_mesh.faces_areas_packed()
    loss = loss + 5000.0 * (face_area - ra).abs().mean()
    loss.backward()
    fused, _, g = _fused(v.float(), f, re, ra, **FACTORS)
    assert abs(float(loss.detach()) - float(fused)) <= 1e-5 * abs(float(fused))
    assert _grad_err(g, points.grad) <= 1e-4


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


def test_rgbd_step_with_mesh_reg_equals_the_autograd_iteration(hip_lib):
    """rgbd_step(mesh_reg=...) = (rgb_depth_loss(render_channels(...)) + surface_mesh_loss(...)).backward(): the loss bit for
    bit, gradients up to the order of the rasterizer backward's float atomics (as tests/test_gpu_iteration.py)."""
    from gaustar_amd import losses
    model, cam, bg4, gt_rgb, gt_d, reg = _small_model()
    params = [p for p in model.parameters() if p.requires_grad]
    img = model.render_channels(cam, bg4, depth_channels=1)[0]
    loss = losses.rgb_depth_loss(img, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5) + losses.surface_mesh_loss(
        model._points, model.mesh_topology(), **reg)
    loss.backward()
    ref = [None if p.grad is None else p.grad.clone() for p in params]
    for p in params:
        p.grad = None
    loss2, img2, _ = model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=reg)
    assert float(loss2) == float(loss) and torch.equal(img2, img.detach())
    for p, r in zip(params, ref):
        assert (p.grad is None) == (r is None)
        if r is not None and r.numel():
            assert torch.allclose(p.grad, r, rtol=2e-4, atol=1e-4 * float(r.abs().max()) + 1e-9), float((p.grad - r).abs().max())
    # the regulariser's share of the vertex gradient is there: without it, _points.grad differs by the fused node's gradient
    g_with = model._points.grad.clone()
    for p in params:
        p.grad = None
    loss3, _, _ = model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5)
    _, _, g_reg = _fused(model._points.detach(), model._surface_mesh_faces, reg["ref_edge_len"].double(), reg["ref_area"].double(),
                         0.5, 1000.0, 5000.0)
    assert float(loss2) > float(loss3)
    g_without = model._points.grad
    # (two renders: their vertex gradients differ by the backward blend's float-atomic order, 1e-4 of the largest each)
    assert torch.allclose(g_with - g_without, g_reg, rtol=1e-3, atol=2e-4 * float(g_without.abs().max()) + 1e-9)
    # a device scale reaches the regulariser's gradient too
    for p in params:
        p.grad = None
    model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, grad_scale=torch.tensor(-0.5, device=DEV), mesh_reg=reg)
    assert torch.allclose(model._points.grad, -0.5 * g_with, rtol=2e-4, atol=1e-4 * float(g_with.abs().max()) + 1e-9)


class _VertexSink:
    """The grad_sink interface of harness._RenderMeshBound (dist.ShardedAdam's grad_views / accepts / written) for `_points`
    alone: a buffer the vertex gradient is written into, and a snapshot of it at the moment the sink hears it is final."""

    def __init__(self, p):
        self.p, self.buf, self.at_written = p, torch.zeros_like(p), None

    def grad_views(self):
        return {id(self.p): self.buf}

    def accepts(self, q):
        return q is self.p

    def written(self, ps):
        if any(q is self.p for q in ps):
            self.at_written = self.buf.clone()


def test_rgbd_step_with_mesh_reg_through_a_gradient_sink(hip_lib):
    """With a gradient sink the vertex gradient lands in the sink's buffer: the regulariser's share must be in it BEFORE the
    sink hears the buffer is final (dist.ShardedAdam starts that bucket's reduce-scatter then)."""
    model, cam, bg4, gt_rgb, gt_d, reg = _small_model()
    model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=reg)
    ref = model._points.grad.clone()
    for p in model.parameters():
        p.grad = None
    sink = _VertexSink(model._points)
    model.grad_sink = sink
    try:
        model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=reg)
    finally:
        model.grad_sink = None
    got = model._points.grad
    assert got.data_ptr() == sink.buf.data_ptr() and sink.at_written is not None
    assert torch.equal(sink.at_written, got)
    assert torch.allclose(got, ref, rtol=2e-4, atol=1e-4 * float(ref.abs().max()) + 1e-9), float((got - ref).abs().max())
