"""GPU: the fused regularisers on the Gaussians' own parameters (gsr_param_reg_forward / _backward,
losses.gaussian_param_loss), live loose binding of a SurfaceGaussians and SurfaceGaussians.rgbd_step(param_reg=...), against
the f64 torch restatement of refine.py:739-748 / :663-669 (tests/param_reg_ref.py) and the autograd compositions."""
import copy
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import param_reg_ref as pr
from conftest import GOLDEN_DIR, ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FACTORS = dict(factor_t=100.0, factor_r=1.0, min_opacity=0.8, sh_factor=1.0)     # refine.py:29-33
N, M = 100_003, 60_001      # N is no multiple of the workgroup's 1024 Gaussians nor of a thread's 4; M < N, M % 4 != 0


def _inputs(seed=0, n=N, m=M, weights="binary"):
    g = torch.Generator(device=DEV).manual_seed(seed)
    r = lambda *s: torch.randn(*s, device=DEV, generator=g)
    dt = r(n, 3) * 0.01
    dt[r(n, 3) > 1.0] = 0.0                                   # exact zeros, as right after loose_bind()
    dr = torch.nn.functional.normalize(torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV) + 0.05 * r(n, 4), dim=-1)
    dr[:, 1:][r(n, 3) > 1.0] = 0.0
    dens = r(n, 1) * 1.5 + 1.4                                # around logit(0.8) = 1.386: both sides well populated
    near = (torch.sigmoid(dens.double()) - FACTORS["min_opacity"]).abs() < 1e-4
    dens[near] += 0.01
    sh = r(n, 1, 3)
    pre = sh[:m, 0].clone() + 0.1 * r(m, 3)
    if weights == "binary":                                   # what detection produces: 1 - face_loss in {0, 1}, per face
        w = (torch.rand(n // 6 + 1, device=DEV, generator=g) > 0.3).float().repeat_interleave(6)[:n].contiguous()
    else:
        w = torch.rand(n, device=DEV, generator=g)
    # the comparisons below exclude nothing, so the inputs must stay off the kinks
    assert float((torch.sigmoid(dens.double()) - FACTORS["min_opacity"]).abs().min()) >= 1e-4
    for d in (dt, dr[:, 1:]):
        assert not bool(((d != 0) & (d.abs() < 1e-12)).any())
    if n >= 1000:
        assert bool((dt == 0).any()) and bool((dr[:, 1:] == 0).any()) and bool((w == 0).any() or weights != "binary")
    return dict(delta_t=dt, delta_r=dr, weight=w, densities=dens, sh_dc=sh, pre_sh_dc=pre)


def _layouts(w):
    return {"[N]": w, "expanded": w[:, None].expand(-1, 3), "materialised": w[:, None].expand(-1, 3).contiguous()}


def _fused(inp, upstream=None, **over):
    from gaustar_amd import losses
    kw = dict(inp, **FACTORS)
    kw.update(over)
    leaves = {}
    for k in ("delta_t", "delta_r", "densities", "sh_dc"):
        if kw.get(k) is not None:
            leaves[k] = kw[k] = kw[k].detach().clone().requires_grad_(True)
    loss, parts = losses.gaussian_param_loss(return_parts=True, **kw)
    if upstream is None:
        loss.backward()
    else:
        loss.backward(torch.tensor(upstream, device=DEV))
    return loss.detach(), parts, {k: v.grad for k, v in leaves.items()}


def _restated(inp, **over):
    kw = dict(inp, **FACTORS)
    kw.update(over)
    leaves = {}
    for k in ("delta_t", "delta_r", "densities", "sh_dc"):
        if kw.get(k) is not None:
            leaves[k] = kw[k] = kw[k].detach().double().requires_grad_(True)
    parts = pr.ref_parts(**kw)
    total = ((parts[0] + parts[1]) + parts[2]) + parts[3]
    total.backward()
    return total.detach(), [p.detach() for p in parts], {k: v.grad for k, v in leaves.items()}


def _sizes():
    """(N, M) = the module's own first (its ids stay as they were), then tests/beyond_caps.py's: config C's 491 520 Gaussians
    (480 workgroups: tree_total's lanes add a second partial) and 524 290 groups of four (a second trip of two groups, the last
    of them ragged)."""
    import beyond_caps
    sizes = beyond_caps.param_reg_sizes()
    assert sizes[0] == (N, M)
    return [pytest.param(w, n, m, id=w if (n, m) == (N, M) else f"{w}-{n}") for n, m in sizes for w in ("binary", "fractional")]


@pytest.mark.parametrize("weights,n,m", _sizes())
def test_forward_and_gradients_against_f64_restatement(weights, n, m, hip_lib):
    """Each part and the total within 1e-5 relative (a sum of non-negative f32 terms: log2(3N) 2^-24 ~ 1.3e-6 for a tree plus
    one rounding per element, 1.4e-6 at the largest N; the kernel sums in double), gradients elementwise at rtol 1e-5 (three to
    five f32 operations per element) with NO element excluded, the exact zeros with ==; the three weight layouts give identical
    bits."""
    inp = _inputs(seed=1, n=n, m=m, weights=weights)
    want, want_parts, gw = _restated(inp)
    results = {}
    for name, w in _layouts(inp["weight"]).items():
        loss, parts, g = _fused(dict(inp, weight=w))
        results[name] = (parts.clone(), {k: v.clone() for k, v in g.items()})
        p = parts.double()
        for i in range(4):
            print(f"[param_reg] {weights} {name} part {i}: {float(p[i]):.9g} vs {float(want_parts[i]):.9g}")
            assert float(want_parts[i]) > 0 and abs(float(p[i]) - float(want_parts[i])) <= 1e-5 * float(want_parts[i]), (name, i)
        assert abs(float(p[4]) - float(want)) <= 1e-5 * float(want) and float(loss) == float(parts[4])
        for k in g:
            worst = float(((g[k].double() - gw[k]).abs() / gw[k].abs().clamp_min(1e-300)).nan_to_num(0.0).max())
            print(f"[param_reg] {weights} {name} grad {k}: worst relative error {worst:.3e}")
            assert torch.allclose(g[k].double(), gw[k], rtol=1e-5, atol=0.0), (name, k, worst)
        # the exact-zero cases
        wcol = inp["weight"][:, None]
        assert bool((g["delta_t"][inp["delta_t"] == 0] == 0).all()) and bool((g["delta_t"][(wcol == 0).expand(-1, 3)] == 0).all())
        assert bool((g["delta_r"][:, 0] == 0).all()) and bool((g["delta_r"][:, 1:][(wcol == 0).expand(-1, 3)] == 0).all())
        assert bool((g["delta_r"][:, 1:][inp["delta_r"][:, 1:] == 0] == 0).all())
        assert bool((g["sh_dc"][m:] == 0).all()) and bool((g["sh_dc"][:m] != 0).any())
        above = torch.sigmoid(inp["densities"].double()) > FACTORS["min_opacity"]
        assert bool((g["densities"][above] == 0).all()) and bool((g["densities"][~above] < 0).all())
    ref_parts_, ref_g = results["[N]"]
    for name in ("expanded", "materialised"):
        assert torch.equal(results[name][0], ref_parts_), name
        for k in ref_g:
            assert torch.equal(results[name][1][k], ref_g[k]), (name, k)


def test_terms_are_skipped_and_small_sizes(hip_lib):
    """A term without its tensor or with factor 0 is 0 and has no gradient; M == N (refine.py:669); N below one thread's four."""
    inp = _inputs(seed=2, n=4099, m=4099)
    loss, parts, g = _fused(inp, factor_t=0.0)
    assert float(parts[0]) == 0.0 and g["delta_t"] is None and float(parts[1]) > 0
    want, wp, gw = _restated(inp, factor_t=0.0)
    assert abs(float(loss) - float(want)) <= 1e-5 * float(want)
    assert torch.allclose(g["sh_dc"].double(), gw["sh_dc"], rtol=1e-5, atol=0.0) and bool((g["sh_dc"] != 0).all(dim=-1).any())
    loss, parts, g = _fused(dict(inp, pre_sh_dc=None, delta_r=None))
    assert float(parts[1]) == 0.0 and float(parts[3]) == 0.0 and g["sh_dc"] is None
    loss, parts, g = _fused(dict(inp, densities=None, weight=None))
    want, wp, gw = _restated(dict(inp, densities=None, weight=None))
    assert float(parts[2]) == 0.0 and abs(float(loss) - float(want)) <= 1e-5 * float(want)
    assert torch.allclose(g["delta_t"].double(), gw["delta_t"], rtol=1e-5, atol=0.0)
    for n, m in ((1, 1), (3, 2), (5, 5), (1023, 7)):
        inp = _inputs(seed=3 + n, n=n, m=m, weights="fractional")
        loss, parts, g = _fused(inp)
        want, wp, gw = _restated(inp)
        assert abs(float(loss) - float(want)) <= 1e-5 * float(want), n
        for k in g:
            assert torch.allclose(g[k].double(), gw[k], rtol=1e-5, atol=0.0), (n, k)


def _ctx(inp, **over):
    from gaustar_amd import harness, losses
    kw = dict(inp, **FACTORS)
    kw.update(over)
    ctx = harness._PlainCtx((True, True, False, False, False, True, False, True, False, False))
    total, parts = losses._GaussianParamLoss.forward(ctx, kw["delta_t"], kw["delta_r"], kw["weight"], kw["factor_t"], kw["factor_r"],
                                                     kw["densities"], kw["min_opacity"], kw["sh_dc"], kw["pre_sh_dc"], kw["sh_factor"])
    return ctx, parts


def _bufs(inp, fill=None):
    mk = (lambda t: torch.empty_like(t)) if fill is None else (lambda t: torch.full_like(t, fill))
    return tuple(mk(inp[k]) for k in ("delta_t", "delta_r", "densities", "sh_dc"))


def test_backward_accumulates_skips_null_outputs_and_is_deterministic(hip_lib):
    from gaustar_amd import losses
    inp = _inputs(seed=4, weights="fractional")
    ctx, parts = _ctx(inp)
    one = torch.ones((), device=DEV)
    G = losses._GaussianParamLoss.grad_into
    a = [b.clone() for b in G(ctx, one, _bufs(inp), 0)]
    b = G(ctx, one, _bufs(inp, float("nan")), 0)                      # a second call, over NaNs: every element is written
    ctx2, parts2 = _ctx(inp)
    assert torch.equal(parts, parts2) and all(torch.equal(x, y) for x, y in zip(a, b))
    g = torch.Generator(device=DEV).manual_seed(5)
    X = [torch.randn(t.shape, device=DEV, generator=g) for t in a]
    acc = G(ctx, one, tuple(x.clone() for x in X), 1)
    for x, f, got in zip(X, a, acc):
        assert torch.equal(got, x + f)                                # one rounding per element, torch's X + fresh
    s = torch.tensor(-3.7, device=DEV)
    scaled = G(ctx, s, _bufs(inp), 0)
    _, _, g_auto = _fused(inp, upstream=-3.7)                         # through autograd: the upstream gradient is the device scale
    for got, k in zip(scaled, ("delta_t", "delta_r", "densities", "sh_dc")):
        assert torch.equal(got, g_auto[k].view(got.shape))
    _, _, g_one = _fused(inp)
    for f, k in zip(a, ("delta_t", "delta_r", "densities", "sh_dc")):
        assert torch.equal(f, g_one[k].view(f.shape))                 # gaussian_param_loss(...).backward() == grad_into
    # NULL outputs: the others are written, nothing else is touched
    for keep in range(4):
        bufs = list(_bufs(inp, 7.0))
        call = tuple(bf if i == keep else None for i, bf in enumerate(bufs))
        G(ctx, one, call, 0)
        assert torch.equal(bufs[keep], a[keep])
        assert all(bool((bufs[i] == 7.0).all()) for i in range(4) if i != keep)
    # a skipped term leaves its buffer as it is, whichever mode
    ctx0, _ = _ctx(inp, factor_t=0.0, pre_sh_dc=None)
    bufs = G(ctx0, one, _bufs(inp, 7.0), 1)
    assert bool((bufs[0] == 7.0).all()) and bool((bufs[3] == 7.0).all()) and torch.equal(bufs[1], torch.full_like(bufs[1], 7.0) + a[1])
    # a second stream
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        ctx3, parts3 = _ctx(inp)
        c = G(ctx3, one, _bufs(inp), 0)
    side.synchronize()
    assert torch.equal(parts3, parts) and all(torch.equal(x, y) for x, y in zip(a, c))
    # an unaligned view takes the scalar path: same bits
    base = torch.zeros(inp["delta_t"].numel() + 1, device=DEV)
    odd = base[1:].view_as(inp["delta_t"])
    assert odd.data_ptr() % 16 != 0
    G(ctx, one, (odd, None, None, None), 0)
    assert torch.equal(odd, a[0])


def _golden_model(loose):
    """The mesh-bound model of tests/golden/mesh_sphere.npz (icosphere level 2, 6 Gaussians per face, its colours, opacities
    and camera) as a SurfaceGaussians."""
    from gaustar_amd import harness, scene
    z = np.load(os.path.join(GOLDEN_DIR, "mesh_sphere.npz"))
    v, f = scene.icosphere(2, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    m = harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), 6, 2, loose_bind=loose).to(DEV)
    op = torch.from_numpy(z["in_opacities"]).to(DEV).view(-1, 1).clamp(1e-4, 1 - 1e-4)
    col = torch.from_numpy(z["in_colors_precomp"]).to(DEV)
    assert m.n_points == op.shape[0] == col.shape[0]
    with torch.no_grad():
        m.all_densities.copy_(torch.log(op / (1 - op)))
        m._sh_coordinates_dc.copy_(((col - 0.5) / scene.SH_C0)[:, None, :])
    cam = harness.nerf_camera_from_scene(scene.look_at_camera((0.4, 1.5, 3.0), scene.SUBJECT_CENTER, 160, 120, focal_px=130.0))
    return m, cam


def test_live_loose_bind_renders_like_a_model_constructed_loose_bound(hip_lib):
    bg = torch.tensor([0.0, 1.0, 0.0], device=DEV)
    m, cam = _golden_model(False)
    with torch.no_grad():
        img0, radii0 = m.render_channels(cam, bg, depth_channels=0)
        assert m.loose_bind() != []
        img1, radii1 = m.render_channels(cam, bg, depth_channels=0)
        pts1 = m.points.clone()
        ref, _ = _golden_model(True)
        missing = ref.load_state_dict(m.state_dict())
        assert not missing.missing_keys and not missing.unexpected_keys
        img2, radii2 = ref.render_channels(cam, bg, depth_channels=0)
        assert torch.equal(img1, img2) and torch.equal(radii1, radii2) and torch.equal(pts1, ref.points)
        assert int((radii1 > 0).sum()) > 500
        assert torch.equal(radii0, radii1)
        print(f"[param_reg] bound vs identity-delta render: max |diff| {float((img0 - img1).abs().max()):.3e}")
        assert torch.allclose(img1, img0, rtol=1e-6, atol=1e-7)
        # rebind(): the deltas stay and are ignored again
        m._delta_t.add_(0.01)
        moved, _ = m.render_channels(cam, bg, depth_channels=0)
        assert not torch.equal(moved, img1)
        m.rebind()
        back, radii_b = m.render_channels(cam, bg, depth_channels=0)
        assert torch.equal(back, img0) and torch.equal(radii_b, radii0)


def _small_model(seed=4):
    from gaustar_amd import harness, scene
    v, f = scene.icosphere(3, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    model = harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), 6, 3).to(DEV)
    g = torch.Generator(device=DEV).manual_seed(seed)
    n = model.n_points
    with torch.no_grad():
        model._sh_coordinates_dc.copy_(torch.rand(n, 1, 3, device=DEV, generator=g) * 2 - 1)
        model._sh_coordinates_rest.copy_(torch.randn(model._sh_coordinates_rest.shape, device=DEV, generator=g) * 0.1)
        model.all_densities.copy_(torch.randn(n, 1, device=DEV, generator=g) * 0.8 + 1.6)
    ref_mesh = model.surface_mesh
    ve = ref_mesh.verts_packed().detach()[ref_mesh.edges_packed()]
    mesh_reg = dict(nc_factor=0.5, ref_edge_len=(ve[:, 0] - ve[:, 1]).norm(dim=1) * 0.98, edge_factor=1000.0,
                    ref_area=ref_mesh.faces_areas_packed().detach() * 0.95, area_factor=5000.0)
    w = (torch.rand(n // 6, device=DEV, generator=g) > 0.4).float().repeat_interleave(6)[:, None].expand(-1, 3)
    model.loose_bind(w)
    with torch.no_grad():      # non-zero deltas
        model._delta_t.copy_(0.004 * torch.randn(n, 3, device=DEV, generator=g))
        model._delta_r.copy_(torch.nn.functional.normalize(
            torch.tensor([1.0, 0.0, 0.0, 0.0], device=DEV) + 0.03 * torch.randn(n, 4, device=DEV, generator=g), dim=-1))
    m_pre = (n // 6 // 2) * 6                                         # track_face_num * 6 rows
    pre = model._sh_coordinates_dc.detach()[:m_pre, 0].clone() + 0.2 * torch.randn(m_pre, 3, device=DEV, generator=g)
    cam = harness.nerf_camera_from_scene(scene.ring_cameras(5, 32, 320, 240, focal_px=200.0)[37])
    bg4 = torch.tensor([0.0, 1.0, 0.0, 10.0], device=DEV)
    gt_rgb = torch.rand(3, 240, 320, device=DEV, generator=g)
    gt_d = torch.rand(240, 320, device=DEV, generator=g) * 12.0
    return model, cam, bg4, gt_rgb, gt_d, dict(FACTORS, pre_sh_dc=pre), mesh_reg


def _param_loss(model, reg, fused):
    """The four terms on the model's parameters: the fused node, or the reference's four torch lines."""
    from gaustar_amd import losses
    pre = reg["pre_sh_dc"]
    if fused:
        return losses.gaussian_param_loss(model._delta_t, model._delta_r, model.unbind_loss_weight, reg["factor_t"], reg["factor_r"],
                                          model.all_densities, reg["min_opacity"], model._sh_coordinates_dc, pre, reg["sh_factor"])
    loss = reg["factor_t"] * (model.unbind_loss_weight * model._delta_t.abs()).mean()
    loss = loss + reg["factor_r"] * (model.unbind_loss_weight * model._delta_r[..., 1:].abs()).mean()
    loss = loss + torch.relu(reg["min_opacity"] - model.strengths.view(-1, 1)).mean()
    return loss + reg["sh_factor"] * ((pre - model._sh_coordinates_dc[:pre.shape[0], 0, :]) ** 2).mean()


def _close(p, r):
    return torch.allclose(p, r, rtol=2e-4, atol=1e-4 * float(r.abs().max()) + 1e-9)


@pytest.mark.parametrize("with_mesh_reg", [False, True], ids=["param_reg", "param_reg + mesh_reg"])
def test_rgbd_step_with_param_reg_equals_the_autograd_iterations(with_mesh_reg, hip_lib):
    """rgbd_step(param_reg=...) = (rgb_depth_loss(render_channels(...)) + gaussian_param_loss(...)).backward() on a deep copy,
    and = the same with refine.py's four torch lines in place of the fused node: the loss and every parameter's gradient, to the
    tolerances tests/test_gpu_mesh_reg.py uses for rgbd_step(mesh_reg=...)."""
    from gaustar_amd import losses
    model, cam, bg4, gt_rgb, gt_d, reg, mesh_reg = _small_model()
    names = [n for n, p in model.named_parameters() if p.requires_grad]
    assert "_delta_t" in names and "_delta_r" in names
    refs = {}
    for fused in (True, False):
        m2 = copy.deepcopy(model)
        assert m2.is_loose_bind() and torch.equal(m2.unbind_loss_weight, model.unbind_loss_weight)
        img = m2.render_channels(cam, bg4, depth_channels=1)[0]
        loss = losses.rgb_depth_loss(img, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5) + _param_loss(m2, reg, fused)
        if with_mesh_reg:
            loss = loss + losses.surface_mesh_loss(m2._points, m2.mesh_topology(), **mesh_reg)
        loss.backward()
        refs[fused] = (float(loss), {n: p.grad.clone() for n, p in m2.named_parameters() if p.grad is not None})
    loss2, _img2, _ = model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, param_reg=reg,
                                      mesh_reg=mesh_reg if with_mesh_reg else None)
    for fused in (True, False):
        want, grads = refs[fused]
        print(f"[param_reg] rgbd_step loss {float(loss2):.8g} vs {'fused' if fused else 'torch lines'} {want:.8g}")
        assert abs(float(loss2) - want) <= 2e-4 * abs(want)
        assert set(grads) == set(names)
        for n, p in model.named_parameters():
            assert _close(p.grad, grads[n]), (fused, n, float((p.grad - grads[n]).abs().max()))
    # the regularisers' share is there: without param_reg the loss is smaller and the delta / density gradients differ
    g_with = {n: p.grad.clone() for n, p in model.named_parameters()}
    for p in model.parameters():
        p.grad = None
    loss3, _, _ = model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=mesh_reg if with_mesh_reg else None)
    assert float(loss2) > float(loss3)
    for n in ("_delta_t", "all_densities", "_sh_coordinates_dc"):
        assert not _close(dict(model.named_parameters())[n].grad, g_with[n]), n
    # a device scale reaches the regularisers' gradients too
    for p in model.parameters():
        p.grad = None
    model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, grad_scale=torch.tensor(-0.5, device=DEV), param_reg=reg,
                    mesh_reg=mesh_reg if with_mesh_reg else None)
    for n, p in model.named_parameters():
        assert _close(p.grad, -0.5 * g_with[n]), n
    # a bound model: the loose terms are off, the opacity and SH terms stay
    model.rebind()
    for p in model.parameters():
        p.grad = None
    loss4, _, _ = model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, param_reg=reg)
    assert model._delta_t.grad is None and model._delta_r.grad is None and float(loss4) > 0
    with pytest.raises(TypeError):
        model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, param_reg=dict(reg, nonsense=1))


def test_param_reg_alone_pulls_the_weighted_deltas_back(hip_lib):
    """Weight 1 on half the faces, 0 on the rest, the regularisers only, 20 optim.Adam steps from small random deltas: |delta_t|
    of the weighted half shrinks, the other half's deltas do not change by a bit."""
    from gaustar_amd import losses, optim
    model, *_ = _small_model(seed=6)
    n = model.n_points
    w = torch.zeros(n, device=DEV)
    w[: n // 2] = 1.0
    model.loose_bind(w)
    dt0, dr0 = model._delta_t.detach().clone(), model._delta_r.detach().clone()
    opt = optim.Adam(model.loose_bind_param_groups(1e-4, 1e-4), eps=1e-15)
    for _ in range(20):
        opt.zero_grad()
        losses.gaussian_param_loss(model._delta_t, model._delta_r, model.unbind_loss_weight).backward()
        opt.step()
    dt, dr = model._delta_t.detach(), model._delta_r.detach()
    assert float(dt[: n // 2].abs().mean()) < 0.8 * float(dt0[: n // 2].abs().mean())
    assert float(dr[: n // 2, 1:].abs().mean()) < float(dr0[: n // 2, 1:].abs().mean())
    assert torch.equal(dt[n // 2:], dt0[n // 2:]) and torch.equal(dr[n // 2:], dr0[n // 2:])
    assert torch.equal(dr[:, 0], dr0[:, 0])


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


_SINK = r'''
import os, sys
sys.path.insert(0, %r); sys.path.insert(0, os.path.join(%r, "tests"))
import torch
os.environ.update(RANK="0", WORLD_SIZE="1", LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=%r, HSA_ENABLE_IPC_MODE_LEGACY="0")
import torch.distributed as dist
torch.cuda.set_device(0)
dist.init_process_group(backend="nccl", rank=0, world_size=1)
import test_gpu_param_reg as T
from gaustar_amd import dist as gd, optim
groups = lambda m: [{"params": [m._points], "lr": 2e-4}, {"params": [m._sh_coordinates_dc, m._sh_coordinates_rest], "lr": 5e-3},
                    {"params": [m._scales, m._quaternions, m.all_densities], "lr": 5e-3}]
def make():
    from gaustar_amd import harness, scene
    v, f = scene.icosphere(3, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    m = harness.SurfaceGaussians(torch.from_numpy(v).float().to(T.DEV), torch.from_numpy(f).long().to(T.DEV), 6, 3).to(T.DEV)
    src, cam, bg4, gt_rgb, gt_d, reg, _ = T._small_model()
    with torch.no_grad():
        for k in ("_sh_coordinates_dc", "_sh_coordinates_rest", "all_densities"):
            getattr(m, k).copy_(getattr(src, k))
    return m, src, (cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5), reg
a, src, args, reg = make()
b, _, _, _ = make()
oa = gd.ShardedAdam(groups(a), ready_order=a.grad_ready_order(), eps=1e-15, bucket_bytes=256 << 10, run_at_world_size_1=True)
ob = optim.Adam(groups(b), eps=1e-15)
a.grad_sink = oa
class Res: pass
res = Res(); res.unbind_weight = src.unbind_loss_weight; res.topo_change_num = 1000
for it in range(4):
    if it == 1:       # the live transition, between step() and the next backward
        assert a.apply_topology_result(res, optimizer=oa, position_lr=2e-4, rotation_lr=1e-3)
        assert b.apply_topology_result(res, optimizer=ob, position_lr=2e-4, rotation_lr=1e-3)
        views = oa.grad_views()
        assert id(a._delta_t) in views and id(a._delta_r) in views
        for m in (a, b):
            with torch.no_grad():
                m._delta_t.copy_(src._delta_t); m._delta_r.copy_(src._delta_r)
    oa.zero_grad(set_to_none=True); ob.zero_grad(set_to_none=True)
    la = a.rgbd_step(*args, param_reg=reg)[0]
    views = oa.grad_views()
    n_alias = sum(1 for p in a.parameters() if p.grad is not None and p.grad.data_ptr() == views[id(p)].data_ptr())
    assert n_alias == (6 if it == 0 else 8), (it, n_alias)
    # the other optimiser steps on the SAME gradients (two renders differ in the last bits of the blend's float atomics)
    for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
        q.grad = None if p.grad is None else p.grad.clone()
    if it == 1:       # ... which are those of the run without a sink, up to that noise
        c = T.copy.deepcopy(b)
        for p in c.parameters():
            p.grad = None
        lc = c.rgbd_step(*args, param_reg=reg)[0]
        assert abs(float(lc) - float(la)) <= 2e-4 * abs(float(lc))
        for (n, p), (_, q) in zip(a.named_parameters(), c.named_parameters()):
            assert T._close(p.grad, q.grad), n
    oa.step(); ob.step()
torch.cuda.synchronize()
for (n, p), (_, q) in zip(a.named_parameters(), b.named_parameters()):
    assert torch.equal(p, q), n
assert not torch.equal(a._delta_t, src._delta_t)
dist.barrier(); dist.destroy_process_group()
print("PARAM_REG_SINK_OK")
'''


def test_rgbd_step_with_param_reg_through_a_sharded_adam_sink():
    """dist.ShardedAdam (RCCL, world size 1) as grad_sink, the deltas joined by add_param_group after the first step: grad_views()
    covers them, all eight gradients land in the flat buffer in place, they equal those of the run without a sink, and the stepped
    parameters are bit-identical to optim.Adam's on the same gradients."""
    code = _SINK % (ROOT, ROOT, str(_free_port()))
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "PARAM_REG_SINK_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
