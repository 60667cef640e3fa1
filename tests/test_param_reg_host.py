"""CPU: the host side of the parameter regularisers and of live loose binding -- the C-ABI table, SurfaceGaussians.loose_bind /
rebind / loose_bind_param_groups / apply_topology_result / face_delta on a CPU model (no kernel runs), and the f64 restatement
(tests/param_reg_ref.py) against closed forms."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import param_reg_ref as pr
from conftest import ROOT

NAMES = ("gsr_param_reg_workspace_bytes", "gsr_param_reg_forward", "gsr_param_reg_backward")


def test_symbols_are_declared_and_abi_is_unchanged():
    from gaustar_amd import _lib
    src = open(os.path.join(ROOT, "include", "gsr.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for n in NAMES:
        assert n in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % n, code), n
    assert _lib.ABI_VERSION == 16
    assert "gsr_param_reg.hip" in __import__("gaustar_amd.build", fromlist=["SOURCES"]).SOURCES


def _model(loose=False):
    from gaustar_amd import harness, scene
    v, f = scene.icosphere(1, 1.0)
    return harness.SurfaceGaussians(torch.from_numpy(v).float(), torch.from_numpy(f).long(), 6, sh_levels=2, loose_bind=loose)


def test_loose_bind_creates_the_reference_parameters_once():
    m = _model()
    N = m.n_points
    assert not m.is_loose_bind() and "_delta_t" not in m.state_dict()
    w = torch.rand(N)[:, None].expand(-1, 3)
    new = m.loose_bind(w)
    assert m.is_loose_bind() and len(new) == 2 and new[0] is m._delta_t and new[1] is m._delta_r
    assert all(isinstance(p, torch.nn.Parameter) and p.requires_grad for p in new)
    assert tuple(m._delta_t.shape) == (N, 3) and torch.equal(m._delta_t.detach(), torch.zeros(N, 3))
    assert tuple(m._delta_r.shape) == (N, 4)
    assert torch.equal(m._delta_r.detach(), torch.tensor([1.0, 0.0, 0.0, 0.0]).repeat(N, 1))
    assert m._geom_cache is None and torch.equal(m.unbind_loss_weight, w) and m.unbind_loss_weight.stride(1) == 0
    assert m.loose_bind() == [] and torch.equal(m.unbind_loss_weight, w)       # second time: nothing new, the weight stays
    sd = m.state_dict()
    assert "_delta_t" in sd and "_delta_r" in sd and "unbind_loss_weight" not in sd
    with torch.no_grad():
        m._delta_t.add_(0.5)
    keep_t, keep_r = m._delta_t, m._delta_r
    m.rebind()
    assert not m.is_loose_bind() and m._delta_t is keep_t and m._delta_r is keep_r
    assert torch.equal(m._delta_t.detach(), torch.full((N, 3), 0.5)) and "_delta_t" in m.state_dict()
    assert m.loose_bind() == [] and m.is_loose_bind()
    # a model constructed loose-bound already has them; its state dict loads into the live-unbound one
    m2 = _model(loose=True)
    assert m2.loose_bind() == [] and set(m2.state_dict()) == set(m.state_dict())
    m2.load_state_dict(m.state_dict())
    with pytest.raises(ValueError):
        m.loose_bind(torch.ones(N + 1))


def test_face_delta():
    m = _model()
    with pytest.raises(RuntimeError):
        m.face_delta()
    m.loose_bind()
    with torch.no_grad():
        m._delta_t.copy_(torch.arange(m.n_points * 3, dtype=torch.float32).view(-1, 3) * 1e-3)
    want = m._delta_t.detach().reshape(-1, 6, 3).mean(dim=1).norm(dim=1, keepdim=True)
    got = m.face_delta()
    assert tuple(got.shape) == (m._surface_mesh_faces.shape[0], 1) and torch.equal(got, want) and not got.requires_grad


def test_param_groups_join_a_torch_adam_and_its_state_round_trips():
    m = _model()
    with pytest.raises(RuntimeError):
        m.loose_bind_param_groups(1e-3, 1e-3)
    opt = torch.optim.Adam([{"params": [m._points], "lr": 2e-4, "name": "points"}], lr=0.0, eps=1e-15)
    m.loose_bind()
    groups = m.loose_bind_param_groups(position_lr=1.6e-4, rotation_lr=1e-3)
    assert [g["name"] for g in groups] == ["delta_t", "delta_r"] and [g["lr"] for g in groups] == [1.6e-4, 1e-3]
    assert groups[0]["params"][0] is m._delta_t and groups[1]["params"][0] is m._delta_r
    for g in groups:
        opt.add_param_group(g)
    (m._points.sum() + (m._delta_t ** 2).sum() + m._delta_r.sum()).backward()
    opt.step()
    sd = opt.state_dict()
    assert [g["name"] for g in sd["param_groups"]] == ["points", "delta_t", "delta_r"] and sorted(sd["state"]) == [0, 1, 2]
    m2 = _model()
    m2.loose_bind()
    opt2 = torch.optim.Adam([{"params": [m2._points], "lr": 2e-4, "name": "points"}], lr=0.0, eps=1e-15)
    for g in m2.loose_bind_param_groups(1.6e-4, 1e-3):
        opt2.add_param_group(g)
    opt2.load_state_dict(sd)
    sd2 = opt2.state_dict()
    assert sd2["param_groups"] == sd["param_groups"]
    for k in sd["state"]:
        assert torch.equal(sd2["state"][k]["exp_avg"], sd["state"][k]["exp_avg"])


@pytest.mark.parametrize("changed,want", [(99, False), (100, True)])
def test_apply_topology_result_threshold(changed, want):
    """refine.py:730-736: fewer than 100 Gaussians of weight 0 -> nothing changes."""
    m = _model()
    N = m.n_points
    w = torch.ones(N)
    w[:changed] = 0.0
    opt = torch.optim.Adam([{"params": [m._points], "lr": 2e-4, "name": "points"}], lr=0.0, eps=1e-15)
    for res in (SimpleNamespace(unbind_weight=w[:, None].expand(-1, 3), topo_change_num=changed),
                SimpleNamespace(unbind_weight=w[:, None].expand(-1, 3))):           # (count taken from the weights)
        if m.is_loose_bind():
            break
        assert m.apply_topology_result(res, optimizer=opt, position_lr=1e-4, rotation_lr=1e-3) is want
    assert m.is_loose_bind() is want and len(opt.param_groups) == (3 if want else 1)
    if want:
        assert torch.equal(m.unbind_loss_weight, w[:, None].expand(-1, 3))
        assert opt.param_groups[1]["params"][0] is m._delta_t and opt.param_groups[2]["lr"] == 1e-3
    else:
        assert getattr(m, "_delta_t", None) is None and m.unbind_loss_weight is None


def test_restatement_against_closed_forms():
    N = 37
    dt = torch.zeros(N, 3, dtype=torch.float64, requires_grad=True)
    p = pr.ref_parts(delta_t=dt, factor_t=100.0)
    p[0].backward()
    assert float(p[0]) == 0.0 and torch.equal(dt.grad, torch.zeros(N, 3, dtype=torch.float64))      # d|x|/dx = 0 at 0
    c = -0.0125
    assert abs(float(pr.ref_parts(delta_t=torch.full((N, 3), c, dtype=torch.float64), weight=torch.ones(N),
                                  factor_t=100.0)[0]) - 100.0 * abs(c)) <= 1e-12
    ident = torch.tensor([1.0, 0.0, 0.0, 0.0], dtype=torch.float64).repeat(N, 1)
    assert float(pr.ref_parts(delta_r=ident, factor_r=1.0)[1]) == 0.0
    logit = math.log(0.8 / 0.2)
    assert float(pr.ref_parts(densities=torch.full((N, 1), logit + 1e-3, dtype=torch.float64), min_opacity=0.8)[2]) == 0.0
    below = pr.ref_parts(densities=torch.full((N, 1), 0.0, dtype=torch.float64), min_opacity=0.8)[2]
    assert abs(float(below) - 0.3) <= 1e-12
    sh, pre = torch.zeros(N, 1, 3, dtype=torch.float64), torch.full((10, 3), 0.5, dtype=torch.float64)
    assert abs(float(pr.ref_parts(sh_dc=sh, pre_sh_dc=pre, sh_factor=2.0)[3]) - 0.5) <= 1e-12
    assert abs(float(pr.ref_total(delta_t=torch.full((N, 3), c, dtype=torch.float64), factor_t=100.0, sh_dc=sh, pre_sh_dc=pre,
                                  sh_factor=2.0)) - (1.25 + 0.5)) <= 1e-12
