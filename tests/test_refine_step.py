"""CPU: the host-side contract of the refinement step (gaustar_amd/refine_step.py) -- the gradient hand-off, the named
parameters with the needs_input_grad derived from them, and the two dict parsers of rgbd_step -- with a fake sink, fake loss
nodes and plain CPU tensors: no GPU, no library."""
import inspect

import pytest
import torch

from gaustar_amd import harness, losses, refine_step as rs, scene


def _model(loose):
    v, f = scene.icosphere(1, 1.0)
    return harness.SurfaceGaussians(torch.from_numpy(v).float(), torch.from_numpy(f).long(), 1, sh_levels=2, loose_bind=loose)


# ---------------------------------------------------------------------------------------------------- the hand-off
class _Sink:
    def __init__(self, accepted):
        self.views = {id(p): torch.zeros_like(p) for p in accepted}
        self.accepted, self.heard = list(accepted), []

    def grad_views(self):
        return self.views

    def accepts(self, p):
        return any(p is q for q in self.accepted)

    def written(self, params):
        self.heard.append(list(params))


def test_hand_off_without_a_sink_gives_no_buffer_and_tells_nobody():
    p = _model(True).render_params()
    hand = rs.GradHandoff(None)
    assert hand.take(p.sh_dc, p.sh_rest, p.densities) == (None, None, None)
    hand.written()
    assert hand.take(p.verts, p.raw_scales, p.raw_complex, p.delta_t, p.delta_r) == (None,) * 5
    hand.written()
    g = torch.ones(3)
    assert hand.fresh(g, None) is g and hand.fresh(None, None) is None


def test_hand_off_gives_the_sinks_views_of_accepted_parameters_and_notifies_once_per_stage():
    p = _model(False).render_params()                 # bound: delta_t / delta_r are None
    sink = _Sink([p.sh_dc, p.densities, p.verts, p.raw_complex])
    hand = rs.GradHandoff(sink)
    colour = hand.take(p.sh_dc, p.sh_rest, p.densities)
    assert colour[0] is sink.views[id(p.sh_dc)] and colour[1] is None and colour[2] is sink.views[id(p.densities)]
    assert sink.heard == []                           # nothing before the stage says so
    hand.written()
    mesh = hand.take(p.verts, p.raw_scales, p.raw_complex, p.delta_t, p.delta_r)
    assert mesh[0] is sink.views[id(p.verts)] and mesh[2] is sink.views[id(p.raw_complex)]
    assert mesh[1] is None and mesh[3] is None and mesh[4] is None
    hand.written()
    assert len(sink.heard) == 2                       # once per stage, colour then mesh, the accepted parameters alone
    assert [id(q) for q in sink.heard[0]] == [id(p.sh_dc), id(p.densities)]
    assert [id(q) for q in sink.heard[1]] == [id(p.verts), id(p.raw_complex)]
    # what goes back to autograd for a sink-backed gradient: a new tensor object on the view's storage
    back = hand.fresh(mesh[0], mesh[0])
    assert back is not mesh[0] and back.data_ptr() == mesh[0].data_ptr() and back.shape == mesh[0].shape
    g = torch.ones(3)
    assert hand.fresh(g, None) is g


def test_a_contribution_runs_at_its_stage_in_order_and_is_skipped_without_its_buffer():
    job = object.__new__(rs.RenderJob)
    log = []
    job.contributions = [rs.Contribution(rs.MeshGrads, ("verts",), lambda g: log.append("a")),
                         rs.Contribution(rs.ColourGrads, ("sh_dc", "densities"), lambda g: log.append("colour")),
                         rs.Contribution(rs.MeshGrads, ("verts",), lambda g: log.append("b")),
                         rs.Contribution(rs.MeshGrads, ("delta_t", "delta_r"), lambda g: log.append("deltas"))]
    t = torch.zeros(1)
    job.contribute(rs.ColourGrads(t, None, t))
    job.contribute(rs.MeshGrads(t, t, t, None, None))
    assert log == ["colour", "a", "b"]
    job.contribute(rs.MeshGrads(None, t, t, t, t))
    assert log == ["colour", "a", "b", "deltas"]


# ---------------------------------------------------------------------------------------------------- the parameters
@pytest.mark.parametrize("loose", [False, True], ids=["bound", "loosely bound"])
def test_render_params_and_the_needs_input_grad_derived_from_them(loose):
    m = _model(loose)
    p = m.render_params()
    assert p._fields == ("verts", "raw_scales", "raw_complex", "densities", "sh_dc", "sh_rest", "delta_t", "delta_r")
    assert list(inspect.signature(rs._RenderMeshBound.forward).parameters) == ["ctx", *p._fields, "job"]
    assert p.verts is m._points and p.raw_scales is m._scales and p.raw_complex is m._quaternions
    assert p.densities is m.all_densities and p.sh_dc is m._sh_coordinates_dc and p.sh_rest is m._sh_coordinates_rest
    if loose:
        assert p.delta_t is m._delta_t and p.delta_r is m._delta_r
    else:
        assert p.delta_t is None and p.delta_r is None
    assert p.needs_input_grad() == (True,) * 6 + (loose, loose) + (False,)
    m._scales.requires_grad_(False)
    m._sh_coordinates_rest.requires_grad_(False)
    if loose:
        m._delta_r.requires_grad_(False)
    assert m.render_params().needs_input_grad() == (True, False, True, True, True, False, loose, False, False)
    if loose:                                         # the deltas stay and are ignored again
        m.rebind()
        assert m.render_params().delta_t is None and m.render_params().needs_input_grad()[6:] == (False, False, False)


def test_the_loss_nodes_name_their_differentiable_inputs_once():
    """needs_input_grad and the backward's return value come from N_INPUTS / GRAD_AT, which match forward's signature."""
    for node, names in ((losses._L1DSSIM, ["pred"]), (losses._DepthL1, ["pred"]), (losses._RGBDepthLoss, ["img6"]),
                        (losses._SurfaceMeshLoss, ["verts"]), (losses._MeshSmoothnessLoss, ["verts"]),
                        (losses._GaussianParamLoss, ["delta_t", "delta_r", "densities", "sh_dc"])):
        inputs = list(inspect.signature(node.forward).parameters)[1:]
        assert len(inputs) == node.N_INPUTS and [inputs[i] for i in node.GRAD_AT] == names
    t, frozen = torch.zeros(1, requires_grad=True), torch.zeros(1)
    assert losses.needs_input_grad(losses._GaussianParamLoss, t, None, frozen, t) == (
        True, False, False, False, False, False, False, True, False, False)
    assert losses.needs_input_grad(losses._SurfaceMeshLoss, t) == (True,) + (False,) * 6
    assert losses.at_inputs(losses._GaussianParamLoss, "abcd") == ("a", "b", None, None, None, "c", None, "d", None, None)
    assert losses.at_inputs(losses._MeshSmoothnessLoss, ()) == (None,) * 5


# ---------------------------------------------------------------------------------------------------- the two dict parsers
def _fake_forward(monkeypatch, node, calls):
    """node.forward replaced by one that records its arguments by name, saves a tensor (so the term has a backward) and
    returns a total."""
    sig = inspect.signature(node.forward)

    def forward(ctx, *args):
        calls.append((node.__name__, sig.bind(ctx, *args).arguments))
        ctx.save_for_backward(torch.zeros(1))
        return torch.tensor(float(len(calls))), None
    monkeypatch.setattr(node, "forward", staticmethod(forward))


@pytest.fixture
def calls(monkeypatch):
    out = []
    for node in (losses._SurfaceMeshLoss, losses._MeshSmoothnessLoss, losses._GaussianParamLoss):
        _fake_forward(monkeypatch, node, out)
    return out


SCALE = torch.ones(())


def test_mesh_reg_parser(calls, monkeypatch):
    m = _model(False)
    own_topology = object()
    monkeypatch.setattr(m, "mesh_topology", lambda: own_topology)
    terms = rs._mesh_reg_terms(m, dict(nc_factor=0.5), SCALE)                       # the defaults: one node
    assert [n for n, _ in calls] == ["_SurfaceMeshLoss"]
    a = calls[0][1]
    assert a["verts"] is m._points and a["topo"] is own_topology and a["ctx"].needs_input_grad == (True,) + (False,) * 6
    assert (a["nc_factor"], a["ref_edge_len"], a["edge_factor"], a["ref_area"], a["area_factor"]) == (0.5, None, 0.0, None, 0.0)
    assert len(terms) == 1 and float(terms[0][0]) == 1.0
    (c,) = terms[0][1]
    assert c.stage is rs.MeshGrads and c.needs == ("verts",)
    del calls[:]
    topo, re_, ra = object(), torch.ones(3), torch.ones(2)
    terms = rs._mesh_reg_terms(m, dict(topology=topo, nc_factor=1, ref_edge_len=re_, edge_factor=2, ref_area=ra, area_factor=3,
                                       laplacian_factor=4, laplacian_method="cotcurv", area_reg_factor=5), SCALE)
    assert [n for n, _ in calls] == ["_SurfaceMeshLoss", "_MeshSmoothnessLoss"] and len(terms) == 2
    a, b = calls[0][1], calls[1][1]
    assert a["topo"] is topo and a["ref_edge_len"] is re_ and a["ref_area"] is ra
    assert (a["nc_factor"], a["edge_factor"], a["area_factor"]) == (1.0, 2.0, 3.0)
    assert b["verts"] is m._points and b["topo"] is topo and b["ctx"].needs_input_grad == (True,) + (False,) * 4
    assert (b["laplacian_factor"], b["method"], b["area_reg_factor"]) == (4.0, "cotcurv", 5.0)
    assert [c.stage for _t, cs in terms for c in cs] == [rs.MeshGrads, rs.MeshGrads]
    del calls[:]
    rs._mesh_reg_terms(m, dict(nc_factor=0.5, area_reg_factor=0.1), SCALE)          # one of the two factors is enough,
    assert calls[1][1]["method"] == "uniform"                                       # "uniform" is the default
    del calls[:]
    rs._mesh_reg_terms(m, dict(nc_factor=0.5, laplacian_factor=0.0, area_reg_factor=0.0), SCALE)
    assert [n for n, _ in calls] == ["_SurfaceMeshLoss"]
    with pytest.raises(ValueError, match="Method should be one of {uniform, cot, cotcurv}"):
        rs._mesh_reg_terms(m, dict(nc_factor=0.5, laplacian_factor=1.0, laplacian_method="cotan"), SCALE)
    with pytest.raises(TypeError, match="mesh_reg: unexpected keys .'nonsense'."):
        rs._mesh_reg_terms(m, dict(nc_factor=0.5, nonsense=1), SCALE)
    m._points.requires_grad_(False)                                                 # frozen vertices: no backward share
    del calls[:]
    rs._mesh_reg_terms(m, dict(nc_factor=0.5), SCALE)
    assert calls[0][1]["ctx"].needs_input_grad == (False,) * 7


def test_param_reg_parser(calls):
    m = _model(True)
    w = torch.rand(m.n_points)
    m.loose_bind(w)
    ((total, contributions),) = rs._param_reg_terms(m, {}, SCALE)                   # the defaults
    a = calls[0][1]
    assert a["delta_t"] is m._delta_t and a["delta_r"] is m._delta_r and a["weight"] is m.unbind_loss_weight
    assert (a["factor_t"], a["factor_r"], a["min_opacity"], a["sh_factor"]) == (100.0, 1.0, 0.8, 1.0)
    assert a["densities"] is m.all_densities
    assert a["sh_dc"] is None and a["pre_sh_dc"] is None                            # no pre_sh_dc: no SH term
    assert a["ctx"].needs_input_grad == (True, True, False, False, False, True, False, False, False, False)
    assert float(total) == 1.0
    assert [(c.stage, c.needs) for c in contributions] == [(rs.ColourGrads, ("sh_dc", "densities")),
                                                          (rs.MeshGrads, ("delta_t", "delta_r"))]
    del calls[:]
    pre, w2 = torch.zeros(4, 3), torch.ones(m.n_points)
    rs._param_reg_terms(m, dict(factor_t=2, factor_r=3, min_opacity=None, pre_sh_dc=pre, sh_factor=4, weight=w2), SCALE)
    a = calls[0][1]
    assert a["densities"] is None and a["min_opacity"] == 0.0                       # min_opacity=None: the opacity term is off
    assert a["sh_dc"] is m._sh_coordinates_dc and a["pre_sh_dc"] is pre and a["weight"] is w2
    assert (a["factor_t"], a["factor_r"], a["sh_factor"]) == (2.0, 3.0, 4.0)
    assert a["ctx"].needs_input_grad == (True, True, False, False, False, False, False, True, False, False)
    with pytest.raises(TypeError, match="param_reg: unexpected keys .'nonsense'."):
        rs._param_reg_terms(m, dict(nonsense=1), SCALE)
    m.rebind()                                                                      # a bound model: the loose terms are off
    del calls[:]
    rs._param_reg_terms(m, dict(pre_sh_dc=pre), SCALE)
    a = calls[0][1]
    assert a["delta_t"] is None and a["delta_r"] is None and a["weight"] is None
    assert a["densities"] is m.all_densities and a["sh_dc"] is m._sh_coordinates_dc
    assert a["ctx"].needs_input_grad == (False, False, False, False, False, True, False, True, False, False)


def test_the_step_lives_in_refine_step_and_harness_still_names_it():
    assert harness._PlainCtx is rs._PlainCtx and harness._RenderMeshBound is rs._RenderMeshBound
    m = _model(False)
    m.grad_sink = object()                            # not a sink: said when a render is made, not at assignment
    cam = harness.nerf_camera_from_scene(scene.look_at_camera((0.5, 1.6, 3.0), scene.SUBJECT_CENTER, 32, 24, focal_px=26.0))
    with pytest.raises(TypeError, match="grad_sink must provide"):
        rs.RenderJob(m, cam, torch.zeros(3), None, 0, True)
    with pytest.raises(ValueError, match="depth_channels must be 0, 1 or 3"):
        rs.RenderJob(m, cam, torch.zeros(3), None, 2, True)
    m.grad_sink = None
    job = rs.RenderJob(m, cam, torch.zeros(4), None, 1, False)
    assert job.params == m.render_params() and job.sh_levels == 2 and job.depth_channels == 1 and job.grad is False
    assert job.contributions == [] and job.sink is None and (job.lo, job.hi) == (float("-inf"), float("inf"))
    with pytest.raises(AttributeError):
        job.verts_grad_hook = None                    # slots: a misspelt field is an error, not "no hook"
