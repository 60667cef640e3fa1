"""GPU: the order of one refinement step (gaustar_amd/refine_step.py) -- which C entry points SurfaceGaussians.rgbd_step and
the backward of render_channels call, in which order, and where in that order a gradient sink hears `written`."""
import pytest
import torch

from test_gpu_launch_rule import _spy
from test_gpu_param_reg import _small_model

pytestmark = pytest.mark.gpu
SMOOTH = dict(laplacian_factor=5.0, laplacian_method="cot", area_reg_factor=0.1)
# (which of its entry points the rasterizer's forward takes -- fused or planned, with or without a second stage -- is its own
# host driver's choice from the plans and the size hint the process has cached: one entry in the record)
RASTERIZER_FORWARD = {"gsr_forward_fused", "gsr_forward_planned", "gsr_forward_stage2_mt"}

STEP = [
    "gsr_mesh_gaussians", "gsr_sh_colors_split", "<rasterizer forward>",
    "gsr_mesh_reg_forward", "gsr_mesh_lap_forward", "gsr_param_reg_forward", "gsr_rgb_depth_loss",
    "gsr_rgb_depth_loss_backward", "gsr_backward_mt",
    "gsr_sh_colors_split_backward", "gsr_param_reg_backward",
    "written:_sh_coordinates_dc,_sh_coordinates_rest,all_densities",
    "gsr_mesh_gaussians_backward", "gsr_mesh_reg_backward", "gsr_mesh_lap_backward", "gsr_param_reg_backward",
    "written:_points,_scales,_quaternions,_delta_t,_delta_r",
]
RENDER_BACKWARD = [
    "gsr_mesh_gaussians", "gsr_sh_colors_split", "<rasterizer forward>",
    "gsr_backward_mt",
    "gsr_sh_colors_split_backward",
    "written:_sh_coordinates_dc,_sh_coordinates_rest,all_densities",
    "gsr_mesh_gaussians_backward",
    "written:_points,_scales,_quaternions,_delta_t,_delta_r",
]


class _LoggingSink:
    """A gradient sink that accepts every parameter and writes `written:<names>` into the spy's record."""

    def __init__(self, model, log):
        self.names = {id(p): n for n, p in model.named_parameters()}
        self.views = {id(p): torch.zeros_like(p) for p in model.parameters()}
        self.log = log

    def grad_views(self):
        return self.views

    def accepts(self, p):
        return True

    def written(self, params):
        self.log.append("written:" + ",".join(self.names[id(p)] for p in params))


def _record(log):
    out = []
    for name in log:
        name = "<rasterizer forward>" if name in RASTERIZER_FORWARD else name
        if not (out and out[-1] == name == "<rasterizer forward>"):
            out.append(name)
    del log[:]
    return out


def test_entry_points_and_sink_notifications_in_order(hip_lib, monkeypatch):
    """One rgbd_step on a loosely bound model with every regulariser on, and one backward of render_channels, both into a sink:
    the record of C entry points and `written` notifications equals STEP / RENDER_BACKWARD.  The two lists were recorded with
    this very spy and sink from the commit BEFORE the step moved into refine_step.py (96ab435), not from the code under test:
    the regularisers' shares land after their producer's backward and before that stage's `written` -- colour stage: the
    parameter regulariser's; mesh stage: surface-mesh, smoothness, parameter regulariser's."""
    model, cam, bg4, gt_rgb, gt_d, param_reg, mesh_reg = _small_model()
    step = lambda: model.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, 0.2, 1.0, 0.5, mesh_reg=dict(mesh_reg, **SMOOTH), param_reg=param_reg)
    step()                                       # (topology lists, plans and hints are built: the record is a steady-state step)
    log = _spy(monkeypatch, hip_lib, model.device, never_null=False)
    model.grad_sink = _LoggingSink(model, log)
    try:
        for p in model.parameters():
            p.grad = None
        step()
        got_step = _record(log)
        for p in model.parameters():
            p.grad = None
        image = model.render_channels(cam, bg4, depth_channels=1)[0]
        image.backward(torch.ones_like(image))
        got_render = _record(log)
    finally:
        model.grad_sink = None
    print("[refine_step] step:", got_step)
    print("[refine_step] render + backward:", got_render)
    assert got_step == STEP
    assert got_render == RENDER_BACKWARD
