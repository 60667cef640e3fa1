"""The refinement step's host driver: the render of mesh-bound Gaussians as ONE autograd node and the
graph-free iteration built on it.

    RenderParams      the eight tensors a render reads, by name (SurfaceGaussians.render_params())
    RenderJob         everything else a render needs, fixed when the call is made
    GradHandoff       where the backward's parameter gradients are written and who hears that they are final
    Contribution      a loss term's share of a stage's gradients, added between the producer's backward and the hand-off
    _RenderMeshBound  the node: forward(ctx, *RenderParams, job)
    rgbd_step         render + image losses + regularisers + backward on plain contexts (SurfaceGaussians.rgbd_step)

This is per-iteration host code of a loop the host can bound (_host.py): slots, no class made per step, no validation pass."""
from __future__ import annotations

from typing import Callable, NamedTuple, Optional, Tuple

import torch

from . import losses as _losses, producers, rasterizer as _rasterizer


class RenderParams(NamedTuple):
    """The inputs of _RenderMeshBound.forward, in its signature's order.  delta_t / delta_r are None unless the model is
    loosely bound.  Also the shape of what its backward returns."""
    verts: Optional[torch.Tensor]
    raw_scales: Optional[torch.Tensor]
    raw_complex: Optional[torch.Tensor]
    densities: Optional[torch.Tensor]
    sh_dc: Optional[torch.Tensor]
    sh_rest: Optional[torch.Tensor]
    delta_t: Optional[torch.Tensor]
    delta_r: Optional[torch.Tensor]

    def needs_input_grad(self) -> Tuple[bool, ...]:
        """What autograd would put into ctx.needs_input_grad for forward(ctx, *self, job)."""
        return tuple(p is not None and p.requires_grad for p in self) + (False,)


class ColourGrads(NamedTuple):
    """The colour stage of the backward: what the colour producer's backward leaves (70 % of the bytes)."""
    sh_dc: Optional[torch.Tensor]
    sh_rest: Optional[torch.Tensor]
    densities: Optional[torch.Tensor]


class MeshGrads(NamedTuple):
    """The mesh stage of the backward: what the mesh producer's backward leaves."""
    verts: Optional[torch.Tensor]
    raw_scales: Optional[torch.Tensor]
    raw_complex: Optional[torch.Tensor]
    delta_t: Optional[torch.Tensor]
    delta_r: Optional[torch.Tensor]


class Contribution(NamedTuple):
    """`add(grads)` adds a loss term's share in place to a stage's gradient buffers: stage = ColourGrads or MeshGrads, grads an
    instance of it.  Called after that stage's producer backward and before a sink hears `written`, in the order of
    RenderJob.contributions; skipped when one of the buffers it `needs` (field names of the stage) is None."""
    stage: type
    needs: Tuple[str, ...]
    add: Callable


class RenderJob:
    """What _RenderMeshBound needs besides the parameters (render_channels, rgbd_step), checked once, here."""
    __slots__ = ("settings", "faces", "bary", "depth_channels", "thickness", "lo", "hi", "sh_levels", "sink", "grad", "params",
                 "contributions")

    def __init__(self, model, camera, bg: torch.Tensor, sh_deg: Optional[int], depth_channels: int, grad: bool):
        if depth_channels not in (0, 1, 3):
            raise ValueError("depth_channels must be 0, 1 or 3")
        self.settings, _view, _campos = model._settings(camera, bg, 0)
        producers._check_faces(model._surface_mesh_faces, int(model._points.shape[0]))
        if model._surface_mesh_faces.dtype != torch.int64 or not model._surface_mesh_faces.is_contiguous():
            # (the one-node render hands the buffer to the kernels as a raw pointer: a strided or int32 replacement of the
            # registered buffer would be read with the wrong layout)
            model._surface_mesh_faces = model._surface_mesh_faces.long().contiguous()
        self.faces, self.bary, self.depth_channels = model._surface_mesh_faces, model._bary_rows(), int(depth_channels)
        self.thickness = model._thickness()
        self.lo = float("-inf") if model.min_gaussian_scale is None else float(model.min_gaussian_scale)
        self.hi = float("inf") if model.max_gaussian_scale is None else float(model.max_gaussian_scale)
        self.sh_levels = (model.sh_levels - 1 if sh_deg is None else int(sh_deg)) + 1
        self.sink = sink = getattr(model, "grad_sink", None)
        self.grad = bool(grad)   # (Function.forward cannot tell whether the caller runs under no_grad: see rasterizer._CALL)
        self.params = model.render_params()
        self.contributions = []
        if self.settings.campos.device != model.device or self.settings.campos.dtype != torch.float32:
            raise RuntimeError("camera matrices must be float32 tensors on the model's device")
        if sink is not None and not (hasattr(sink, "grad_views") and hasattr(sink, "written") and hasattr(sink, "accepts")):
            raise TypeError("grad_sink must provide grad_views(), accepts(p) and written(params) (gaustar_amd.dist.ShardedAdam)")

    def contribute(self, grads) -> None:
        """Every contribution to the stage `grads` is an instance of, in order."""
        for c in self.contributions:
            if c.stage is type(grads) and all(getattr(grads, n) is not None for n in c.needs):
                c.add(grads)


class GradHandoff:
    """One backward's hand-off of parameter gradients to a gradient sink (dist.ShardedAdam: views of its flat gradient buffer):
    the gradients are written where the reduce-scatter reads them, and the sink hears about a stage's -- the colour producer's
    first -- BEFORE the next producer's backward is launched, so their buckets leave while that one still runs.  Without a sink
    every buffer is None and nobody is told."""
    __slots__ = ("_sink", "_views", "_open")

    def __init__(self, sink):
        self._sink, self._views, self._open = sink, (sink.grad_views() if sink is not None else None), ()

    def take(self, *params):
        """-> per parameter the sink's buffer to write its gradient into, or None: no sink, no such parameter, or one the sink
        does not accept (accepts(): first delivery of this step only -- a second render under the same loss goes through
        autograd's own addition).  Opens a stage: written() speaks of these parameters."""
        sink, views = self._sink, self._views
        if sink is None:
            return (None,) * len(params)
        bufs = tuple(views.get(id(p)) if (p is not None and sink.accepts(p)) else None for p in params)
        self._open = [p for p, o in zip(params, bufs) if o is not None]
        return bufs

    def written(self) -> None:
        """The buffers of the stage take() opened are final."""
        if self._sink is not None:
            self._sink.written(self._open)
            self._open = ()

    @staticmethod
    def fresh(grad, buf):
        """What goes back to autograd for a gradient written into `buf`: a FRESH tensor object on the same storage.
        AccumulateGrad adopts an incoming gradient as p.grad only if nobody else holds that tensor object -- the optimiser's
        cached views would make it clone all 77 MB instead.  Without a buffer: the gradient as it is."""
        return grad if (grad is None or buf is None) else grad.view(grad.shape)


class _PlainCtx:
    """Stand-in for an autograd context: lets rgbd_step run the Functions' forward / backward bodies directly."""
    __slots__ = ("needs_input_grad", "saved_tensors", "__dict__")

    def __init__(self, needs_input_grad):
        self.needs_input_grad, self.saved_tensors = needs_input_grad, ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        pass

    def set_materialize_grads(self, value):
        pass


class _RenderMeshBound(torch.autograd.Function):
    """A render of mesh-bound Gaussians as ONE autograd node: the model's parameters in, the image out.  Forward = mesh
    producer -> colour producer (coefficients read from `_sh_coordinates_dc` / `_sh_coordinates_rest` where they live,
    sigmoid of the densities from the same kernel) -> rasterizer; backward = the three backward calls in reverse, the
    colour producer's gradient w.r.t. the positions added in place to the rasterizer's.  The same kernels on the same
    numbers as the composition of autograd nodes in render_image_gaussian_rasterizer -- what goes away is what autograd puts
    between them per iteration at config-C size: torch.cat of the coefficients and the two copies that split its gradient
    (53 MB each way), sigmoid and its backward, the add of the two position gradients, the zero fill of the screen-space
    gradient carrier, and five graph nodes' worth of host work (tools/window_phases.py)."""

    @staticmethod
    def forward(ctx, verts, raw_scales, raw_complex, densities, sh_dc, sh_rest, delta_t, delta_r, job):
        dev = verts.device
        x = RenderParams(*[None if t is None else _rasterizer._dev_f32(t.detach(), dev)
                           for t in (verts, raw_scales, raw_complex, densities, sh_dc, sh_rest, delta_t, delta_r)])
        st, p = job.settings, job.params
        D, M = job.sh_levels - 1, 1 + int(x.sh_rest.size(1))
        view = st.viewmatrix if job.depth_channels else None
        # A sharded optimiser may have left the all-gather of some parameters in flight (dist.ShardedAdam(gather_first=...)):
        # each producer's inputs are fenced right before it is launched, so the mesh producer runs under the SH buckets' gather
        fence = getattr(job.sink, "wait_params", None)
        if fence is not None:
            fence((p.verts, p.raw_scales, p.raw_complex, p.delta_t, p.delta_r))
        need_bwd = any(ctx.needs_input_grad) and job.grad
        # (without a gradient sink the backward's vertex-gradient accumulator is made here and cleared by the forward's launch)
        need_verts = RenderParams._make(ctx.needs_input_grad[:-1]).verts
        ctx.d_verts = torch.empty_like(x.verts) if need_bwd and need_verts and job.sink is None else None
        points, scaling, quats = producers._mesh_forward_raw(x.verts, job.faces, job.bary, x.raw_scales, x.raw_complex, job.thickness,
                                                             job.lo, job.hi, x.delta_t, x.delta_r, clear=ctx.d_verts)
        if fence is not None:
            fence((p.sh_dc, p.sh_rest, p.densities))
        colors, opac = producers._sh_forward_raw(points, st.campos, x.sh_dc, x.sh_rest, D, M, view, job.depth_channels, x.densities)
        box = []
        out = _rasterizer.rasterize_gaussians_native(
            st.bg, points, colors, opac, scaling, quats, st.scale_modifier, None, st.viewmatrix, st.projmatrix, st.tanfovx,
            st.tanfovy, st.image_height, st.image_width, None, 0, st.campos, st.prefiltered, st.debug, need_backward=need_bwd,
            scratch_box=box)
        num_rendered, color, radii, geom, binning, img, _max_tile, num_segments = out
        ctx.save_for_backward(x.verts, x.raw_scales, x.raw_complex, x.delta_r, x.sh_dc, x.sh_rest, points, scaling, quats, colors,
                              opac, radii, geom, binning, img)
        ctx.job, ctx.counts = job, (num_rendered, num_segments, D, M, x.delta_t is not None, tuple(densities.shape))
        ctx.zeroed_scratch = box[0] if box else None
        ctx.mark_non_differentiable(radii)
        ctx.set_materialize_grads(False)
        return color, radii

    @staticmethod
    def backward(ctx, grad_color, _):
        if grad_color is None:
            return (None,) * 9
        v, rs, rc, dr, dc, rest, points, scaling, quats, colors, opac, radii, geom, binning, img = ctx.saved_tensors
        job, (num_rendered, num_segments, D, M, has_dt, dens_shape) = ctx.job, ctx.counts
        st, p = job.settings, job.params
        zeroed, ctx.zeroed_scratch = ctx.zeroed_scratch, None
        _dm2d, d_colors, d_opac, d_points, _dcov, _dsh, d_scaling, d_quats = _rasterizer.rasterize_gaussians_backward_native(
            st.bg, points, radii, colors, scaling, quats, st.scale_modifier, None, st.viewmatrix, st.projmatrix, st.tanfovx,
            st.tanfovy, grad_color, None, 0, st.campos, geom, num_rendered, binning, img, st.debug, num_segments=num_segments,
            zeroed_scratch=zeroed)
        view = st.viewmatrix if job.depth_channels else None
        hand = GradHandoff(job.sink)
        # the colour stage (a model of one SH level has no rest coefficients to write)
        o_colour = hand.take(p.sh_dc, p.sh_rest if M > 1 else None, p.densities)
        d_dc, d_rest, _, d_dens = producers._sh_backward_raw(points, _rasterizer._dev_f32(st.campos, points.device), dc, rest, D, M,
                                                             _rasterizer._dev_f32(view, points.device), job.depth_channels, d_colors,
                                                             opac, d_opac, dpos_inout=d_points, out=o_colour)
        job.contribute(ColourGrads(d_dc, d_rest, d_dens))
        hand.written()
        # the mesh stage
        o_mesh = hand.take(p.verts, p.raw_scales, p.raw_complex, p.delta_t, p.delta_r)
        pre, ctx.d_verts = getattr(ctx, "d_verts", None), None      # (cleared by the forward: good for one backward)
        cleared = o_mesh[0] is None and pre is not None
        d_mesh = MeshGrads(*producers._mesh_backward_raw(v, job.faces, job.bary, rs, rc, dr, job.lo, job.hi, has_dt, d_points, d_scaling,
                                                         d_quats, out=(pre,) + o_mesh[1:] if cleared else o_mesh, verts_cleared=cleared))
        job.contribute(d_mesh)
        hand.written()
        o_mesh, fresh = MeshGrads(*o_mesh), hand.fresh
        return RenderParams(verts=fresh(d_mesh.verts, o_mesh.verts), raw_scales=fresh(d_mesh.raw_scales, o_mesh.raw_scales),
                            raw_complex=fresh(d_mesh.raw_complex, o_mesh.raw_complex), densities=d_dens.view(dens_shape),
                            sh_dc=fresh(d_dc, o_colour[0]), sh_rest=fresh(d_rest, o_colour[1]),
                            delta_t=fresh(d_mesh.delta_t, o_mesh.delta_t), delta_r=fresh(d_mesh.delta_r, o_mesh.delta_r)) + (None,)


# ---------------------------------------------------------------------------------------- the graph-free iteration
def _vertex_term(node, model, args, scale):
    """A loss node over the vertices, forward now -> (its total, its contributions: the share of the vertex gradient)."""
    ctx = _PlainCtx(_losses.needs_input_grad(node, model._points))
    total, _parts = node.forward(ctx, model._points, *args)
    if not ctx.saved_tensors:
        return total, []
    return total, [Contribution(MeshGrads, ("verts",), lambda g: node.grad_into(ctx, scale, g.verts, 1))]


def _mesh_reg_terms(model, mesh_reg: dict, scale):
    """rgbd_step's mesh_reg: the keyword arguments of losses.surface_mesh_loss (`topology` defaults to mesh_topology()) and, in
    the same dict, of losses.mesh_smoothness_loss as laplacian_factor, laplacian_method ("uniform") and area_reg_factor -- that
    node runs only when one of its two factors is not 0.  -> [(total, contributions)] in the order they are summed."""
    kw = dict(mesh_reg)
    topo = kw.pop("topology", None) or model.mesh_topology()
    surface = (topo, float(kw.pop("nc_factor")), kw.pop("ref_edge_len", None), float(kw.pop("edge_factor", 0.0)),
               kw.pop("ref_area", None), float(kw.pop("area_factor", 0.0)))
    smooth = (topo, float(kw.pop("laplacian_factor", 0.0)), kw.pop("laplacian_method", "uniform"), float(kw.pop("area_reg_factor", 0.0)))
    smooth_on = smooth[1] != 0.0 or smooth[3] != 0.0
    if smooth_on and smooth[2] not in _losses._LAP_METHODS:
        raise ValueError("Method should be one of {uniform, cot, cotcurv}")
    if kw:
        raise TypeError(f"mesh_reg: unexpected keys {sorted(kw)}")
    terms = [_vertex_term(_losses._SurfaceMeshLoss, model, surface, scale)]
    if smooth_on:
        terms.append(_vertex_term(_losses._MeshSmoothnessLoss, model, smooth, scale))
    return terms


def _param_reg_terms(model, param_reg: dict, scale):
    """rgbd_step's param_reg: the scalar keyword arguments of losses.gaussian_param_loss (min_opacity=None switches the opacity
    term off), optional `pre_sh_dc` (without it there is no SH term) and `weight` (default: unbind_loss_weight).  The tensors are
    the model's own parameters; the loose-bind terms are on only while is_loose_bind().  -> [(total, contributions)]."""
    kw = dict(param_reg)
    min_op, pre = kw.pop("min_opacity", 0.8), kw.pop("pre_sh_dc", None)
    weight = kw.pop("weight", None)
    if weight is None:
        weight = getattr(model, "unbind_loss_weight", None)
    factor_t, factor_r, sh_factor = float(kw.pop("factor_t", 100.0)), float(kw.pop("factor_r", 1.0)), float(kw.pop("sh_factor", 1.0))
    if kw:
        raise TypeError(f"param_reg: unexpected keys {sorted(kw)}")
    p, node = model.render_params(), _losses._GaussianParamLoss
    p_dt, p_dr = p.delta_t, p.delta_r                                  # (None on a bound model)
    p_dens, p_dc = p.densities if min_op is not None else None, p.sh_dc if pre is not None else None
    ctx = _PlainCtx(_losses.needs_input_grad(node, p_dt, p_dr, p_dens, p_dc))
    total, _parts = node.forward(ctx, p_dt, p_dr, weight if p_dt is not None else None, factor_t, factor_r, p_dens,
                                 0.0 if min_op is None else float(min_op), p_dc, pre, sh_factor)
    if not ctx.saved_tensors:
        return [(total, [])]
    on = lambda q, buf: buf if (q is not None and q.requires_grad) else None
    return [(total, [
        Contribution(ColourGrads, ("sh_dc", "densities"),
                     lambda g: node.grad_into(ctx, scale, (None, None, on(p_dens, g.densities), on(p_dc, g.sh_dc)), 1)),
        Contribution(MeshGrads, ("delta_t", "delta_r"),
                     lambda g: node.grad_into(ctx, scale, (on(p_dt, g.delta_t), on(p_dr, g.delta_r), None, None), 1))])]


def _unit_scale(model, dev):
    one = getattr(model, "_one_cache", None)
    if one is None or one.device != dev:
        one = model._one_cache = torch.ones((), device=dev)
    return one


def rgbd_step(model, camera, bg, gt_rgb, gt_depth, max_depth, dssim_factor=0.2, depth_factor=1.0, mask_factor=1.0, grad_scale=None,
              sh_deg=None, mesh_reg=None, param_reg=None):
    """SurfaceGaussians.rgbd_step: the nodes' forward / backward bodies run back to back on plain contexts."""
    image_loss = _losses._RGBDepthLoss
    with torch.no_grad():
        job = RenderJob(model, camera, bg, sh_deg, 1, True)
        params = job.params
        rctx = _PlainCtx(params.needs_input_grad())
        image, radii = _RenderMeshBound.forward(rctx, *params, job)
        scale = _unit_scale(model, image.device) if grad_scale is None else grad_scale
        terms = _mesh_reg_terms(model, mesh_reg, scale) if mesh_reg is not None else []
        if param_reg is not None:
            terms += _param_reg_terms(model, param_reg, scale)
        lctx = _PlainCtx(_losses.at_inputs(image_loss, (True,), False))
        loss, _parts = image_loss.forward(lctx, image, gt_rgb, gt_depth, float(dssim_factor), None, float(max_depth),
                                          float(depth_factor), float(mask_factor))
        for total, contributions in terms:
            loss = loss + total
            job.contributions += contributions
        d_image = image_loss.backward(lctx, scale, None)[0]
        grads = _RenderMeshBound.backward(rctx, d_image, None)
        for p, g in zip(params, grads):
            if p is None or g is None or not p.requires_grad:
                continue
            if p.grad is None:
                p.grad = g
            else:
                p.grad.add_(g)
    return loss, image, radii
