"""Image-space losses of the GauSTAR refinement loop as fused HIP ops.

Host-side mirror of gaustar_utils/loss_utils.py (`l1_loss`, `ssim`) and of the loss assembly in
gaustar_trainers/refine.py:451-453 (`(1 - f) * l1 + f * (1 - ssim)`, on the margin-cropped view of
:584-594) and :634-660 (masked depth + silhouette L1).  Each op is ONE call into libgsr_hip.so that returns
the loss value; the gradient pass is a second call made from autograd's backward, which hands the kernels the incoming
scalar as a DEVICE pointer, so d loss / d pred leaves them final (no elementwise multiply over the image).  The gradient
w.r.t. the ground-truth image is not provided (the trainer never needs it).

There is no CPU path: CPU tensors raise, like the rasterizer (gaustar_amd/rasterizer.py).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Sequence

import torch

from . import _host, _lib
from ._host import current_stream as _stream
from ._lib import ptr as _vp


def at_inputs(node, values, fill=None):
    """A tuple with one entry per input of node.forward: `values` at the node's differentiable inputs (node.GRAD_AT, in that
    order), `fill` at the others.  Both a backward's return value and a plain context's needs_input_grad are made here."""
    out = [fill] * node.N_INPUTS
    for i, x in zip(node.GRAD_AT, values):
        out[i] = x
    return tuple(out)


def needs_input_grad(node, *inputs):
    """What autograd would put into ctx.needs_input_grad, from the node's differentiable inputs in GRAD_AT order."""
    return at_inputs(node, [t is not None and t.requires_grad for t in inputs], False)


def _scratch(n_bytes, n_out, dev):
    """-> (the workspace, the float32 vector of parts a forward's kernel fills), both uninitialised."""
    return torch.empty(n_bytes, dtype=torch.uint8, device=dev), torch.empty(n_out, dtype=torch.float32, device=dev)


def _finish(ctx, node, parts, saved):
    """The common tail of the forwards: `saved` is kept only if a backward will ask for it, and the parts vector carries no
    gradient -- nor gets a zero-filled one per backward (one fill kernel)."""
    if any(ctx.needs_input_grad[i] for i in node.GRAD_AT):
        ctx.save_for_backward(*saved)
    ctx.mark_non_differentiable(parts)
    ctx.set_materialize_grads(False)


def _backward_into_fresh(node, ctx, g_loss):
    """The backward of a node over the vertices: its grad_into on a fresh buffer."""
    if not ctx.saved_tensors or g_loss is None:
        return at_inputs(node, ())
    grad = node.grad_into(ctx, g_loss, torch.empty_like(ctx.saved_tensors[0]), 0)
    return at_inputs(node, (grad.to(ctx.in_dtype),))


def _chw_view(t: torch.Tensor, what: str) -> torch.Tensor:
    """[C,H,W] or [1,C,H,W] float32 HIP tensor, any strides (views are used as they are, never copied)."""
    if not t.is_cuda:
        raise RuntimeError(f"gaustar_amd.losses: {what} must live on a HIP (cuda) device -- there is no CPU path")
    if t.dim() == 4 and t.size(0) == 1:
        t = t[0]
    if t.dim() != 3:
        raise RuntimeError(f"{what} must have dimensions (C, H, W) or (1, C, H, W), got {tuple(t.shape)}")
    if t.dtype != torch.float32:
        t = t.float()
    return t


def _crop(t: torch.Tensor, margin: Optional[Sequence[int]]) -> torch.Tensor:
    """refine.py:587: pred[..., m2:-m3, m0:-m1] with margin = (left, right, top, bottom)."""
    if margin is None:
        return t
    m0, m1, m2, m3 = (int(v) for v in margin)
    return t[..., m2:(-m3 if m3 else None), m0:(-m1 if m1 else None)]


def _scale_ptr(g_loss: torch.Tensor, dev):
    """autograd's incoming d(total)/d(loss) as a float32 device scalar the gradient kernels read (no host sync, and no
    elementwise multiply over the image afterwards); the tensor is returned to keep it alive over the launch."""
    g = g_loss
    if g.dtype != torch.float32 or g.device != dev or g.dim() != 0 or not g.is_contiguous():
        g = g.detach().to(device=dev, dtype=torch.float32).reshape(()).contiguous()
    return g, _vp(g)


class _L1DSSIM(torch.autograd.Function):
    """Forward: the value pass (gsr_l1_ssim without a gradient buffer).  Backward: gsr_l1_ssim_backward from the workspace the
    value pass left, scaled by the incoming gradient ON THE DEVICE."""
    N_INPUTS, GRAD_AT = 4, (0,)

    @staticmethod
    def forward(ctx, pred, gt, dssim_factor, margin):
        lib = _lib.load()
        p_full = _chw_view(pred, "pred")
        g_full = _chw_view(gt, "gt")
        if p_full.shape != g_full.shape:
            raise RuntimeError(f"pred {tuple(p_full.shape)} and gt {tuple(g_full.shape)} differ in shape")
        p, g = _crop(p_full, margin), _crop(g_full, margin)
        C, H, W = (int(v) for v in p.shape)
        if H <= 0 or W <= 0:
            raise RuntimeError("the margin leaves an empty image")
        dev = p.device
        with _host.on_device(dev):
            ws, out = _scratch(lib.gsr_l1_ssim_workspace_bytes(C, H, W), 3, dev)
            _lib.check(lib.gsr_l1_ssim(
                C, H, W, _vp(p), p.stride(0), p.stride(1), p.stride(2),
                _vp(g), g.stride(0), g.stride(1), g.stride(2), float(dssim_factor),
                _vp(ws), _vp(out), None, 0, 0, 0, _stream()), "gsr_l1_ssim")
        ctx.cfg = (float(dssim_factor), margin, pred.shape, pred.dtype)
        _finish(ctx, _L1DSSIM, out, (p_full, g_full, ws))
        return out[0], out

    @staticmethod
    def backward(ctx, g_loss, _g_parts):
        if not ctx.saved_tensors or g_loss is None:
            return at_inputs(_L1DSSIM, ())
        lib = _lib.load()
        p_full, g_full, ws = ctx.saved_tensors
        f, margin, pred_shape, in_dtype = ctx.cfg
        p, g = _crop(p_full, margin), _crop(g_full, margin)
        C, H, W = (int(v) for v in p.shape)
        dev = p.device
        with _host.on_device(dev):
            # planar [C,H,W] -- the layout the backward blend reads; zero outside the crop
            grad_full = (torch.zeros if margin is not None else torch.empty)(p_full.shape, dtype=torch.float32, device=dev)
            gv = _crop(grad_full, margin)
            keep, sp = _scale_ptr(g_loss, dev)
            _lib.check(lib.gsr_l1_ssim_backward(
                C, H, W, _vp(p), p.stride(0), p.stride(1), p.stride(2),
                _vp(g), g.stride(0), g.stride(1), g.stride(2), f, _vp(ws), sp,
                _vp(gv), gv.stride(0), gv.stride(1), gv.stride(2), _stream()), "gsr_l1_ssim_backward")
        return at_inputs(_L1DSSIM, (grad_full.reshape(pred_shape).to(in_dtype),))


def l1_dssim_loss(pred: torch.Tensor, gt: torch.Tensor, dssim_factor: float = 0.2,
                  margin: Optional[Sequence[int]] = None, return_parts: bool = False):
    """(1 - f) * l1_loss(pred, gt) + f * (1 - ssim(pred, gt)) on pred[..., m2:-m3, m0:-m1] (refine.py:451-453,
    :584-594).  pred/gt: [C,H,W] or [1,C,H,W], any strides.  With return_parts also returns the device vector
    {loss, l1 mean, ssim mean} (no host sync anywhere)."""
    if gt.requires_grad:
        raise NotImplementedError("gaustar_amd.losses: no gradient w.r.t. the ground-truth image")
    loss, parts = _L1DSSIM.apply(pred, gt, float(dssim_factor), None if margin is None else tuple(margin))
    return (loss, parts) if return_parts else loss


def l1_loss(network_output: torch.Tensor, gt: torch.Tensor) -> torch.Tensor:
    """loss_utils.py:17-18."""
    return l1_dssim_loss(network_output, gt, 0.0)


def ssim(img1: torch.Tensor, img2: torch.Tensor, window_size: int = 11, size_average: bool = True) -> torch.Tensor:
    """loss_utils.py:33-43 with the defaults the trainer uses (window 11, mean over everything)."""
    if window_size != 11 or not size_average:
        raise NotImplementedError("gaustar_amd.losses.ssim: only window_size=11, size_average=True (the trainer's use)")
    return 1.0 - l1_dssim_loss(img1, img2, 1.0)


class _DepthL1(torch.autograd.Function):
    N_INPUTS, GRAD_AT = 5, (0,)

    @staticmethod
    def forward(ctx, pred, gt, max_depth, depth_factor, mask_factor):
        lib = _lib.load()
        if not pred.is_cuda:
            raise RuntimeError("gaustar_amd.losses: pred must live on a HIP (cuda) device -- there is no CPU path")
        if pred.dim() != 2 or pred.shape != gt.shape:
            raise RuntimeError(f"pred and gt must both be (H, W), got {tuple(pred.shape)} and {tuple(gt.shape)}")
        p = pred if pred.dtype == torch.float32 else pred.float()
        g = gt if gt.dtype == torch.float32 else gt.float()
        H, W = (int(v) for v in p.shape)
        dev = p.device
        with _host.on_device(dev):
            ws, out = _scratch(lib.gsr_depth_l1_workspace_bytes(), 4, dev)
            _lib.check(lib.gsr_depth_l1(
                H, W, _vp(p), p.stride(0), p.stride(1), _vp(g),
                g.stride(0), g.stride(1), float(max_depth), float(depth_factor), float(mask_factor),
                _vp(ws), _vp(out), None, 0, 0, _stream()), "gsr_depth_l1")
        ctx.cfg = (float(max_depth), float(depth_factor), float(mask_factor), pred.dtype)
        _finish(ctx, _DepthL1, out, (p, g, out))
        return out[0] + out[1], out

    @staticmethod
    def backward(ctx, g_loss, _g_parts):
        if not ctx.saved_tensors or g_loss is None:
            return at_inputs(_DepthL1, ())
        lib = _lib.load()
        p, g, out = ctx.saved_tensors
        max_depth, depth_factor, mask_factor, in_dtype = ctx.cfg
        H, W = (int(v) for v in p.shape)
        dev = p.device
        with _host.on_device(dev):
            grad = torch.empty(H, W, dtype=torch.float32, device=dev)
            keep, sp = _scale_ptr(g_loss, dev)
            _lib.check(lib.gsr_depth_l1_backward(
                H, W, _vp(p), p.stride(0), p.stride(1), _vp(g), g.stride(0),
                g.stride(1), max_depth, depth_factor, mask_factor, _vp(out), sp,
                _vp(grad), W, 1, _stream()), "gsr_depth_l1_backward")
        return at_inputs(_DepthL1, (grad.to(in_dtype),))


def depth_mask_l1_loss(pred_depth: torch.Tensor, gt_depth: torch.Tensor, max_depth: float, depth_factor: float = 1.0,
                       mask_factor: float = 1.0, return_parts: bool = False):
    """depth_factor * |pred - gt|.mean over {gt < max_depth} + mask_factor * |pred - max_depth|.mean over
    {gt > max_depth} (refine.py:634-660, depth_alpha = False).  parts = {depth term, mask term, #fg, #bg}."""
    loss, parts = _DepthL1.apply(pred_depth, gt_depth, float(max_depth), float(depth_factor), float(mask_factor))
    return (loss, parts) if return_parts else loss


class _RGBDepthLoss(torch.autograd.Function):
    """l1 + dssim on channels 0-2 and masked depth L1 on channel 3 of ONE [6,H,W] / [4,H,W] render.  Forward: both value
    passes and ONE reduction kernel (gsr_rgb_depth_loss) -> the total as a device scalar.  Backward: the two gradient passes
    write d(total)/d(render), scaled by the incoming gradient on the device, into ONE tensor (channels 4-5 zero)."""
    N_INPUTS, GRAD_AT = 8, (0,)

    @staticmethod
    def forward(ctx, img6, gt_rgb, gt_depth, dssim_factor, margin, max_depth, depth_factor, mask_factor):
        lib = _lib.load()
        if not img6.is_cuda:
            raise RuntimeError("gaustar_amd.losses: the render must live on a HIP (cuda) device -- there is no CPU path")
        if img6.dim() != 3 or img6.size(0) not in (4, 6):
            raise RuntimeError(f"the two-target render must have dimensions (6, H, W) or (4, H, W), got {tuple(img6.shape)}")
        x = img6 if img6.dtype == torch.float32 else img6.float()
        g_full = _chw_view(gt_rgb, "gt_rgb")
        if tuple(g_full.shape) != (3,) + tuple(x.shape[1:]):
            raise RuntimeError(f"gt_rgb {tuple(g_full.shape)} does not match the render {tuple(x.shape)}")
        if gt_depth.dim() != 2 or tuple(gt_depth.shape) != tuple(x.shape[1:]):
            raise RuntimeError(f"gt_depth must be (H, W) = {tuple(x.shape[1:])}, got {tuple(gt_depth.shape)}")
        gd = gt_depth if gt_depth.dtype == torch.float32 else gt_depth.float()
        p, g = _crop(x[:3], margin), _crop(g_full, margin)
        C, H, W = (int(v) for v in p.shape)
        if H <= 0 or W <= 0:
            raise RuntimeError("the margin leaves an empty image")
        d = x[3]
        Hd, Wd = (int(v) for v in d.shape)
        dev = x.device
        with _host.on_device(dev):
            ws, out = _scratch(lib.gsr_l1_ssim_workspace_bytes(C, H, W), 8, dev)   # {loss, l1, ssim | depth term, mask term, #fg, #bg | total}
            wd = torch.empty(lib.gsr_depth_l1_workspace_bytes(), dtype=torch.uint8, device=dev)
            _lib.check(lib.gsr_rgb_depth_loss(
                C, H, W, _vp(p), p.stride(0), p.stride(1), p.stride(2), _vp(g), g.stride(0), g.stride(1), g.stride(2),
                float(dssim_factor), _vp(ws), Hd, Wd, _vp(d), d.stride(0), d.stride(1), _vp(gd), gd.stride(0), gd.stride(1),
                float(max_depth), float(depth_factor), float(mask_factor), _vp(wd), _vp(out), _stream()), "gsr_rgb_depth_loss")
        ctx.cfg = (float(dssim_factor), margin, float(max_depth), float(depth_factor), float(mask_factor), img6.dtype)
        # (what backward reads -- the pixel counts the depth gradient divides by -- is the second copy of the eight numbers the
        # reduction kernel leaves in the workspace's tail (include/gsr.h), not the vector handed to the caller: `out` goes out
        # as it is, without the 32-byte device copy that used to separate the two)
        parts = out[:7]
        _finish(ctx, _RGBDepthLoss, parts, (x, g_full, gd, ws))
        return out[7], parts

    @staticmethod
    def backward(ctx, g_loss, _g_parts):
        if not ctx.saved_tensors or g_loss is None:
            return at_inputs(_RGBDepthLoss, ())
        lib = _lib.load()
        x, g_full, gd, ws = ctx.saved_tensors
        f, margin, max_depth, depth_factor, mask_factor, in_dtype = ctx.cfg
        p, g = _crop(x[:3], margin), _crop(g_full, margin)
        C, H, W = (int(v) for v in p.shape)
        d = x[3]
        Hd, Wd = (int(v) for v in d.shape)
        dev = x.device
        with _host.on_device(dev):
            grad6 = torch.empty_like(x, memory_format=torch.contiguous_format)
            if x.size(0) > 4:
                grad6[4:].zero_()
            if margin is not None:
                grad6[:3].zero_()
            gv, gdv = _crop(grad6[:3], margin), grad6[3]
            keep, sp = _scale_ptr(g_loss, dev)
            _lib.check(lib.gsr_rgb_depth_loss_backward(
                C, H, W, _vp(p), p.stride(0), p.stride(1), p.stride(2), _vp(g), g.stride(0), g.stride(1), g.stride(2), f, _vp(ws),
                Hd, Wd, _vp(d), d.stride(0), d.stride(1), _vp(gd), gd.stride(0), gd.stride(1), max_depth, depth_factor, mask_factor,
                ctypes.c_void_p(ws.data_ptr() + ws.numel() - 256), sp, _vp(gv), gv.stride(0), gv.stride(1), gv.stride(2), _vp(gdv),
                gdv.stride(0), gdv.stride(1), _stream()),
                "gsr_rgb_depth_loss_backward")
        return at_inputs(_RGBDepthLoss, (grad6.to(in_dtype),))


def rgb_depth_loss(render6: torch.Tensor, gt_rgb: torch.Tensor, gt_depth: torch.Tensor, max_depth: float,
                   dssim_factor: float = 0.2, depth_factor: float = 1.0, mask_factor: float = 1.0,
                   margin: Optional[Sequence[int]] = None, return_parts: bool = False):
    """The image losses of one refinement iteration on the ONE-pass render ([6,H,W] or [4,H,W]: channels 0-2 RGB, channel 3
    depth-as-colour):
    l1_dssim_loss(render6[:3], gt_rgb, dssim_factor, margin) + depth_mask_l1_loss(render6[3], gt_depth, max_depth,
    depth_factor, mask_factor) (refine.py:451-453, :584-594, :634-660).  Same two kernels as the separate functions; what
    it saves is autograd's handling of the two slices (two zero-filled [6,H,W] tensors, two slice copies and their sum):
    both kernels write into one gradient tensor.  parts = {l1+dssim loss, l1 mean, ssim mean, depth term, mask term,
    #fg, #bg}."""
    if gt_rgb.requires_grad or gt_depth.requires_grad:
        raise NotImplementedError("gaustar_amd.losses: no gradient w.r.t. the ground truth")
    loss, parts = _RGBDepthLoss.apply(render6, gt_rgb, gt_depth, float(dssim_factor),
                                      None if margin is None else tuple(margin), float(max_depth), float(depth_factor),
                                      float(mask_factor))
    return (loss, parts) if return_parts else loss


def _mesh_reg_refs(ref, n, dev, what):
    if ref is None:
        return None
    if ref.requires_grad:
        raise NotImplementedError(f"gaustar_amd.losses: no gradient w.r.t. {what}")
    r = ref.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
    if r.numel() != n:
        raise RuntimeError(f"{what} must hold {n} values, got {r.numel()}")
    return r


def _mesh_verts(verts, topo):
    """verts [V,3] on the topology's device, checked -> the detached contiguous float32 tensor the mesh-loss kernels read"""
    if not verts.is_cuda:
        raise RuntimeError("gaustar_amd.losses: verts must live on a HIP (cuda) device -- there is no CPU path")
    if verts.dim() != 2 or verts.size(1) != 3 or int(verts.size(0)) != topo.V:
        raise RuntimeError(f"verts must have dimensions ({topo.V}, 3), got {tuple(verts.shape)}")
    if topo.device != verts.device:
        raise RuntimeError("the mesh topology lives on another device than the vertices")
    v = verts.detach()
    if v.dtype != torch.float32 or not v.is_contiguous():
        v = v.float().contiguous()
    return v


def _check_vertex_grad(dL_dverts, v, topo):
    """The buffer a mesh loss's grad_into writes must match the saved vertices v -> their device"""
    dev = v.device
    if dL_dverts.dtype != torch.float32 or not dL_dverts.is_contiguous() or tuple(dL_dverts.shape) != tuple(v.shape) \
            or dL_dverts.device != dev:
        raise RuntimeError(f"dL_dverts must be a contiguous float32 ({topo.V}, 3) tensor on {dev}")
    return dev


class _SurfaceMeshLoss(torch.autograd.Function):
    """The three surface-mesh regularisers of refine.py:676-706 as ONE autograd node over the vertices.  Forward:
    gsr_mesh_reg_forward (an element pass + a fixed-order reduction) -> {nc, edge, area, total} on the device.  Backward:
    gsr_mesh_reg_backward, one vertex-major launch scaled by the incoming gradient on the device."""
    N_INPUTS, GRAD_AT = 7, (0,)

    @staticmethod
    def forward(ctx, verts, topo, nc_factor, ref_edge_len, edge_factor, ref_area, area_factor):
        lib = _lib.load()
        v, dev = _mesh_verts(verts, topo), verts.device
        re = _mesh_reg_refs(ref_edge_len, topo.E, dev, "ref_edge_len")
        ra = _mesh_reg_refs(ref_area, topo.F, dev, "ref_area")
        cfg = (float(nc_factor), float(edge_factor), float(area_factor))
        with _host.on_device(dev):
            ws, out = _scratch(lib.gsr_mesh_reg_workspace_bytes(topo.V, topo.F, topo.E, topo.Q), 4, dev)
            _lib.check(lib.gsr_mesh_reg_forward(
                topo.V, topo.F, topo.E, topo.Q, _vp(v), _vp(topo.faces), _vp(topo.edges), _vp(topo.pairs), _vp(re), _vp(ra), *cfg,
                _vp(ws), _vp(out), _stream()), "gsr_mesh_reg_forward")
        ctx.topo, ctx.cfg, ctx.in_dtype = topo, cfg, verts.dtype
        _finish(ctx, _SurfaceMeshLoss, out, (v, re, ra))
        return out[3], out

    @staticmethod
    def grad_into(ctx, g_loss, dL_dverts, accumulate):
        """gsr_mesh_reg_backward into dL_dverts [V,3] f32 (accumulate = 1: added to what is there, one rounding per element)."""
        lib = _lib.load()
        v, re, ra = ctx.saved_tensors
        topo = ctx.topo
        dev = _check_vertex_grad(dL_dverts, v, topo)
        with _host.on_device(dev):
            keep, sp = _scale_ptr(g_loss, dev)
            _lib.check(lib.gsr_mesh_reg_backward(
                topo.V, topo.F, topo.E, topo.Q, _vp(v), _vp(topo.faces), _vp(topo.edges), _vp(topo.pairs), _vp(topo.csr_offsets),
                _vp(topo.csr_entries), _vp(re), _vp(ra), *ctx.cfg, sp, _vp(dL_dverts), int(accumulate), _stream()),
                "gsr_mesh_reg_backward")
        return dL_dverts

    @staticmethod
    def backward(ctx, g_loss, _g_parts):
        return _backward_into_fresh(_SurfaceMeshLoss, ctx, g_loss)


def surface_mesh_loss(verts: torch.Tensor, topology, nc_factor: float, ref_edge_len: Optional[torch.Tensor] = None,
                      edge_factor: float = 0.0, ref_area: Optional[torch.Tensor] = None, area_factor: float = 0.0,
                      return_parts: bool = False):
    """nc_factor * mesh_normal_consistency(mesh) + edge_factor * ((edge_len - ref_edge_len)**2).mean()
    + area_factor * (face_area - ref_area).abs().mean()  (refine.py:685-706) on verts [V,3] with the faces of `topology`
    (gaustar_amd.meshes.MeshTopology; ref_edge_len in its edges_packed order).  A term whose factor is 0 or whose reference
    is None is left out.  One fused HIP op each way, no host synchronisation; parts = the device vector {nc, edge, area,
    total}."""
    loss, parts = _SurfaceMeshLoss.apply(verts, topology, float(nc_factor), ref_edge_len, float(edge_factor), ref_area,
                                         float(area_factor))
    return (loss, parts) if return_parts else loss


_LAP_METHODS = {"uniform": 0, "cot": 1, "cotcurv": 2}


class _MeshSmoothnessLoss(torch.autograd.Function):
    """The Laplacian-smoothing loss of refine.py:681-683 and the small-area regulariser of :713-718 as ONE autograd node over
    the vertices.  Forward: gsr_mesh_lap_forward -> {laplacian, area_reg, total} on the device, each already multiplied by
    its factor.  Backward: gsr_mesh_lap_backward, one vertex-major launch over the workspace the forward left, scaled by the
    incoming gradient on the device."""
    N_INPUTS, GRAD_AT = 5, (0,)

    @staticmethod
    def forward(ctx, verts, topo, laplacian_factor, method, area_reg_factor):
        v, dev = _mesh_verts(verts, topo), verts.device
        lib = _lib.load()
        cfg = (_LAP_METHODS[method], float(laplacian_factor), float(area_reg_factor))
        lists = (*topo.vertex_neighbours, *topo.vertex_face_csr)
        with _host.on_device(dev):
            ws, out = _scratch(lib.gsr_mesh_lap_workspace_bytes(topo.V, topo.F), 3, dev)
            _lib.check(lib.gsr_mesh_lap_forward(
                topo.V, topo.F, _vp(v), _vp(topo.faces), *[_vp(t) for t in lists], *cfg, _vp(ws), _vp(out), _stream()),
                "gsr_mesh_lap_forward")
        ctx.topo, ctx.cfg, ctx.in_dtype = topo, cfg, verts.dtype
        _finish(ctx, _MeshSmoothnessLoss, out, (v, ws))
        return out[2], out

    @staticmethod
    def grad_into(ctx, g_loss, dL_dverts, accumulate):
        """gsr_mesh_lap_backward into dL_dverts [V,3] f32 (accumulate = 1: added to what is there, one rounding per element)."""
        lib = _lib.load()
        v, ws = ctx.saved_tensors
        topo = ctx.topo
        dev = _check_vertex_grad(dL_dverts, v, topo)
        lists = (*topo.vertex_neighbours, *topo.vertex_face_csr)
        with _host.on_device(dev):
            keep, sp = _scale_ptr(g_loss, dev)
            _lib.check(lib.gsr_mesh_lap_backward(
                topo.V, topo.F, _vp(v), _vp(topo.faces), *[_vp(t) for t in lists], *ctx.cfg, _vp(ws), sp, _vp(dL_dverts),
                int(accumulate), _stream()), "gsr_mesh_lap_backward")
        return dL_dverts

    @staticmethod
    def backward(ctx, g_loss, _g_parts):
        return _backward_into_fresh(_MeshSmoothnessLoss, ctx, g_loss)


def mesh_smoothness_loss(verts: torch.Tensor, topology, laplacian_factor: float = 1.0, method: str = "uniform",
                         area_reg_factor: float = 0.0, return_parts: bool = False):
    """laplacian_factor * mesh_laplacian_smoothing(mesh, method) + area_reg_factor * relu(mean_area / face_area - 2).mean()
    (refine.py:681-683, :713-718; mean_area a constant) on verts [V,3] with the faces of `topology`
    (gaustar_amd.meshes.MeshTopology).  method: "uniform", "cot" or "cotcurv", as pytorch3d names them; the rules are restated
    in include/gsr.h (parity with pytorch3d itself is not pinned).  The weights are constants.  A term whose factor is 0 is left
    out.  A face of area exactly 0 makes the area regulariser +inf and contributes no gradient.  One fused HIP op each way, no
    host synchronisation, bit-reproducible; parts = the device vector {laplacian, area_reg, total}, each times its factor."""
    if method not in _LAP_METHODS:
        raise ValueError("Method should be one of {uniform, cot, cotcurv}")
    loss, parts = _MeshSmoothnessLoss.apply(verts, topology, float(laplacian_factor), method, float(area_reg_factor))
    return (loss, parts) if return_parts else loss


def _flat_f32(t, dev, n_cols, what):
    """Detached contiguous float32 view (copy only if needed) of a parameter-like tensor holding n_cols floats per Gaussian."""
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"gaustar_amd.losses: {what} must live on a HIP (cuda) device -- there is no CPU path")
    x = t.detach()
    if x.dtype != torch.float32 or not x.is_contiguous() or x.device != dev:
        x = x.to(device=dev, dtype=torch.float32).contiguous()
    if x.numel() % n_cols:
        raise RuntimeError(f"{what} must hold {n_cols} values per Gaussian, got shape {tuple(t.shape)}")
    return x


def _weight_strides(weight, N, dev):
    """(tensor, row stride, column stride) in elements of a [N], [N,1] or [N,3] weight read in place (expanded views included)."""
    if weight is None:
        return None, 0, 0
    if weight.requires_grad:
        raise NotImplementedError("gaustar_amd.losses: no gradient w.r.t. weight")
    w = weight.detach()
    if w.dtype != torch.float32 or w.device != dev:
        w = w.to(device=dev, dtype=torch.float32)
    if w.dim() == 1 and w.size(0) == N:
        return w, int(w.stride(0)), 0
    if w.dim() == 2 and w.size(0) == N and w.size(1) in (1, 3):
        return w, int(w.stride(0)), int(w.stride(1)) if w.size(1) == 3 else 0
    raise RuntimeError(f"weight must have dimensions ({N},), ({N}, 1) or ({N}, 3), got {tuple(weight.shape)}")


class _GaussianParamLoss(torch.autograd.Function):
    """The regularisers on the Gaussians' own parameters (refine.py:739-740, :743-748, :663-669) as ONE autograd node.
    Forward: gsr_param_reg_forward -> {loose_t, loose_r, opacity, sh, total} on the device.  Backward: gsr_param_reg_backward,
    one elementwise launch scaled by the incoming gradient on the device."""
    N_INPUTS, GRAD_AT = 10, (0, 1, 5, 7)       # delta_t, delta_r, densities, sh_dc: the order of grad_into's buffers

    @staticmethod
    def forward(ctx, delta_t, delta_r, weight, factor_t, factor_r, densities, min_opacity, sh_dc, pre_sh_dc, sh_factor):
        lib = _lib.load()
        given = [t for t in (delta_t, delta_r, densities, sh_dc) if t is not None]
        if not given:
            raise RuntimeError("gaussian_param_loss: give at least one of delta_t, delta_r, densities, sh_dc")
        dev = given[0].device
        dt, dr = _flat_f32(delta_t, dev, 3, "delta_t"), _flat_f32(delta_r, dev, 4, "delta_r")
        dens, dc = _flat_f32(densities, dev, 1, "densities"), _flat_f32(sh_dc, dev, 3, "sh_dc")
        counts = {x.numel() // k for x, k in ((dt, 3), (dr, 4), (dens, 1), (dc, 3)) if x is not None}
        if len(counts) != 1:
            raise RuntimeError(f"delta_t, delta_r, densities and sh_dc disagree on the number of Gaussians: {sorted(counts)}")
        N = counts.pop()
        if pre_sh_dc is not None and pre_sh_dc.requires_grad:
            raise NotImplementedError("gaustar_amd.losses: no gradient w.r.t. pre_sh_dc")
        pre = _flat_f32(pre_sh_dc, dev, 3, "pre_sh_dc")
        M = pre.numel() // 3 if pre is not None else 0
        if M > N:
            raise RuntimeError(f"pre_sh_dc holds {M} rows, more than the {N} Gaussians")
        w, w_rs, w_cs = _weight_strides(weight, N, dev)
        cfg = (N, M, w_rs, w_cs, float(factor_t), float(factor_r), float(min_opacity), float(sh_factor))
        with _host.on_device(dev):
            ws, out = _scratch(lib.gsr_param_reg_workspace_bytes(N), 5, dev)
            _lib.check(lib.gsr_param_reg_forward(
                N, M, _vp(dt), _vp(dr), _vp(w), w_rs, w_cs, cfg[4], cfg[5], _vp(dens), cfg[6], _vp(dc), _vp(pre), cfg[7],
                _vp(ws), _vp(out), _stream()), "gsr_param_reg_forward")
        ctx.cfg = cfg
        ctx.have = tuple(x is not None for x in (dt, dr, w, dens, dc, pre))
        ctx.in_meta = tuple(None if t is None else (t.shape, t.dtype) for t in (delta_t, delta_r, densities, sh_dc))
        _finish(ctx, _GaussianParamLoss, out, [x for x in (dt, dr, w, dens, dc, pre) if x is not None])
        return out[4], out

    @staticmethod
    def grad_into(ctx, g_loss, buffers, accumulate):
        """gsr_param_reg_backward into buffers = (dL_ddelta_t, dL_ddelta_r, dL_ddensities, dL_dsh_dc): contiguous float32
        tensors with the inputs' element counts, any of them None (accumulate = 1: added to what is there, one rounding per
        element).  A term that was skipped in the forward leaves its buffer untouched."""
        lib = _lib.load()
        it = iter(ctx.saved_tensors)
        dt, dr, w, dens, dc, pre = (next(it) if h else None for h in ctx.have)
        N, M, w_rs, w_cs, factor_t, factor_r, min_opacity, sh_factor = ctx.cfg
        dev = next(x for x in (dt, dr, dens, dc) if x is not None).device
        for b, k, what in zip(buffers, (3, 4, 1, 3), ("dL_ddelta_t", "dL_ddelta_r", "dL_ddensities", "dL_dsh_dc")):
            if b is not None and (b.dtype != torch.float32 or not b.is_contiguous() or b.numel() != N * k or b.device != dev):
                raise RuntimeError(f"{what} must be a contiguous float32 tensor of {N * k} elements on {dev}")
        with _host.on_device(dev):
            keep, sp = _scale_ptr(g_loss, dev)
            _lib.check(lib.gsr_param_reg_backward(
                N, M, _vp(dt), _vp(dr), _vp(w), w_rs, w_cs, factor_t, factor_r, _vp(dens), min_opacity, _vp(dc), _vp(pre),
                sh_factor, sp, *[_vp(b) for b in buffers], int(accumulate), _stream()), "gsr_param_reg_backward")
        return buffers

    @staticmethod
    def backward(ctx, g_loss, _g_parts):
        if not ctx.saved_tensors or g_loss is None:
            return at_inputs(_GaussianParamLoss, ())
        it = iter(ctx.saved_tensors)
        dt, dr, _w, dens, dc, pre = (next(it) if h else None for h in ctx.have)
        _N, M, _rs, _cs, factor_t, factor_r, _mo, sh_factor = ctx.cfg
        need_dt, need_dr, need_dens, need_dc = (ctx.needs_input_grad[i] for i in _GaussianParamLoss.GRAD_AT)
        # (a term that is off leaves its buffer untouched: no buffer is made for it, its input's gradient is None)
        srcs = (dt if need_dt and factor_t != 0.0 else None, dr if need_dr and factor_r != 0.0 else None,
                dens if need_dens else None, dc if need_dc and pre is not None and M > 0 and sh_factor != 0.0 else None)
        bufs = tuple(None if s is None else torch.empty_like(s) for s in srcs)
        if any(b is not None for b in bufs):
            _GaussianParamLoss.grad_into(ctx, g_loss, bufs, 0)
        return at_inputs(_GaussianParamLoss, [None if b is None else b.view(m[0]).to(m[1]) for b, m in zip(bufs, ctx.in_meta)])


def gaussian_param_loss(delta_t: Optional[torch.Tensor] = None, delta_r: Optional[torch.Tensor] = None,
                        weight: Optional[torch.Tensor] = None, factor_t: float = 100.0, factor_r: float = 1.0,
                        densities: Optional[torch.Tensor] = None, min_opacity: float = 0.8,
                        sh_dc: Optional[torch.Tensor] = None, pre_sh_dc: Optional[torch.Tensor] = None, sh_factor: float = 1.0,
                        return_parts: bool = False):
    """factor_t * (weight * delta_t.abs()).mean() + factor_r * (weight * delta_r[..., 1:].abs()).mean()
    + relu(min_opacity - sigmoid(densities)).mean() + sh_factor * ((pre_sh_dc - sh_dc[:M]) ** 2).mean()
    (refine.py:739-740, :743-748, :663-669; defaults of refine.py:29-33) on the model's `_delta_t` [N,3], `_delta_r` [N,4],
    `all_densities` [N,1] and `_sh_coordinates_dc` [N,1,3]; pre_sh_dc [M,3] or [M,1,3] is the tracked prefix (M <= N).  weight:
    [N], [N,1] or [N,3], read in place whatever its strides (refine.py:737's expanded view included); None = 1.  A term whose
    tensor is None or whose factor is 0 is left out.  One fused HIP op each way, no host synchronisation, bit-reproducible;
    parts = the device vector {loose_t, loose_r, opacity, sh, total}."""
    loss, parts = _GaussianParamLoss.apply(delta_t, delta_r, weight, float(factor_t), float(factor_r), densities,
                                           float(min_opacity), sh_dc, pre_sh_dc, float(sh_factor))
    return (loss, parts) if return_parts else loss
