"""Rig-wide topology-error detection (gaustar_trainers/refined_mesh.py:697-920, `detect_topo_err`) on the GPU.

At iteration `loose_bind_from` the refinement loop (refine.py:720-734) asks where the refined mesh disagrees with the rig's GT
depth and, if at least 100 Gaussians sit on fully wrong faces, turns on loose binding.  The reference needs open3d, pytorch3d,
trimesh and cv2 for it.  Here the depth term -- the only one refine.py switches on -- runs as HIP kernels (include/gsr.h,
gsr_topo.hip) behind two calls:

    res = detect_topology_errors(model, cameras, gt_depth)       # native: face_loss [F], unbind_weight [N,3], topo_change_num
    face_loss = detect_topo_err(sugar, nerfmodel, work_dir, cmr, ite, use_depth_loss=True, depth_scalar=3,
                                use_color_loss=False, use_densifier_grad=False, mesh_prop=20)      # the reference's signature

Per camera: the depth render and the solid-surface depth render (bg = max_depth, colour = view-space z) go through the
rasterizer directly under no_grad, then three launches reduce the GT edge statistic and write the camera's row of a [C, V]
table (loss, or -1 where the vertex is not visible).  Cameras are sharded over ranks (sweep.camera_shard) and rendered
`views_in_flight` at a time (pipelines.ViewPipelines); the rows come back with one all_gather (sweep.gather_rows).  Over the
rig every rank runs the same deterministic passes on the same table: mean per vertex, floor, propagation sweeps, voxel grid,
kNN interpolation, face quantisation.  The one host synchronisation is the read of topo_change_num at the end.

Not implemented (ValueError in the adapter): the colour and densifier-gradient terms, save_inter / save_render images.
`save_mesh` is accepted and ignored: there is no OBJ writer.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Callable, Optional, Sequence, Union

import numpy as np
import torch

from . import _host, _lib, _rig, knn, sweep
from ._lib import ptr as _p

MAX_DEPTH = 10.0   # refined_mesh.py:24


def rig_from_cameras(cameras: Sequence) -> dict:
    """The reference's `cmr` dict (rgb_cameras.npz; the layout: _rig.py) for NerfCameras, float64 numpy and int64 shape; the
    reference's projection ignores the principal point in the intrinsics.  The extrinsic is the inverse of
    NerfCamera.rasterizer_camera()'s axis flip: the world-to-camera matrix its view matrix holds, in double."""
    C = len(cameras)
    intr = np.zeros((C, 3, 3))
    extr = np.zeros((C, 4, 4))
    shape = np.zeros((C, 2), dtype=np.int64)
    for i, cam in enumerate(cameras):
        c2w = np.eye(4)
        c2w[:np.asarray(cam.c2w).shape[0], :] = np.asarray(cam.c2w, dtype=np.float64)
        c2w[:3, 1:3] *= -1
        extr[i] = np.linalg.inv(c2w)
        px, py = (float(v) for v in cam.principal_ndc)
        intr[i] = [[cam.fx, 0.0, cam.width * 0.5 - px * cam.width * 0.5], [0.0, cam.fy, cam.height * 0.5 - py * cam.height * 0.5],
                   [0.0, 0.0, 1.0]]
        shape[i] = (cam.height, cam.width)
    return {"intrinsics": intr, "extrinsics": extr, "shape": shape}


@dataclass
class TopologyErrors:
    """face_loss [F] f32 in [0, 1] (the reference's return value); face_colour [F] uint8 (face_loss * 255);
    unbind_weight [N,3] f32 = 1 - face_loss repeated over the face's Gaussians (face-major) and the three axes
    (refine.py:729, :736); topo_change_num = Gaussians with unbind weight 0 (refine.py:730 -- it counts Gaussians, not
    faces); decision = topo_change_num >= 100, i.e. loose binding starts (:731-736).
    With return_stages: count [V] int32, value [V] f64 after the mean / floor, propagated [V] f64, interpolated [V] f64,
    n_voxels, and table [C,V] f32 (the per-camera rows, -1 = not visible)."""
    face_loss: torch.Tensor
    face_colour: torch.Tensor
    unbind_weight: torch.Tensor
    topo_change_num: int
    decision: bool
    count: Optional[torch.Tensor] = None
    value: Optional[torch.Tensor] = None
    propagated: Optional[torch.Tensor] = None
    interpolated: Optional[torch.Tensor] = None
    n_voxels: Optional[int] = None
    table: Optional[torch.Tensor] = None


def vertex_neighbours(topo) -> tuple:
    """meshes.MeshTopology.vertex_neighbours: (offsets [V+1], neighbours) int32, built once per MeshTopology."""
    return topo.vertex_neighbours


def unbind_weights(face_loss: torch.Tensor, face_colour: torch.Tensor, G: int) -> tuple:
    """refine.py:729-730: unbind_weight [F G, 3] = 1 - face_loss repeated over each face's G Gaussians (face-major, numpy's
    `repeat`) and the three axes; topo_change_num (a device scalar) = the Gaussians whose weight is 0, i.e. G per face of
    colour 255 -- Gaussians, not faces, despite the reference's name."""
    unbind = (1.0 - face_loss).repeat_interleave(G)[:, None].expand(-1, 3)
    return unbind, (face_colour == 255).sum() * G


class DepthRenders:
    """The two renders of refined_mesh.py:762-772 for one model state: colour = each Gaussian's view-space z, bg = max_depth in
    all three channels, with the model's scales and with the solid-surface scales (sugar_model.py:1230-1232, computed once
    here).  Called per camera -> (render_depth [H,W], surface_depth [H,W]), channel 0 of the rasterizer's image: the very
    call render_image_gaussian_rasterizer(camera, bg_color=[max_depth] * 3, point_colors=view_depth_colors(camera)
    [, use_solid_surface=True]) makes, without autograd."""

    def __init__(self, model, max_depth: float = MAX_DEPTH):
        self.model = model
        with torch.no_grad():
            self.pts, self.ops, self.quats = model.points.detach(), model.strengths.detach().view(-1, 1), model.quaternions.detach()
            self.scales = model.scaling.detach()
            self.solid = model._scales_for_render(True, False).detach()
            self.zeros2d = torch.zeros_like(self.pts)
        self.bg = torch.full((3,), float(max_depth), dtype=torch.float32, device=model.device)

    @torch.no_grad()
    def __call__(self, camera):
        from . import GaussianRasterizer
        settings, view, _campos = self.model._settings(camera, self.bg, self.model.sh_levels - 1)
        z = (self.pts @ view[:3, 2:3] + view[3, 2]).expand(-1, 3)      # SurfaceGaussians.view_depth_colors
        raster = GaussianRasterizer(settings)
        kw = dict(means3D=self.pts, means2D=self.zeros2d, shs=None, colors_precomp=z, opacities=self.ops, rotations=self.quats,
                  cov3D_precomp=None)
        render = raster(scales=self.scales, **kw)[0][0].contiguous()
        surface = raster(scales=self.solid, **kw)[0][0].contiguous()
        return render, surface


@torch.no_grad()
def detect_topology_errors(model, cameras: Sequence, gt_depth: Union[torch.Tensor, Callable[[int], torch.Tensor]], rig: Optional[dict] = None,
                           depth_scalar: float = 3.0, min_observe: int = 4, mesh_prop: int = 20, detect_floor: bool = True,
                           voxel_size: float = 0.01, max_depth: float = MAX_DEPTH, views_in_flight: int = 2,
                           rank: Optional[int] = None, world: Optional[int] = None, return_stages: bool = False) -> TopologyErrors:
    """detect_topo_err's depth term for a harness.SurfaceGaussians `model` seen by `cameras` (NerfCameras).  gt_depth: [C,H,W]
    or a callable i -> [H,W] (any device; read once per camera of this rank's shard).  rig: the `cmr` dict the projection
    uses (default rig_from_cameras(cameras)).  Defaults are refine.py:724-727's call.  mesh_prop: propagation sweeps (0 =
    none, as the reference's `if mesh_prop:`)."""
    lib = _lib.load()
    dev = model.device
    if dev.type != "cuda":
        raise RuntimeError("detect_topology_errors needs the model on a GPU")
    rig = _rig.Rig.of(rig_from_cameras(cameras) if rig is None else rig)
    C = len(cameras)
    verts = model._points.detach().float().contiguous()
    V = int(verts.shape[0])
    topo = model.mesh_topology()
    F, G = topo.F, model.n_gaussians_per_surface_triangle

    # ---- per camera: two depth renders and one row of the table
    renders = DepthRenders(model, max_depth)
    mine = sweep.camera_shard(C, rank, world)
    for i in mine:
        cameras[i].on_device(dev)        # matrices uploaded before the workers start (the per-camera cache is not locked)
    local = torch.empty(len(mine), V, dtype=torch.float32, device=dev)
    ws_bytes = int(lib.gsr_topo_view_workspace_bytes(1, 1))

    def gt_of(i):
        g = gt_depth(i) if callable(gt_depth) else gt_depth[i]
        g = g[..., 0] if g.dim() == 3 else g
        return g.to(device=dev, dtype=torch.float32).contiguous()

    def per_camera(j, i):
        render, surface = renders(cameras[i])
        g = gt_of(i)
        H, W = rig.hw(i)
        if tuple(g.shape) != (H, W) or tuple(render.shape) != (H, W):
            raise ValueError(f"camera {i}: GT depth {tuple(g.shape)} / render {tuple(render.shape)} vs rig shape {(H, W)}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_topo_view(H, W, V, _p(verts), _p(g), _p(render), _p(surface), float(max_depth),
                                     rig.cam14(i), _p(ws), _p(local[j]), _host.stream_of(verts)),
                   "gsr_topo_view")

    with _host.on_device(verts.device):
        sweep.run_cameras(mine, per_camera, views_in_flight, dev)
        table = sweep.gather_rows(local, C, rank, world)

        # ---- over the rig (every rank, same table, same bits)
        stream = _host.stream_of(verts)
        value = torch.empty(V, dtype=torch.float64, device=dev)
        count = torch.empty(V, dtype=torch.int32, device=dev)
        valid = torch.empty(V, dtype=torch.uint8, device=dev)
        ymin = verts[:, 1].min().reshape(1) if V else None
        _lib.check(lib.gsr_topo_aggregate(C, V, _p(table.contiguous()), _p(verts), _p(ymin), float(depth_scalar), int(min_observe),
                                          int(bool(detect_floor)), _p(value), _p(count), _p(valid), stream), "gsr_topo_aggregate")
        off, nbr = topo.vertex_neighbours
        sweeps = int(mesh_prop) if mesh_prop else 0
        prop = torch.empty_like(value)
        tmp = torch.empty_like(value)
        va, vb = torch.empty_like(valid), torch.empty_like(valid)
        _lib.check(lib.gsr_topo_propagate(V, _p(off), _p(nbr), sweeps, _p(value), _p(valid), _p(prop), _p(tmp), _p(va), _p(vb), stream),
                   "gsr_topo_propagate")

        vmin, skeys, order, vid, _head, flags = knn.voxel_groups(lib, verts, voxel_size, stream)
        vox_ws = torch.empty(int(lib.gsr_topo_voxel_workspace_bytes(V)) // 4 + 4, dtype=torch.float32, device=dev)
        vox_value = torch.empty(V, dtype=torch.float64, device=dev)
        interp = torch.empty(V, dtype=torch.float64, device=dev)
        _lib.check(lib.gsr_topo_voxel_interp(V, _p(verts), _p(vmin), float(voxel_size), _p(skeys), _p(order.contiguous()), _p(vid),
                                             _p(prop), _p(vox_ws), _p(vox_value), _p(interp), stream), "gsr_topo_voxel_interp")
        face_colour = torch.empty(F, dtype=torch.uint8, device=dev)
        face_loss = torch.empty(F, dtype=torch.float32, device=dev)
        _lib.check(lib.gsr_topo_faces(F, _p(topo.faces), _p(interp), _p(face_colour), _p(face_loss), stream), "gsr_topo_faces")

    unbind, n_changed = unbind_weights(face_loss, face_colour, G)
    head = torch.stack([n_changed, flags[0].long(), vid[-1] + 1 if V else torch.zeros((), dtype=torch.long, device=dev)]).cpu()
    if int(head[1]):
        raise ValueError(f"the mesh spans more than 2^21 voxels of {voxel_size} along an axis")
    n = int(head[0])
    res = TopologyErrors(face_loss=face_loss, face_colour=face_colour, unbind_weight=unbind, topo_change_num=n, decision=n >= 100)
    if return_stages:
        res.count, res.value, res.propagated, res.interpolated = count, value, prop, interp
        res.n_voxels, res.table = int(head[2]), table
    return res


def detect_topo_err(refined_sugar, nerfmodel, work_dir, cmr, ite, use_depth_loss=True, depth_scalar=1, use_color_loss=True,
                    color_scalar=1, use_densifier_grad=False, grad_scalar=1, use_opacity_loss=False, save_inter=False,
                    save_render=False, save_mesh=True, mesh_prop=False, detect_floor=True, min_observe=4, voxel_size=0.01,
                    views_in_flight: int = 2) -> np.ndarray:
    """refined_mesh.py:697-920 with the reference's signature and defaults; returns face_loss [F] float64 numpy.
    `refined_sugar` is a harness.SurfaceGaussians; `nerfmodel` needs `get_gt_depth(camera_indices=i)` ([H,W,1] or [H,W])
    and its camera list as `cameras` (harness.NerfCamera, in the order of `cmr`).  `work_dir` and `ite` only name the
    reference's output folders and are unused.  save_mesh is accepted and ignored (no OBJ export).  Raises ValueError for
    what is not implemented: use_color_loss, use_densifier_grad, use_opacity_loss, save_inter, save_render -- and for
    use_depth_loss=False, which leaves nothing to detect."""
    for name, on in (("use_color_loss", use_color_loss), ("use_densifier_grad", use_densifier_grad),
                     ("use_opacity_loss", use_opacity_loss), ("save_inter", save_inter), ("save_render", save_render)):
        if on:
            raise ValueError(f"detect_topo_err: {name}=True is not implemented (depth term only)")
    if not use_depth_loss:
        raise ValueError("detect_topo_err: use_depth_loss=False is not implemented")
    res = detect_topology_errors(refined_sugar, nerfmodel.cameras, lambda i: nerfmodel.get_gt_depth(camera_indices=i), rig=cmr,
                                 depth_scalar=float(depth_scalar), min_observe=int(min_observe), mesh_prop=int(mesh_prop or 0),
                                 detect_floor=bool(detect_floor), voxel_size=float(voxel_size), views_in_flight=views_in_flight)
    return res.face_colour.cpu().numpy().astype(np.float64) / 255


__all__ = ["rig_from_cameras", "detect_topology_errors", "detect_topo_err", "TopologyErrors", "DepthRenders", "vertex_neighbours",
           "unbind_weights"]
