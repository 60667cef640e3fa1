"""Host-side counterpart of the reference's render harness:
`SuGaR.render_image_gaussian_rasterizer` and the properties it reads (gaustar_scene/sugar_model.py:1065-1311, :417-508,
:442-450, :674-718), assembled from this package's fused ops.  The reference module itself cannot be imported here
(open3d / pytorch3d), so this mirrors its interface -- same parameter names in the state dict, same argument names
and return conventions of the render call -- for the mesh-bound ("binded_to_surface_mesh") case GauSTAR uses.

    model = SurfaceGaussians.from_checkpoint(formats.load_sugar_checkpoint("2000.pt"), device)
    image = model.render_image_gaussian_rasterizer(camera=cam, bg_color=[0, 1, 0], sh_deg=3)          # [H,W,3]
    rgb, depth = model.render_rgb_depth(camera=cam, bg_color=[0, 1, 0], max_depth=10.0, sh_deg=3)     # one pass

What differs from the reference, by design: per-camera matrices are built once and cached on the device (the reference
redoes a numpy inverse and three uploads per call, :1129-1163); points / scaling / quaternions come from one fused kernel
(and one backward) per parameter version instead of ~50 elementwise kernels per property access.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from typing import Dict, Optional, Sequence

import numpy as np
import torch
from torch import nn

from . import producers, refine_step as _refine_step, scene
from .rasterizer import GaussianRasterizationSettings, GaussianRasterizer
from .refine_step import RenderJob, RenderParams, _PlainCtx, _RenderMeshBound  # noqa: F401 (the last two: their old home)

BARY_COORDS = {  # sugar_model.py:186-226
    1: [[1 / 3, 1 / 3, 1 / 3]],
    3: [[1 / 2, 1 / 4, 1 / 4], [1 / 4, 1 / 2, 1 / 4], [1 / 4, 1 / 4, 1 / 2]],
    4: [[1 / 3, 1 / 3, 1 / 3], [2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]],
    6: [[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12], [5 / 12, 1 / 6, 5 / 12],
        [5 / 12, 5 / 12, 1 / 6]],
}


@dataclass
class NerfCamera:
    """One camera as CamerasWrapper holds it: `c2w` is the [3,4] (or [4,4]) NeRF 'transform_matrix' -- camera-to-world
    with OpenGL/Blender axes (Y up, Z back) --, pinhole intrinsics in pixels."""
    c2w: np.ndarray
    fx: float
    fy: float
    width: int
    height: int
    znear: float = 1e-4
    zfar: float = 100.0
    principal_ndc: Sequence[float] = (0.0, 0.0)   # p3d K[0,0,2], K[0,1,2]; 0 when cx = W/2, cy = H/2 (cameras.py:276-277)
    # camera centre handed to the rasterizer instead of c2w[:3, 3] (with_extrinsic: the reference's -T R^-1 differs from it
    # for a non-rigid extrinsic); a declared field, so dataclasses.replace / copy / pickle keep it
    center_override: Optional[np.ndarray] = None
    _cache: Dict = field(default_factory=dict, repr=False, compare=False)

    def rasterizer_camera(self) -> scene.Camera:
        """sugar_model.py:1129-1163: flip to COLMAP axes, invert, R stored transposed, world_view = getWorld2View(R, T)^T,
        proj = getProjectionMatrix(...)^T with the principal-point entries, full = world_view @ proj."""
        c2w = np.eye(4)
        c2w[:np.asarray(self.c2w).shape[0], :] = np.asarray(self.c2w, dtype=np.float64)
        c2w[:3, 1:3] *= -1                                    # :1134
        w2c = np.linalg.inv(c2w)                              # :1138
        R, T = np.transpose(w2c[:3, :3]), w2c[:3, 3]          # :1139-1140
        fovx, fovy = scene.focal2fov(self.fx, self.width), scene.focal2fov(self.fy, self.height)
        view_t = scene.get_world2view(R, T).transpose()       # :1149-1150
        proj_t = scene.get_projection_matrix(self.znear, self.zfar, fovx, fovy).transpose().copy()
        proj_t[2, 0] = -float(self.principal_ndc[0])          # :1159-1160
        proj_t[2, 1] = -float(self.principal_ndc[1])
        full_t = (view_t @ proj_t).astype(np.float32)
        campos = np.asarray(self.c2w, dtype=np.float64)[:3, 3]    # p3d get_camera_center() = camera position
        if self.center_override is not None:                  # (with_extrinsic: the reference's own formula)
            campos = np.asarray(self.center_override, dtype=np.float64)
        return scene.Camera(W=int(self.width), H=int(self.height), tanfovx=math.tan(fovx * 0.5), tanfovy=math.tan(fovy * 0.5),
                            viewmatrix=np.ascontiguousarray(view_t, dtype=np.float32), projmatrix=np.ascontiguousarray(full_t),
                            campos=campos.astype(np.float32))

    def with_extrinsic(self, extr) -> "NerfCamera":
        """The camera `overwrite_extr` turns this one into (sugar_model.py:1119-1127 and :1141-1147): `extr` is a [4,4]
        WORLD-TO-CAMERA matrix in COLMAP axes (X right, Y down, Z forward).  The reference stores R = inverse(extr[:3,:3])
        and T = extr[:3,3] in its pytorch3d camera with the first two axes negated, negates them back, and hands
        getWorld2View(R, T) = [R^T | T] to the rasterizer; its camera centre is pytorch3d's -T R^-1 of the stored pair, i.e.
        -extr[:3,:3]^T ... for a rotation, the camera position.  Intrinsics, image size and clip planes are kept."""
        E = np.asarray(extr.detach().cpu().numpy() if isinstance(extr, torch.Tensor) else extr, dtype=np.float64).reshape(4, 4)
        key = ("extr", E.tobytes())                          # (the derived camera and its device tensors are built once per pose)
        hit = self._cache.get(key)
        if hit is not None:
            return hit
        R = np.linalg.inv(E[:3, :3])                          # :1121 (p3d_camera.R, the two sign flips of :1122 / :1143 cancel)
        T = E[:3, 3].copy()                                   # :1123
        w2c = np.eye(4)
        w2c[:3, :3] = R.transpose()                           # getWorld2View: Rt[:3,:3] = R^T, Rt[:3,3] = t
        w2c[:3, 3] = T
        c2w = np.linalg.inv(w2c)
        c2w[:3, 1:3] *= -1                                    # back to the NeRF axes rasterizer_camera() starts from
        # pytorch3d's get_camera_center() of the stored (R, T) pair: C = -T_p3d R_p3d^-1 with R_p3d = R D, T_p3d = T D
        # (D = diag(-1, -1, 1)) = -T R^-1 -- equal to c2w[:3, 3] for a rigid `extr`, and what the reference uses otherwise
        cam = NerfCamera(c2w=c2w[:3, :], fx=self.fx, fy=self.fy, width=self.width, height=self.height, znear=self.znear,
                         zfar=self.zfar, principal_ndc=self.principal_ndc,
                         center_override=(-(T @ np.linalg.inv(R))).astype(np.float32))
        if len(self._cache) > 64:                             # (a pose optimised per iteration must not grow the cache for ever)
            for k_ in [k_ for k_ in self._cache if isinstance(k_, tuple) and k_[0] == "extr"]:
                del self._cache[k_]
        self._cache[key] = cam
        return cam

    def on_device(self, device):
        """(Camera, viewmatrix, full_proj, campos) with the three tensors resident on `device`, built once."""
        key = str(device)
        if key not in self._cache:
            cam = self.rasterizer_camera()
            t = lambda x: torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32)).to(device)
            self._cache[key] = (cam, t(cam.viewmatrix), t(cam.projmatrix), t(cam.campos))
        return self._cache[key]


def nerf_camera_from_scene(cam: scene.Camera, znear: float = 1e-4, zfar: float = 100.0) -> NerfCamera:
    """The NeRF-convention camera that produces `cam` (tests: scene.look_at_camera builds COLMAP-axes cameras)."""
    w2c = np.asarray(cam.viewmatrix, dtype=np.float64).T
    c2w = np.linalg.inv(w2c)
    c2w[:3, 1:3] *= -1
    fx = cam.W / (2.0 * cam.tanfovx)
    fy = cam.H / (2.0 * cam.tanfovy)
    return NerfCamera(c2w=c2w[:3, :], fx=fx, fy=fy, width=cam.W, height=cam.H, znear=znear, zfar=zfar)


@dataclass
class PostprocessResult:
    """SurfaceGaussians.postprocess_mesh: the new model, face_mask [F] bool over the old model's faces (True: kept),
    kept_per_iteration: the faces left after every peel, restored: the peeled faces the density brought back."""
    model: "SurfaceGaussians"
    face_mask: torch.Tensor
    kept_per_iteration: list
    restored: int


class SurfaceGaussians(nn.Module):
    """Gaussians bound to a triangle mesh: SuGaR with binded_to_surface_mesh = True (sugar_model.py:160-403), parameters
    under the reference's names so that a reference state dict loads with load_state_dict."""

    def __init__(self, verts: torch.Tensor, faces: torch.Tensor, n_gaussians_per_surface_triangle: int = 6,
                 sh_levels: int = 4, surface_mesh_thickness: float = 1e-6, min_gaussian_scale: Optional[float] = None,
                 max_gaussian_scale: Optional[float] = None, loose_bind: bool = False):
        super().__init__()
        G = int(n_gaussians_per_surface_triangle)
        if G not in BARY_COORDS:
            raise ValueError("n_gaussians_per_surface_triangle must be 1, 3, 4 or 6")
        F = int(faces.shape[0])
        N = F * G
        dev = verts.device
        self.n_gaussians_per_surface_triangle = G
        self.sh_levels = int(sh_levels)
        self.min_gaussian_scale, self.max_gaussian_scale = min_gaussian_scale, max_gaussian_scale
        self.return_one_densities = False
        self._points = nn.Parameter(verts.detach().clone().float())
        self.register_buffer("_surface_mesh_faces", faces.detach().long().contiguous().clone())   # (clone() keeps strides: the kernels read it as a dense [F, 3] int64 array)
        self.register_buffer("surface_triangle_bary_coords", torch.tensor(BARY_COORDS[G], dtype=torch.float32, device=dev)[..., None])
        self.register_buffer("surface_mesh_thickness", torch.tensor(float(surface_mesh_thickness), device=dev))
        # initial in-plane scale: the inscribed-circle radius of the face (sugar_model.py:216, :357)
        fv = self._points.detach()[self._surface_mesh_faces]
        edge = torch.stack([(fv[:, 0] - fv[:, 1]).norm(dim=-1), (fv[:, 1] - fv[:, 2]).norm(dim=-1), (fv[:, 2] - fv[:, 0]).norm(dim=-1)], -1)
        radius = {1: 1 / (2 * math.sqrt(3)), 3: 1 / (2 * (math.sqrt(3) + 1)), 4: 1 / (4 * math.sqrt(3)), 6: 1 / (4 + 2 * math.sqrt(3))}[G]
        init = (edge.min(dim=-1).values * radius).clamp(min=1e-8).log()
        self._scales = nn.Parameter(init[:, None, None].expand(F, G, 2).reshape(N, 2).contiguous())
        self._quaternions = nn.Parameter(torch.tensor([1.0, 0.0], device=dev).repeat(N, 1))          # 2-D rotation, identity
        self.all_densities = nn.Parameter(torch.full((N, 1), 2.2, device=dev))                      # sigmoid ~ 0.9
        self._sh_coordinates_dc = nn.Parameter(torch.zeros(N, 1, 3, device=dev))
        self._sh_coordinates_rest = nn.Parameter(torch.zeros(N, self.sh_levels ** 2 - 1, 3, device=dev))
        self._loose_bind = bool(loose_bind)
        if loose_bind:
            self._delta_t = nn.Parameter(torch.zeros(N, 3, device=dev))
            self._delta_r = nn.Parameter(torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(N, 1))
        # refine.py:737's per-Gaussian weight of the loose-bind penalties; not saved, as in the reference
        self.register_buffer("unbind_loss_weight", None, persistent=False)
        self._geom_cache = None
        # optional: an object with grad_views() / written(params) (gaustar_amd.dist.ShardedAdam) that receives the parameter
        # gradients of render_channels' backward in place -- see refine_step.GradHandoff (checked when a render is made)
        self.grad_sink = None

    def __getstate__(self):
        """copy.deepcopy / pickle of the model: the gradient sink (an optimiser with process-group handles and hooks on THIS
        model's parameters) and the per-object caches stay behind."""
        d = self.__dict__.copy()
        for k in ("grad_sink", "_geom_cache", "_thickness_cache", "_bary_rows_cache"):
            if k in d:
                d[k] = None
        return d

    # -------------------------------------------------------------------------------- construction from a checkpoint
    @classmethod
    def from_checkpoint(cls, ckpt: Dict, device, **kw) -> "SurfaceGaussians":
        """`ckpt` = formats.load_sugar_checkpoint(path)."""
        N, F = ckpt["raw_scales"].shape[0], ckpt["faces"].shape[0]
        m = cls(ckpt["verts"].to(device), ckpt["faces"].to(device), n_gaussians_per_surface_triangle=N // F,
                sh_levels=int(round(math.sqrt(ckpt["sh"].shape[1]))), loose_bind=ckpt.get("delta_r") is not None,
                surface_mesh_thickness=ckpt["thickness"] if ckpt.get("thickness") is not None else 1e-6, **kw)
        with torch.no_grad():
            m._scales.copy_(ckpt["raw_scales"]); m._quaternions.copy_(ckpt["raw_complex"])
            m.all_densities.copy_(ckpt["densities"].view(-1, 1))
            m._sh_coordinates_dc.copy_(ckpt["sh"][:, :1]); m._sh_coordinates_rest.copy_(ckpt["sh"][:, 1:])
            if m._loose_bind:
                m._delta_t.copy_(ckpt["delta_t"]); m._delta_r.copy_(ckpt["delta_r"])
        return m

    # -------------------------------------------------------------------------------- loose binding on a live model
    def is_loose_bind(self) -> bool:      # sugar_model.py:602-603
        return self._loose_bind

    def loose_bind(self, unbind_weight: Optional[torch.Tensor] = None):
        """sugar_model.py:596-597 on a live model: from now on `_delta_t` / `_delta_r` move the Gaussians off their faces.
        A model built without them gets `_delta_t` = 0 and `_delta_r` = identity here, as nn.Parameters under the
        reference's names; they are returned so that an optimiser can take them in (loose_bind_param_groups) -- an empty
        list if they existed.  unbind_weight ([N], [N,1] or [N,3]; refine.py:737) becomes `unbind_loss_weight`, kept as it
        is laid out (an expanded view stays one)."""
        new = []
        if getattr(self, "_delta_t", None) is None:
            N, dev = self.n_points, self.device
            self._delta_t = nn.Parameter(torch.zeros(N, 3, device=dev))
            self._delta_r = nn.Parameter(torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev).repeat(N, 1))
            new = [self._delta_t, self._delta_r]
        self._loose_bind = True
        self._geom_cache = None
        if unbind_weight is not None:
            w = torch.as_tensor(unbind_weight).detach().to(device=self.device, dtype=torch.float32)
            if w.dim() not in (1, 2) or w.size(0) != self.n_points or (w.dim() == 2 and w.size(1) not in (1, 3)):
                raise ValueError(f"unbind_weight must have dimensions (N,), (N, 1) or (N, 3) with N = {self.n_points}, "
                                 f"got {tuple(w.shape)}")
            self.unbind_loss_weight = w
        return new

    def rebind(self) -> None:
        """sugar_model.py:599-600: the deltas stay (parameters and values) and are ignored again."""
        self._loose_bind = False
        self._geom_cache = None

    def loose_bind_param_groups(self, position_lr: float, rotation_lr: float):
        """The two groups of sugar_optimizer.py:86-87, for `optimizer.add_param_group` (torch.optim.Adam, optim.Adam,
        dist.ShardedAdam -- there between step() and the next backward, on every rank)."""
        if getattr(self, "_delta_t", None) is None:
            raise RuntimeError("loose_bind_param_groups: the model has no deltas yet -- call loose_bind() first")
        return [{"params": [self._delta_t], "lr": float(position_lr), "name": "delta_t"},
                {"params": [self._delta_r], "lr": float(rotation_lr), "name": "delta_r"}]

    def apply_topology_result(self, res, optimizer=None, min_changed: int = 100, position_lr: float = 0.0,
                              rotation_lr: float = 0.0) -> bool:
        """refine.py:729-737 on the result of detect_topology_errors: with fewer than `min_changed` Gaussians of weight 0
        nothing changes (-> False); otherwise the model is loose-bound with res.unbind_weight, the parameters this created
        join `optimizer` (if given) as loose_bind_param_groups(position_lr, rotation_lr), -> True."""
        n = getattr(res, "topo_change_num", None)
        if n is None:
            w = res.unbind_weight
            n = int(((w if w.dim() == 1 else w[:, 0]) == 0).sum())
        if int(n) < int(min_changed):
            return False
        new = self.loose_bind(res.unbind_weight)
        if optimizer is not None and new:
            for g in self.loose_bind_param_groups(position_lr, rotation_lr):
                optimizer.add_param_group(g)
        return True

    def face_delta(self) -> torch.Tensor:
        """sugar_model.py:605-611 `get_face_delta`: [F,1], the norm of each face's mean `_delta_t`."""
        if not self._loose_bind:
            raise RuntimeError("face_delta: the model is not loose-bound")
        self._fence(self._delta_t)
        d = self._delta_t.detach().reshape(-1, self.n_gaussians_per_surface_triangle, 3)
        return d.mean(dim=1).norm(dim=1, keepdim=True)

    def grad_ready_order(self):
        """The optimiser's parameters (sugar_optimizer.py:67-87) in the order their gradients become final in the backward
        of a render: the rasterizer's backward feeds the SH producer's backward first (`_sh_coordinates_*`, 70 % of the
        bytes) and `all_densities` (one sigmoid), then the mesh producer's backward (`_points`, `_scales`,
        `_quaternions`, `_delta_*`).  dist.GradAllReducer buckets in this order and starts a bucket's all-reduce as soon
        as its last gradient lands."""
        ps = [self._sh_coordinates_rest, self._sh_coordinates_dc, self.all_densities, self._scales, self._quaternions]
        if self._loose_bind:
            ps += [self._delta_t, self._delta_r]
        return ps + [self._points]

    def mesh_parameters(self):
        """The parameters the mesh producer reads -- the FIRST thing a render needs (dist.ShardedAdam(gather_first=...): their
        all-gather is waited for in step(), the SH coefficients' runs under the next render's mesh producer)."""
        ps = [self._points, self._scales, self._quaternions]
        if self._loose_bind:
            ps += [self._delta_t, self._delta_r]
        return ps

    def _fence(self, *params) -> None:
        """Readers of parameters outside the fused render: if the optimiser left their all-gather in flight
        (dist.ShardedAdam(gather_first=...)), order this stream behind it.  No sink, nothing pending: one attribute look-up."""
        fence = getattr(self.grad_sink, "wait_params", None)
        if fence is not None:
            fence(params if params else None)

    def state_dict(self, *a, **kw):
        """nn.Module.state_dict behind a fence on every lazily gathered parameter (a checkpoint must not read torn shards)."""
        self._fence()
        return super().state_dict(*a, **kw)

    # -------------------------------------------------------------------------------- the reference's properties
    @property
    def device(self):
        return self._points.device

    @property
    def n_points(self) -> int:
        return int(self._scales.shape[0])

    def _thickness(self) -> float:
        """surface_mesh_thickness as a Python float, read back from the device ONCE per value: `float(buffer)` is a
        device-to-host copy that waits for everything queued before it -- as a per-render call it drained the GPU once per
        iteration (the host could never run ahead of the previous iteration's optimiser step)."""
        t = self.surface_mesh_thickness
        c = getattr(self, "_thickness_cache", None)
        if c is None or c[0] is not t or c[1] != t._version:
            c = (t, t._version, float(t))
            self._thickness_cache = c
        return c[2]

    def _geometry(self):
        """(points, scaling, quaternions) from one fused call, shared by the three properties while no parameter
        changes (the reference recomputes each property from scratch on every access)."""
        params = [self._points, self._scales, self._quaternions] + ([self._delta_t, self._delta_r] if self._loose_bind else [])
        self._fence(*params)
        key = (tuple(p._version for p in params), torch.is_grad_enabled())
        if self._geom_cache is None or self._geom_cache[0] != key:
            out = producers.mesh_bound_gaussians(
                self._points, self._surface_mesh_faces, self.surface_triangle_bary_coords[..., 0], self._scales,
                self._quaternions, self._thickness(), self.min_gaussian_scale, self.max_gaussian_scale,
                self._delta_t if self._loose_bind else None, self._delta_r if self._loose_bind else None)
            self._geom_cache = (key, out)
        return self._geom_cache[1]

    @property
    def points(self):                 # sugar_model.py:417-435
        return self._geometry()[0]

    @property
    def scaling(self):                # :457-476
        return self._geometry()[1]

    @property
    def quaternions(self):            # :478-508
        return self._geometry()[2]

    @property
    def strengths(self):              # :442-447
        self._fence(self.all_densities)
        if self.return_one_densities:
            return torch.ones_like(self.all_densities.view(-1, 1))
        return torch.sigmoid(self.all_densities.view(-1, 1))

    @property
    def sh_coordinates(self):         # :449-450
        self._fence(self._sh_coordinates_dc, self._sh_coordinates_rest)
        return torch.cat([self._sh_coordinates_dc, self._sh_coordinates_rest], dim=1)

    def get_points_rgb(self, positions=None, camera_centers=None, directions=None, sh_levels=None, sh_coordinates=None):
        """sugar_model.py:674-718: colours for one camera centre (fused HIP producer) or, when `camera_centers` is None, for
        the given `directions`, taken as they are (torch operations, producers.points_rgb_from_directions)."""
        sh = self.sh_coordinates if sh_coordinates is None else sh_coordinates
        levels = self.sh_levels if sh_levels is None else int(sh_levels)
        if camera_centers is not None:                                        # :698-699 (takes precedence, as in the reference)
            positions = self.points if positions is None else positions
            return producers.points_rgb(positions, camera_centers, sh, levels)
        if directions is not None:                                            # :700-701
            return producers.points_rgb_from_directions(directions, sh, levels)
        raise ValueError("Either camera_centers or directions must be provided.")   # :703

    @property
    def surface_mesh(self):           # sugar_model.py:568-576 (without the vertex-colour texture)
        from . import meshes
        return meshes.Meshes(verts=[self._points], faces=[self._surface_mesh_faces])

    def mesh_topology(self):
        """meshes.MeshTopology of `_surface_mesh_faces` (built once per face tensor)."""
        from . import meshes
        return meshes.MeshTopology.of(self._surface_mesh_faces, int(self._points.shape[0]))

    def detect_topology_errors(self, cameras, gt_depth, **kw):
        """Where the mesh's topology disagrees with the GT depth of `cameras` (refined_mesh.py:697-920, depth term):
        topology.detect_topology_errors(self, cameras, gt_depth, **kw)."""
        from . import topology
        return topology.detect_topology_errors(self, cameras, gt_depth, **kw)

    def reset_neighbors(self, knn_to_track: Optional[int] = None, force: bool = False) -> None:
        """sugar_model.py:847-864: `knn_idx` [n_points, K] int64 and `knn_dists` [n_points, K] f32 of the current Gaussian
        centres among themselves (knn.knn_points; every row starts with the point itself, or a duplicate of it at a lower
        index, at distance 0).  K = knn_to_track, else the last one used, else 16.  The reference skips the call for a
        model bound to a mesh unless force is set, with a warning; every model here is bound, so the neighbours are always
        computed and `force` is accepted for the signature only."""
        from . import knn
        if knn_to_track is None:
            knn_to_track = getattr(self, "knn_to_track", 16)
        self.knn_to_track = int(knn_to_track)
        with torch.no_grad():
            pts = self.points.detach().float().contiguous()
            res = knn.knn_points(pts[None], pts[None], K=self.knn_to_track)
        self.knn_dists, self.knn_idx = res.dists[0], res.idx[0]

    def get_neighbors_of_random_points(self, num_samples: int) -> torch.Tensor:
        """sugar_model.py:804-809: the rows of `knn_idx` (reset_neighbors) of `num_samples` random points, all rows in
        order for a negative count."""
        if num_samples >= 0:
            return self.knn_idx[torch.randperm(self.n_points, device=self.device)[:num_samples]]
        return self.knn_idx

    # -------------------------------------------------------------------------------- the density field and the border clean-up
    def get_covariance(self, return_full_matrix=False, return_sqrt=False, inverse_scales=False):
        """sugar_model.py:619-639: density.get_covariance(self.scaling, self.quaternions, ...)."""
        from . import density
        return density.get_covariance(self.scaling, self.quaternions, return_full_matrix, return_sqrt, inverse_scales)

    def get_gaussians_closest_to_samples(self, x, n_closest_gaussian=None):
        """sugar_model.py:1007-1015: [Q,K] int64, the K nearest Gaussian centres of every row of x [Q,3] f32 (knn.knn_points, so
        a slot beyond the Gaussians there are holds 0, as pytorch3d pads).  K = n_closest_gaussian, else `knn_to_track`,
        which is set to 16 if the model has none (:1009-1011)."""
        from . import knn
        if n_closest_gaussian is None:
            if not hasattr(self, "knn_to_track"):
                self.knn_to_track = 16
            n_closest_gaussian = self.knn_to_track
        with torch.no_grad():
            return knn.knn_points(x[None], self.points.detach()[None], K=int(n_closest_gaussian)).idx[0]

    def compute_density(self, x, closest_gaussians_idx=None, density_factor=1., return_closest_gaussian_opacities=False):
        """sugar_model.py:1017-1040 on the model's own points / scaling / quaternions / strengths: density.compute_density,
        with the `knn_to_track` nearest Gaussians (16 if the model has none) when no indices are given."""
        from . import density
        if closest_gaussians_idx is None and not hasattr(self, "knn_to_track"):
            self.knn_to_track = 16
        with torch.no_grad():
            return density.compute_density(x, self.points, self.scaling, self.quaternions, self.strengths,
                                           closest_gaussians_idx=closest_gaussians_idx, K=getattr(self, "knn_to_track", 16),
                                           density_factor=density_factor,
                                           return_closest_gaussian_opacities=return_closest_gaussian_opacities)

    @torch.no_grad()
    def postprocess_mesh(self, iterations: int = 5, density_threshold: float = 0.1, K: Optional[int] = None) -> "PostprocessResult":
        """--postprocess_mesh (refined_mesh.py:1155-1217): `iterations` times the faces with an edge that fewer than two of the
        remaining faces share are peeled off (:1173-1177, by regions' masked edge counts), then a peeled face returns iff the
        density of ALL the model's Gaussians at its centre ((v0 + v1) + v2) / 3 is > density_threshold (:1180-1182; the K
        nearest, K = `knn_to_track` or 16), and a new model is built on the faces that are left: the same vertices,
        unreferenced ones included, the parameters gathered by face, not loose-bound (:1185-1216).  Every face starts inside:
        the reference's initial mask (:1169) has one entry per Gaussian and fits its per-face use only with one Gaussian per
        triangle.  -> PostprocessResult.  ValueError if no face is left.  One host read, at the end."""
        from . import _host, _meshargs, density, regions
        G = self.n_gaussians_per_surface_triangle
        self._fence()
        faces = _meshargs.faces_i32(self._surface_mesh_faces)
        F, dev = int(faces.shape[0]), faces.device
        verts = self._points.detach()
        err = torch.zeros(2, dtype=torch.int32, device=dev)       # [0]: the edge kernels' word, [1]: the density's
        mask = torch.ones(F, dtype=torch.bool, device=dev)
        kept = []
        with _host.on_device(dev):
            for _ in range(int(iterations)):
                if F == 0:
                    break
                counts = regions._edge_counts(faces, err[0:1], mask.view(torch.uint8))
                mask = mask & (counts >= 2).all(dim=1)
                kept.append(mask.sum())
        removed = ~mask
        fv = verts[self._surface_mesh_faces]
        centres = ((fv[:, 0] + fv[:, 1]) + fv[:, 2]) / 3
        if K is None:
            K = getattr(self, "knn_to_track", 16)
        pts = self.points.detach()
        records = density.pack_records(pts, self.scaling.detach(), self.quaternions.detach(), self.strengths.detach())
        # which faces were removed stays on the device: a face that stayed asks with a NaN centre, which the search answers
        # with an empty row without looking at a candidate, and whose density, 0, is not read
        centres = torch.where(removed[:, None], centres, torch.full_like(centres, float("nan"))).contiguous()
        idx = density.closest_gaussians(centres, pts.contiguous(), int(K))
        dens, _ = density.eval_records(centres, idx, records, 1.0, False, err[1:2])
        back = removed & (dens > float(density_threshold))
        mask = mask | back
        host = torch.stack([err[0].long(), err[1].long(), back.sum(), mask.sum(), *kept]).cpu().tolist()
        _meshargs.raise_if(host[0])
        _meshargs.raise_if(host[1], **density.ERR_TEXTS)
        if host[3] == 0:
            raise ValueError("postprocess_mesh: no face is left")
        sel = torch.argsort((~mask).to(torch.uint8), stable=True)[:host[3]]      # the kept faces in order, their number known: no read
        new = SurfaceGaussians(verts, self._surface_mesh_faces[sel], n_gaussians_per_surface_triangle=G, sh_levels=self.sh_levels,
                               surface_mesh_thickness=self._thickness(), min_gaussian_scale=self.min_gaussian_scale,
                               max_gaussian_scale=self.max_gaussian_scale, loose_bind=False)
        rows = (sel[:, None] * G + torch.arange(G, device=dev)).reshape(-1)
        for name in ("_scales", "_quaternions", "all_densities", "_sh_coordinates_dc", "_sh_coordinates_rest"):
            getattr(new, name).copy_(getattr(self, name).detach()[rows])
        new.return_one_densities = self.return_one_densities
        return PostprocessResult(model=new, face_mask=mask, kept_per_iteration=[int(k) for k in host[4:]], restored=int(host[2]))

    def to_gaussian_cloud(self):
        """convert_refined_sugar_into_gaussians (sugar_model.py:1416-1437) -> formats.GaussianCloud on the host: xyz = points,
        opacity = all_densities (logits), features_dc / features_rest = the SH parameters, scaling = log(scaling)
        (scale_inverse_activation), rotation = quaternions."""
        from . import formats
        with torch.no_grad():
            self._fence()
            n = lambda t: t.detach().float().cpu().numpy()
            return formats.GaussianCloud(xyz=n(self.points), features_dc=n(self._sh_coordinates_dc),
                                         features_rest=n(self._sh_coordinates_rest), opacity=n(self.all_densities.view(-1, 1)),
                                         scaling=n(torch.log(self.scaling)), rotation=n(self.quaternions))

    def export_ply(self, path: str) -> None:
        """--export_ply (train_seq.py's default): the 3DGS viewer's PLY of to_gaussian_cloud(), by formats.save_ply."""
        from . import formats
        formats.save_ply(path, self.to_gaussian_cloud())

    def warp_mesh(self, cameras, frames, **kw):
        """The surface mesh moved to the next frame along the optical flow of `cameras` (warp_mesh.py:216-401):
        warp.warp_mesh(vertices, faces, topology.rig_from_cameras(cameras), frames, **kw) (`rig` may be passed in kw)."""
        from . import topology, warp
        rig = kw.pop("rig", None) or topology.rig_from_cameras(cameras)
        return warp.warp_mesh(self._points.detach(), self._surface_mesh_faces, rig, frames, **kw)

    def render_mesh_depth(self, camera_or_index, cameras=None, **kw):
        """The surface mesh's own depth map, mask and (return_faces=True) visible face per pixel for one camera
        (render_depth_from_mesh.py:13-101 on the model's mesh): mesh_depth.mesh_depth_view(vertices, faces, ...) with the
        camera's row of topology.rig_from_cameras -> mesh_depth.MeshDepthView.  camera_or_index: a NerfCamera, or an index into
        `cameras`.  use_principal_point=True (in kw) reads the camera's principal point instead of (W / 2, H / 2)."""
        from . import _rig, mesh_depth, topology
        cam = cameras[int(camera_or_index)] if isinstance(camera_or_index, (int, np.integer)) else camera_or_index
        rig = _rig.Rig.of(topology.rig_from_cameras([cam]))
        if kw.pop("use_principal_point", False):
            kw["principal_point"] = rig.principal(0, True)
        return mesh_depth.mesh_depth_view(self._points.detach(), self._surface_mesh_faces, rig.extr[0], rig.intr[0], *rig.hw(0), **kw)

    def track(self, tracker):
        """Where a tracking.SurfaceTracker's points sit on the model's own mesh (tracking_util.py:70): tracker.positions(vertices,
        faces) -> [K,3] f64, the f32 vertices widened."""
        return tracker.positions(self._points.detach(), self._surface_mesh_faces)

    # -------------------------------------------------------------------------------- editing (gstar_edit.py): gaustar_amd.edit
    def cut(self, keep_faces):
        """edit.cut_model(self, keep_faces): a new model of the faces with keep_faces [F] bool set and their Gaussians."""
        from . import edit
        return edit.cut_model(self, keep_faces)

    def merged_with(self, other):
        """edit.merge_models(self, other): one model of both, other's faces behind this model's."""
        from . import edit
        return edit.merge_models(self, other)

    def transform(self, R, t, rotate_sh: bool = True):
        """edit.transform_model(self, R, t, rotate_sh): x -> R x + t in place, the SH coefficients turned with it."""
        from . import edit
        return edit.transform_model(self, R, t, rotate_sh)

    def paint_decal(self, anchors, uv, triangles, texture, **kw):
        """edit.paint_decal(self, anchors, uv, triangles, texture, **kw): a texture glued to tracked points, in place."""
        from . import edit
        return edit.paint_decal(self, anchors, uv, triangles, texture, **kw)

    def surface_distance(self, points):
        """The closest point of the model's own mesh for every point of points [K,3] f64: evaluate.surface_distance(points,
        vertices, faces) -> evaluate.SurfaceHit, the f32 vertices widened."""
        from . import evaluate
        return evaluate.surface_distance(points, self._points.detach(), self._surface_mesh_faces)

    def mesh_distance_to(self, verts, faces, **kw):
        """The model's own mesh, as the result, against a ground-truth mesh: evaluate.mesh_distance((vertices, faces), (verts,
        faces), **kw) -> evaluate.MeshDistance (Chamfer distance, precision, recall and F-score)."""
        from . import evaluate
        return evaluate.mesh_distance((self._points.detach(), self._surface_mesh_faces), (verts, faces), **kw)

    def extract_mesh_fusion(self, cameras, **kw):
        """The surface the renders of `cameras` (and of the 60 sampled cameras around them) agree on, by TSDF fusion and
        marching cubes (refined_mesh.py:311-459): fusion.fuse_mesh(self, cameras, **kw) -> fusion.FusionMesh.  smooth_iterations=K
        and simplify_face_num=N smooth and decimate it (refined_mesh.py:451-458, gaustar_amd.remesh)."""
        from . import fusion
        return fusion.fuse_mesh(self, cameras, **kw)

    def topology_update_regions(self, res, **kw):
        """The regions of the mesh that update_mesh_topo re-meshes (refined_mesh.py:516-571), from the face colours of
        detect_topology_errors' result `res`: regions.select_update_regions(vertices, faces, points, res.face_colour, G, **kw)
        -> regions.UpdateRegions.  Once per frame: it does not depend on aabb_pad."""
        from . import regions
        with torch.no_grad():
            return regions.select_update_regions(self._points.detach().float(), self._surface_mesh_faces, self.points.detach(),
                                                 res.face_colour, self.n_gaussians_per_surface_triangle, **kw)

    def cut_update_regions(self, update_regions, fusion_mesh, aabb_pad: float = 0.02):
        """Per merged box of update_regions.boxes(aabb_pad) a regions.RegionCut: the box, the patch of `fusion_mesh`
        (fusion.FusionMesh) with any vertex inside it, colours carried (refined_mesh.py:583), and the base mesh without the
        faces that have a vertex inside it, with its face_mask over the base mesh's faces (:609-614).  Each cut is made from
        the UNCUT base mesh: the reference cuts what the previous box's splice left (`base_mesh = connected_mesh`, :660);
        stitch_update_region joins one box's two cuts, and that chaining over boxes is the caller's."""
        from . import regions
        verts, faces = self._points.detach().float(), self._surface_mesh_faces.int()
        out = []
        for box in update_regions.boxes(aabb_pad):
            out.append(regions.RegionCut(box=box,
                                         fusion_patch=regions.cut_mesh_by_box(fusion_mesh.verts, fusion_mesh.faces, box, False,
                                                                              attrs=(fusion_mesh.colors,)),
                                         base_cut=regions.cut_mesh_by_box(verts, faces, box, True)))
        return out

    def stitch_update_region(self, cut, outlier_face_threshold=50, pad: float = 0.02):
        """One box of update_mesh_topo's loop (refined_mesh.py:583-658) without fill_holes: the fused patch of `cut`
        (regions.RegionCut) loses its outlier components (:590-599), its boundary vertices across the box (:600) and the base
        cut's boundary vertices inside the box grown by `pad` (:619) are found, and regions.connect_two_meshes joins the base
        cut (mesh 1) and the patch (mesh 2) along them (:628).  -> regions.RegionStitch: stitched (regions.StitchedMesh), patch
        (the patch that was stitched, colours in attrs[0]) and base_face_mask [F_base] bool over the UNCUT base mesh's faces:
        cut.base_cut.face_mask with the stitch's face_mask written into its True entries (:656-658).  None where the
        reference sets cc_success_flag = 0: an empty cut or no boundary vertices (:586, :601, :611, :620).

        Holes that fill_holes would have closed (:589, :617, :652) remain and can make `stitched.watertight` False.  What to do
        with a result that is not watertight (the reference skips the box, :639-643) is the caller's decision, and so is the
        chaining over several boxes (:660-664): every RegionCut of cut_update_regions was cut from the uncut base mesh.
        update_mesh_topology below is the whole loop, with the holes filled and the boxes chained."""
        from . import regions
        patch, base = cut.fusion_patch, cut.base_cut
        if patch.verts.shape[0] == 0 or base.verts.shape[0] == 0:
            return None
        patch, patch_boundary, _keep, _n_new = regions._patch_for_box(patch, cut.box, outlier_face_threshold, fill=False)
        if patch_boundary.shape[0] == 0:
            return None
        _faces, base_boundary, _n_new = regions._base_for_box(base, cut.box, pad, fill=False)
        if base_boundary.shape[0] == 0:
            return None
        st = regions.connect_two_meshes(base.verts, base.faces, base_boundary, patch.verts, patch.faces, patch_boundary)
        base_face_mask = regions.compose_face_mask(base.face_mask, st.face_mask[:int(base.faces.shape[0])])
        return regions.RegionStitch(stitched=st, patch=patch, base_face_mask=base_face_mask)

    def update_mesh_topology(self, res, fusion_mesh, aabb_pad: Optional[float] = None, delta_threshold: float = 0.6,
                             cc_face_threshold: int = 80, colors: bool = False, **kw):
        """update_mesh_topo and the choice of its pad (refined_mesh.py:463-693, :1033-1060) from detect_topology_errors' result
        `res` and extract_mesh_fusion's `fusion_mesh`: the regions are selected once (they do not depend on the pad); with
        aabb_pad=None the five pads are tried (regions.choose_aabb_pad) and the best one is run again, as the reference does;
        kw goes to regions.update_mesh_topology (outlier_face_threshold, force_watertight, force_short_edge,
        max_hole_vert_num).  -> regions.TopologyUpdate (its save() writes updated_mesh.obj and face_corr.npz), or None when
        there is nothing to update or cc_update_num == 0 (:1041, :1054).  Unlike stitch_update_region this fills the small
        holes (regions.fill_small_holes) and cuts every box out of what the previous box left.  colors=True: the result also
        carries colour (TopologyUpdate.with_colors(self.color_mesh()[2], fusion_mesh.colors)), so that its save() writes a
        coloured updated_mesh.obj from which from_mesh builds the re-refined model (train_seq.py:184-213)."""
        from . import regions
        sel = self.topology_update_regions(res, delta_threshold=delta_threshold, cc_face_threshold=cc_face_threshold)
        verts, faces = self._points.detach().float(), self._surface_mesh_faces.int()
        run = lambda pad: regions.update_mesh_topology(verts, faces, sel, fusion_mesh, aabb_pad=pad, **kw)
        if aabb_pad is None:
            aabb_pad, _scores = regions.choose_aabb_pad(run)
            if aabb_pad is None:
                return None
        out = run(aabb_pad)
        if out.cc_update_num <= 0:
            return None
        return out.with_colors(self.color_mesh()[2], fusion_mesh.colors) if colors else out

    # -------------------------------------------------------------------------------- the frame hand-over
    def color_mesh(self):
        """get_color_mesh (sugar_model.py:578-588) on the device: (verts [V,3] f32, faces [F,3] int64, face_rgba [F,4] uint8), a
        face's colour from the mean SH dc of its Gaussians (handover.sh_face_colors), alpha 255."""
        from . import handover
        self._fence(self._points, self._sh_coordinates_dc)
        rgba = handover.sh_face_colors(self._sh_coordinates_dc.detach(), self.n_gaussians_per_surface_triangle)
        return self._points.detach(), self._surface_mesh_faces, rgba

    def save_color_mesh(self, path: str) -> None:
        """color_mesh.obj (refined_mesh.py:1223-1226): the face colours become vertex colours (handover.face_to_vertex_colors,
        this project's statement of trimesh's conversion on OBJ export) and are written as `v x y z r g b` with u8 / 255 --
        the file warp.warp_mesh reads and carries to warp_smooth.obj, and the reference mesh of every later frame
        (train_seq.py:115)."""
        from . import formats, handover
        verts, faces, rgba = self.color_mesh()
        vrgba = handover.face_to_vertex_colors(faces, rgba, int(verts.shape[0]))
        formats.save_obj(path, verts.cpu().numpy(), faces.cpu().numpy(), vrgba[:, :3].cpu().numpy().astype(np.float64) / 255.0)

    @classmethod
    def from_mesh(cls, verts, faces, vertex_colors, n_gaussians_per_surface_triangle: int = 6, sh_levels: int = 4,
                  initial_opacity: float = 0.1, **kw) -> "SurfaceGaussians":
        """A fresh model on a coloured mesh, as the reference's constructor builds one from surface_mesh_to_bind
        (sugar_model.py:228-240, :315, :386).  verts [V,3], faces [F,3], vertex_colors [V,>=3] in [0,1]: tensors or numpy arrays
        of any float / integer width (formats.load_obj's float64 and int64 among them).  `_sh_coordinates_dc` is RGB2SH of the
        barycentric blend of every face's vertex colours (handover.sh_dc_from_vertex_colors), `_sh_coordinates_rest` zero,
        `all_densities` inverse_sigmoid(initial_opacity) -- the reference's value when opacities are learnt (:315).
        kw: `device` (default: the tensors' GPU, else the current one) and __init__'s other arguments.  Missing colours
        raise ValueError."""
        from . import _host, _meshargs as _ma, handover
        if vertex_colors is None:
            raise ValueError("from_mesh needs vertex colours: the mesh file has none")
        dev = _host.resolve_device(kw.pop("device", None), verts, what="from_mesh")
        v, f, c = _ma.upload(verts, dev, torch.float32), _ma.upload(faces, dev, torch.long), _ma.upload(vertex_colors, dev, torch.float32)
        if c.dim() != 2 or c.shape[0] != v.shape[0] or c.shape[1] < 3:
            raise ValueError(f"vertex_colors must be [V,>=3] with V = {int(v.shape[0])}, got {tuple(c.shape)}")
        if not 0.0 < float(initial_opacity) < 1.0:
            raise ValueError("initial_opacity must lie strictly between 0 and 1")
        m = cls(v, f, n_gaussians_per_surface_triangle=n_gaussians_per_surface_triangle, sh_levels=sh_levels, **kw)
        x = torch.full((1,), float(initial_opacity), dtype=torch.float32)
        density = float(torch.log(x / (1 - x)))                  # inverse_sigmoid in f32, as the reference forms it
        with torch.no_grad():
            dc = handover.sh_dc_from_vertex_colors(m._surface_mesh_faces, c, m.surface_triangle_bary_coords[..., 0].contiguous())
            m._sh_coordinates_dc.copy_(dc.view(-1, 1, 3))
            m.all_densities.fill_(density)
        return m

    # -------------------------------------------------------------------------------- rendering
    def _settings(self, camera: NerfCamera, bg: torch.Tensor, sh_degree: int):
        cam, view, proj, campos = camera.on_device(self.device)
        return GaussianRasterizationSettings(image_height=cam.H, image_width=cam.W, tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg,
                                             scale_modifier=1.0, viewmatrix=view, projmatrix=proj, sh_degree=int(sh_degree),
                                             campos=campos, prefiltered=False, debug=False), view, campos

    def _scales_for_render(self, use_solid_surface: bool, use_same_scale_in_all_directions: bool):
        scales = self.scaling
        if use_same_scale_in_all_directions:                                  # :1226-1228
            scales = scales.mean(dim=-1, keepdim=True).expand(-1, 3)
        if use_solid_surface:                                                 # :1230-1232
            scales = scales.clone()
            mean_scale = scales[..., 1:].mean()
            scales[..., 1:] = torch.maximum(mean_scale, scales[..., 1:])
        return scales

    def render_image_gaussian_rasterizer(self, camera: NerfCamera, bg_color=None, sh_deg: Optional[int] = None,
                                         sh_rotations=None, compute_color_in_rasterizer: bool = False,
                                         compute_covariance_in_rasterizer: bool = True, return_2d_radii: bool = False,
                                         quaternions=None, use_solid_surface: bool = False,
                                         use_same_scale_in_all_directions: bool = False, return_opacities: bool = False,
                                         return_colors: bool = False, positions=None, point_colors=None, overwrite_extr=None):
        """sugar_model.py:1065-1311 with `camera` in place of (nerf_cameras, camera_indices).  Returns the image [H,W,3]
        or, with return_2d_radii / return_opacities / return_colors, the reference's dict.  `overwrite_extr` (a [4,4]
        world-to-camera matrix, COLMAP axes; :1119-1127, :1141-1147) replaces the camera's pose and keeps its intrinsics;
        `sh_rotations` ([P,3,3]) turns every view direction before the SH evaluation (:1200-1205);
        `compute_covariance_in_rasterizer=False` hands the rasterizer R diag(s^2) R^T instead of scales + quaternions
        (:1237-1260)."""
        if overwrite_extr is not None:
            camera = camera.with_extrinsic(overwrite_extr)
        dev = self.device
        bg = torch.zeros(3, device=dev) if bg_color is None else torch.as_tensor(bg_color, dtype=torch.float32, device=dev)
        sh_deg = self.sh_levels - 1 if sh_deg is None else int(sh_deg)
        if (positions is None and point_colors is None and quaternions is None and not compute_color_in_rasterizer
                and not use_solid_surface and not use_same_scale_in_all_directions and sh_rotations is None
                and compute_covariance_in_rasterizer
                and not (return_2d_radii or return_opacities or return_colors)):
            # the plain call (what the refinement loop issues, refine.py:552): the whole render as one autograd node
            img, _ = self.render_channels(camera, bg, sh_deg=sh_deg, depth_channels=0)
            return img.transpose(0, 1).transpose(1, 2)                        # :1298
        settings, _view, campos = self._settings(camera, bg, sh_deg)
        positions = self.points if positions is None else positions
        shs = splat_colors = None
        if point_colors is None:
            if compute_color_in_rasterizer:
                shs = self.sh_coordinates                                     # :1208
            elif sh_rotations is None:
                splat_colors = self.get_points_rgb(positions=positions, camera_centers=campos, sh_levels=sh_deg + 1)
            else:                                                             # :1200-1205
                dirs = (torch.nn.functional.normalize(positions - campos.view(1, 3), dim=-1).unsqueeze(1) @ sh_rotations)[..., 0, :]
                splat_colors = self.get_points_rgb(positions=positions, camera_centers=None, directions=dirs, sh_levels=sh_deg + 1)
        else:
            splat_colors = point_colors                                       # :1211
        splat_opacities = self.strengths.view(-1, 1)
        quaternions = self.quaternions if quaternions is None else quaternions
        scales = self._scales_for_render(use_solid_surface, use_same_scale_in_all_directions)
        screenspace_points = torch.zeros(self.n_points, 3, dtype=positions.dtype, requires_grad=True, device=dev)
        if return_2d_radii:
            screenspace_points.retain_grad()
        cov3D = None
        if not compute_covariance_in_rasterizer:                              # :1237-1260
            cov3D = producers.covariance_3d(scales, quaternions)
            scales = quaternions = None
        rendered_image, radii = GaussianRasterizer(settings)(means3D=positions, means2D=screenspace_points, shs=shs,
                                                            colors_precomp=splat_colors, opacities=splat_opacities,
                                                            scales=scales, rotations=quaternions, cov3D_precomp=cov3D)
        image = rendered_image.transpose(0, 1).transpose(1, 2)                # :1298
        if not (return_2d_radii or return_opacities or return_colors):
            return image
        outputs = {"image": image, "radii": radii, "viewspace_points": screenspace_points}
        if return_opacities:
            outputs["opacities"] = splat_opacities
        if return_colors:
            outputs["colors"] = splat_colors
        return outputs

    def view_depth_colors(self, camera: NerfCamera, positions=None):
        """refine.py:603-605: view-space z of every Gaussian, expanded to three channels."""
        _cam, view, _proj, _campos = camera.on_device(self.device)
        positions = self.points if positions is None else positions
        return (positions @ view[:3, 2:3] + view[3, 2]).expand(-1, 3)

    def render_channels(self, camera: NerfCamera, bg: torch.Tensor, sh_deg: Optional[int] = None, depth_channels: int = 1):
        """-> (image [3 + depth_channels, H, W], radii): SH colours (+ view-space depth as `depth_channels` = 0, 1 or 3 more
        colour channels; bg has one entry per channel) rendered through ONE autograd node (_RenderMeshBound) -- the
        refinement loop's render.  Values and gradients are those of render_image_gaussian_rasterizer / the composition of
        producers.points_rgb_depth, torch.sigmoid and GaussianRasterizer (tests/test_gpu_harness.py)."""
        job = RenderJob(self, camera, bg, sh_deg, depth_channels, torch.is_grad_enabled())
        return _RenderMeshBound.apply(*job.params, job)

    def render_params(self) -> RenderParams:
        """The eight tensors a render reads, by name.  The one place that knows: `_delta_t` / `_delta_r` count only while the
        model is loosely bound."""
        loose = self._loose_bind
        return RenderParams(verts=self._points, raw_scales=self._scales, raw_complex=self._quaternions, densities=self.all_densities,
                            sh_dc=self._sh_coordinates_dc, sh_rest=self._sh_coordinates_rest,
                            delta_t=self._delta_t if loose else None, delta_r=self._delta_r if loose else None)

    def rgbd_step(self, camera: NerfCamera, bg: torch.Tensor, gt_rgb: torch.Tensor, gt_depth: torch.Tensor, max_depth: float,
                  dssim_factor: float = 0.2, depth_factor: float = 1.0, mask_factor: float = 1.0, grad_scale: Optional[torch.Tensor] = None,
                  sh_deg: Optional[int] = None, mesh_reg: Optional[dict] = None, param_reg: Optional[dict] = None):
        """One refinement iteration's render + losses + backward WITHOUT an autograd graph: the 4-channel render of
        render_channels(depth_channels=1), losses.rgb_depth_loss on it, the regularisers asked for and all backward passes, run
        through the very functions the autograd path runs; the parameters' `.grad` are set (added to, if present) exactly as
        `loss.backward()` would.  -> (loss, image, radii), all detached.  What it takes out is host time (tools/window_phases.py).
        grad_scale: a device scalar d(total)/d(loss), default 1.
        mesh_reg: dict of the keyword arguments of losses.surface_mesh_loss and, optionally, of losses.mesh_smoothness_loss as
        laplacian_factor / laplacian_method / area_reg_factor.  param_reg: dict of the scalar keyword arguments of
        losses.gaussian_param_loss, plus optional `pre_sh_dc` and `weight`.  The terms are those functions' (and their defaults
        refine_step._mesh_reg_terms / _param_reg_terms state); their gradients are added in place to the buffers the render's
        backward fills, before a sink hears of them; the returned loss is image + surface + smoothness + parameter terms, summed in
        that order -- what `(rgb_depth_loss(...) + surface_mesh_loss(...) + ...).backward()` gives.  None (default): without."""
        return _refine_step.rgbd_step(self, camera, bg, gt_rgb, gt_depth, max_depth, dssim_factor, depth_factor, mask_factor,
                                      grad_scale, sh_deg, mesh_reg, param_reg)

    def _bary_rows(self):
        b = getattr(self, "_bary_rows_cache", None)
        if b is None or b.device != self.device:
            b = self.surface_triangle_bary_coords[..., 0].detach().to(torch.float32).contiguous()
            self._bary_rows_cache = b
        return b

    def render_rgb_depth(self, camera: NerfCamera, bg_color=None, max_depth: float = 10.0, sh_deg: Optional[int] = None):
        """The two renders of a refinement iteration (refine.py:552 RGB, :607 depth-as-colour with bg = max_depth) as ONE
        4-channel pass (RGB + one depth channel) through one autograd node (render_channels):
        -> (rgb [H,W,3], depth [H,W])."""
        dev = self.device
        bg_rgb = torch.zeros(3, device=dev) if bg_color is None else torch.as_tensor(bg_color, dtype=torch.float32, device=dev)
        bg4 = torch.cat([bg_rgb, torch.full((1,), float(max_depth), device=dev)])   # RGB + one depth channel
        img, _ = self.render_channels(camera, bg4, sh_deg=sh_deg, depth_channels=1)
        return img[:3].permute(1, 2, 0), img[3]


def tracked_pre_sh(pre, track_face_mask=None, G: int = 6):
    """refine.py:379-383: the previous frame's SH coefficients a re-refined model is held to.  `pre`: a state dict (the
    previous model's state_dict()) or a checkpoint holding one under 'state_dict'.  -> (pre_sh_dc [M,3], pre_sh [M,K,3]):
    cat(_sh_coordinates_dc, _sh_coordinates_rest) over the Gaussians of the faces that survived the topology update
    (track_face_mask [F0] bool, regions.TopologyUpdate.track_face_mask or regions.load_tracking; each face's G Gaussians
    together, as TopologyUpdate.gaussian_mask(G) repeats it), all of them without a mask.  The surviving faces are the prefix of
    the updated mesh's faces, so pre_sh_dc is ready for rgbd_step's param_reg=dict(pre_sh_dc=...)."""
    sd = pre["state_dict"] if "state_dict" in pre else pre
    sh = torch.cat([sd["_sh_coordinates_dc"], sd["_sh_coordinates_rest"]], dim=1).detach()
    if track_face_mask is not None:
        mask = torch.as_tensor(track_face_mask).to(device=sh.device, dtype=torch.bool)
        if mask.dim() != 1 or mask.shape[0] * int(G) != sh.shape[0]:
            raise ValueError(f"track_face_mask must be [F0] with F0 G = {int(sh.shape[0])} Gaussians, got {tuple(mask.shape)} and G = {int(G)}")
        sh = sh[mask.repeat_interleave(int(G))]
    return sh[:, 0].contiguous(), sh
