"""Editing a tracked sequence (include/gsr.h, gsr_edit.hip): what gaustar_tools/internal_use_tools/gstar_edit.py does with a
finished sequence -- cut a model (cut_gstar, :74-119), attach a second one that rides rigidly on tracked anchors (merge_gstar,
:122-184, best_fit_transform, :28-71), paint a texture that stays glued to tracked points (edit_gs_color, :295-388) -- on
device tensors, with the planes, anchors and paths as arguments instead of lines of the file.

    fit = fit_rigid(anchors0, face_trajectory)                        # R [T,3,3], t [T,3], n [T], ok [T]: one launch set, one read
    transform_model(model, R, t)                                      # vertices, loose-bind deltas and SH coefficients, in place
    mask = faces_in_halfspaces(verts, faces, [planes_a, planes_b])    # OR over groups of AND over planes, on face centres
    part = cut_model(model, mask)                                     # a new model of the kept faces and their Gaussians
    both = merge_models(a, b);  both = attach(a, b, R, t)             # b's faces behind a's; attach moves a copy of b first
    res = paint_decal(model, anchors_t, uv, triangles, texture)       # PaintResult(n_inside, n_painted, n_outside), in place
    edit_sequence(work_dir, out_dir, frames, 2000, [CutOp(...), AttachOp(...), PaintOp(...)], trajectory)

Every device result is stated operation by operation in include/gsr.h and restated in numpy by tests/edit_ref.py: the same
inputs give the same bits.  What stays on the host is a 3 x 3 SVD per frame and the SH rotation matrices (a least-squares
fit per band), both numpy float64.

Departures from the reference, on purpose:
  * An attached object's SH coefficients turn with it (rotate_sh=True).  The reference rotates the vertices and leaves the
    world-frame coefficients alone, so a turning object's view-dependent colour stays fixed in the world.  rotate_sh=False is
    the reference's behaviour.
  * A Gaussian the paint does not touch keeps its bits (the reference sends every dc through SH2RGB and RGB2SH), a Gaussian's
    centre is formed in float64, a texture is (r, g, b[, a]) where cv2's is (b, g, r[, a]), and a texel outside the texture is
    counted and skipped where numpy's indexing would wrap around or raise.
  * point_to_bary is this project's statement of trimesh's points_to_barycentric (gaustar_amd.tracking).
"""
from __future__ import annotations

import copy
import ctypes
import os
import shutil
from typing import Callable, List, NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import _host, _lib, _meshargs as _ma
from ._lib import ptr as _p
from .scene import SH_C0, SH_C1, SH_C2, SH_C3

MAX_GROUPS, MAX_PLANES, MAX_TRIANGLES, MAX_TABLES = 16, 64, 64, 8      # csrc/gsr_edit.hip
_PARAMS = ("_scales", "_quaternions", "all_densities", "_sh_coordinates_dc", "_sh_coordinates_rest")
_DELTAS = ("_delta_t", "_delta_r")
_MODES = {"multiply": 0, "replace": 1}


class RigidFit(NamedTuple):
    """fit_rigid's result, numpy float64: b ~ R a + t per frame.  n [T]: the anchors that counted; ok [T]: n >= 3 and the
    anchors not collinear.  A frame that is not ok has NaN in R and t."""
    R: np.ndarray
    t: np.ndarray
    n: np.ndarray
    ok: np.ndarray


class PaintResult(NamedTuple):
    """paint_decal's counters: n_inside[i] Gaussians inside triangle i, n_painted Gaussians whose dc was rewritten, n_outside
    (Gaussian, triangle) pairs whose texel fell outside the texture."""
    n_inside: List[int]
    n_painted: int
    n_outside: int


# ------------------------------------------------------------------------------------------------ argument checks
def _host_f64(x, shape, what: str) -> np.ndarray:
    """x (numpy, list or tensor) as a C-contiguous float64 array whose shape matches `shape` (None: any length)."""
    if torch.is_tensor(x):
        if x.dtype != torch.float64:
            raise ValueError(f"{what} must be float64")
        x = x.detach().cpu().numpy()
    a = np.asarray(x)
    if a.dtype != np.float64:
        raise ValueError(f"{what} must be float64")
    if a.ndim != len(shape) or any(s is not None and s != d for s, d in zip(shape, a.shape)):
        raise ValueError(f"{what} must be [{','.join('n' if s is None else str(s) for s in shape)}], got {list(a.shape)}")
    return np.ascontiguousarray(a)


def _rotation(R) -> np.ndarray:
    R = _host_f64(R, (3, 3), "R")
    if not np.isfinite(R).all():
        raise ValueError("R must be finite")
    return R


def _mesh(verts, faces):
    if not torch.is_tensor(verts) or not torch.is_tensor(faces) or faces.device.type != "cuda" or verts.device != faces.device:
        raise ValueError("verts and faces must be tensors on one GPU")
    return _ma.mesh_f32(verts, faces)


def _model(model, what: str = "model", gpu: bool = True):
    """The type first; gpu=False leaves the device to _on_gpu, for callers that check their other arguments in between."""
    from .harness import SurfaceGaussians
    if not isinstance(model, SurfaceGaussians):
        raise ValueError(f"{what} must be a SurfaceGaussians")
    return _on_gpu(model, what) if gpu else model


def _on_gpu(model, what: str = "model"):
    if model.device.type != "cuda":
        raise ValueError(f"{what} must be on a GPU")
    return model


def _has_deltas(model) -> bool:
    return getattr(model, "_delta_t", None) is not None


def _params(model) -> List[str]:
    return [*_PARAMS, *(_DELTAS if _has_deltas(model) else ())]


def _like(model, verts: torch.Tensor, faces: torch.Tensor):
    """A model on another mesh with `model`'s settings; its per-Gaussian parameters are to be filled."""
    from .harness import SurfaceGaussians
    new = SurfaceGaussians(verts, faces, n_gaussians_per_surface_triangle=model.n_gaussians_per_surface_triangle,
                           sh_levels=model.sh_levels, surface_mesh_thickness=model._thickness(),
                           min_gaussian_scale=model.min_gaussian_scale, max_gaussian_scale=model.max_gaussian_scale,
                           loose_bind=_has_deltas(model))
    new._loose_bind = model._loose_bind
    new.return_one_densities = model.return_one_densities
    return new


# ------------------------------------------------------------------------------------------------ 1. rigid fit
def rigid_from_sums(sums: np.ndarray) -> RigidFit:
    """best_fit_transform's tail (:55-64) per row {n, abar, bbar, H} of gsr_edit_fit_sums, numpy float64: U, S, Vt = svd(H),
    R = Vt^T U^T; if det R < 0, Vt[2] is negated and R formed again; t = bbar - R abar; ok = n >= 3 and S[1] > 1e-12 S[0]
    (collinear anchors leave the rotation about their line undetermined)."""
    sums = np.asarray(sums, np.float64).reshape(-1, 16)
    T = sums.shape[0]
    R, t = np.full((T, 3, 3), np.nan), np.full((T, 3), np.nan)
    n, ok = sums[:, 0].astype(np.int64), np.zeros(T, bool)
    for i in range(T):
        H = sums[i, 7:].reshape(3, 3)
        if n[i] < 3 or not np.isfinite(sums[i]).all():
            continue
        U, S, Vt = np.linalg.svd(H)
        Ri = np.dot(Vt.T, U.T)
        if np.linalg.det(Ri) < 0:
            Vt[2, :] *= -1
            Ri = np.dot(Vt.T, U.T)
        if S[1] > 1e-12 * S[0]:
            R[i], t[i], ok[i] = Ri, sums[i, 4:7] - np.dot(Ri, sums[i, 1:4]), True
    return RigidFit(R, t, n, ok)


def _f64_tensor(x, what: str) -> torch.Tensor:
    t = x.detach() if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(np.asarray(x)))
    if t.dtype != torch.float64:
        raise ValueError(f"{what} must be float64")
    return t


@torch.no_grad()
def fit_sums(src, dst, device=None) -> torch.Tensor:
    """[T,16] f64 on the device: per frame {n, abar, bbar, H} of include/gsr.h's gsr_edit_fit_sums.  src [K,3], dst [T,K,3] or
    [K,3] float64 (numpy or tensors); an anchor with a coordinate that is not finite is left out of its frame.  Nothing is read."""
    a, b = _f64_tensor(src, "src"), _f64_tensor(dst, "dst")
    if a.dim() != 2 or a.shape[1] != 3:
        raise ValueError(f"src must be [K,3], got {list(a.shape)}")
    if b.dim() == 2:
        b = b[None]
    if b.dim() != 3 or tuple(b.shape[1:]) != (int(a.shape[0]), 3):
        raise ValueError(f"dst must be [T,K,3] or [K,3] with src's K = {int(a.shape[0])}, got {list(b.shape)}")
    T, K = int(b.shape[0]), int(a.shape[0])
    if K == 0:
        raise ValueError("fit_rigid needs anchors")
    if T > 65535:
        raise ValueError("at most 65535 frames in one call")
    dev = _host.resolve_device(device, a if a.is_cuda else b, what="gaustar_amd.edit", exc=ValueError)
    a, b = a.to(dev).contiguous(), b.to(dev).contiguous()
    out = torch.empty(T, 16, dtype=torch.float64, device=dev)
    lib = _lib.load()
    with _host.on_device(dev):
        ws = torch.empty(int(lib.gsr_edit_fit_workspace_bytes(T, K)), dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_edit_fit_sums(T, K, _p(a), _p(b), _p(ws), _p(out), None, _host.stream_of(out)), "gsr_edit_fit_sums")
    return out


def fit_rigid(src, dst, device=None) -> RigidFit:
    """best_fit_transform (:28-71) of the anchors src [K,3] onto every frame of dst [T,K,3] (or [K,3]: T = 1), float64: the sums
    on the device in one set of launches (fit_sums), one host read of [T,16] doubles, then rigid_from_sums."""
    return rigid_from_sums(fit_sums(src, dst, device).cpu().numpy())


# ------------------------------------------------------------------------------------------------ 2. moving a model
def sh_basis(dirs: np.ndarray, sh_levels: int) -> np.ndarray:
    """[n, sh_levels^2] f64: the real SH basis get_points_rgb evaluates (gaustar_utils/spherical_harmonics.py:117-172, its
    constants and signs) at unit directions dirs [n,3]; colour = basis @ coefficients."""
    d = np.asarray(dirs, np.float64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    cols = [np.full_like(x, SH_C0)]
    if sh_levels > 1:
        cols += [-SH_C1 * y, SH_C1 * z, -SH_C1 * x]
    if sh_levels > 2:
        xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
        cols += [SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy)]
    if sh_levels > 3:
        cols += [SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy),
                 SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy), SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy),
                 SH_C3[6] * x * (xx - 3 * yy)]
    return np.stack(cols, axis=1)


def fibonacci_sphere(n: int = 32) -> np.ndarray:
    """[n,3] f64 unit vectors: z_i = 1 - 2 (i + 0.5) / n, azimuth (i + 0.5) pi (3 - sqrt 5)."""
    i = np.arange(n, dtype=np.float64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def sh_rotation_matrices(R, sh_levels: int) -> np.ndarray:
    """[M,M] f64, M = sh_levels^2, block diagonal 1 + 3 + 5 + 7: coefficients c of an object become D c when the object turns
    by R, so that the colour of the turned object in direction d is the colour the object had in direction R^T d.  Band l's
    block is lstsq(Y_l(d), Y_l(d R)) over the 32 directions of fibonacci_sphere taken as rows: a band is closed under
    rotation, so the fit is exact up to rounding (the bands' condition numbers are 1.0 to 1.2)."""
    R = _rotation(R)
    L = int(sh_levels)
    if L not in (1, 2, 3, 4):
        raise ValueError("sh_levels must be 1, 2, 3 or 4")
    if np.abs(R @ R.T - np.eye(3)).max() > 1e-8 or np.linalg.det(R) < 0:
        raise ValueError("R must be a rotation matrix: the SH coefficients of a reflected or sheared object are not defined here")
    d = fibonacci_sphere(32)
    Y0, Y1 = sh_basis(d, L), sh_basis(d @ R, L)
    D = np.zeros((L * L, L * L))
    for l in range(L):
        o, w = l * l, 2 * l + 1
        D[o:o + w, o:o + w] = np.linalg.lstsq(Y0[:, o:o + w], Y1[:, o:o + w], rcond=None)[0]
    return D


def _transform_rows(x: torch.Tensor, offset: int, R: np.ndarray, t: Optional[np.ndarray]) -> None:
    """Columns [offset, offset + 3) of the rows of x [n, stride] f32, in place: include/gsr.h's gsr_edit_transform_points."""
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("a model's arrays are contiguous float32")
    rp = R.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    tp = None if t is None else t.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    _lib.check(_lib.load().gsr_edit_transform_points(int(x.shape[0]), int(x.shape[1]), int(offset), _p(x), rp, tp, None, _host.stream_of(x)),
               "gsr_edit_transform_points")


def rotate_sh_rest(rest: torch.Tensor, D, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """rest [N, M - 1, 3] f32 turned by D [M,M] (sh_rotation_matrices; numpy, or a float64 tensor on rest's GPU): include/gsr.h's
    gsr_edit_rotate_sh.  out: where the result goes (rest itself: in place); default a new tensor."""
    if not torch.is_tensor(rest) or rest.device.type != "cuda" or rest.dtype != torch.float32 or rest.dim() != 3 or rest.shape[2] != 3:
        raise ValueError("rest must be [N, M - 1, 3] float32 on a GPU")
    M = int(rest.shape[1]) + 1
    if M not in (4, 9, 16):
        raise ValueError("rest must hold the 3, 8 or 15 coefficients above the dc (sh_levels 2, 3 or 4)")
    dev = rest.device
    D = D.to(dev) if torch.is_tensor(D) else torch.from_numpy(_host_f64(D, (M, M), "D")).to(dev)
    if tuple(D.shape) != (M, M) or D.dtype != torch.float64:
        raise ValueError(f"D must be [{M},{M}] float64")
    src = rest.detach()
    if not src.is_contiguous() or src.data_ptr() % 16:
        if out is rest:
            raise ValueError("rest must be contiguous and 16-byte aligned to be turned in place")
        src = src.contiguous().clone()
    if out is None:
        out = torch.empty_like(src)
    elif out.shape != rest.shape or out.dtype != torch.float32 or out.device != dev or not out.is_contiguous() or out.data_ptr() % 16:
        raise ValueError("out must be a contiguous, 16-byte aligned float32 tensor of rest's shape on its GPU")
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_edit_rotate_sh(int(src.shape[0]), M, _p(D.contiguous()), _p(src), _p(out.detach()), None,
                                                  _host.stream_of(src)), "gsr_edit_rotate_sh")
    return out


@torch.no_grad()
def transform_model(model, R, t, rotate_sh: bool = True):
    """The model moved rigidly, x -> R x + t, in place (:146 for the vertices): the vertices; the loose-bind deltas, if the
    model has them -- with R_gauss = delta R_mesh (sugar_model.py:503-505) a rigid Q gives delta' = Q delta Q^T, so `_delta_t`
    and the vector part of `_delta_r` turn like directions and its real part stays; and (rotate_sh) the SH coefficients
    above the dc.  The in-plane `_quaternions`, `_scales` and the densities do not change.  R exactly the identity launches
    nothing for the SH.  -> the model."""
    model = _model(model)
    R = _rotation(R)
    t = _host_f64(t, (3,), "t")
    if not np.isfinite(t).all():
        raise ValueError("t must be finite")
    D = None
    if rotate_sh and model.sh_levels > 1 and not np.array_equal(R, np.eye(3)):
        D = sh_rotation_matrices(R, model.sh_levels)
    model._fence()
    with _host.on_device(model.device):
        _transform_rows(model._points.data, 0, R, t)
        if _has_deltas(model):
            _transform_rows(model._delta_t.data, 0, R, None)
            _transform_rows(model._delta_r.data, 1, R, None)
        if D is not None:
            rest = model._sh_coordinates_rest.data
            if rest.is_contiguous() and rest.data_ptr() % 16 == 0:
                rotate_sh_rest(rest, D, out=rest)
            else:
                rest.copy_(rotate_sh_rest(rest, D))
    model._geom_cache = None
    return model


# ------------------------------------------------------------------------------------------------ 3. selecting and cutting
def _plane_groups(groups):
    if isinstance(groups, np.ndarray) or torch.is_tensor(groups):
        raise ValueError("groups must be a list of [n,4] plane sets")
    groups = [_host_f64(g, (None, 4), "a plane set") for g in groups]
    if not 1 <= len(groups) <= MAX_GROUPS:
        raise ValueError(f"between 1 and {MAX_GROUPS} groups of planes, got {len(groups)}")
    if any(len(g) == 0 for g in groups):
        raise ValueError("a group needs at least one plane")
    total = sum(len(g) for g in groups)
    if total > MAX_PLANES:
        raise ValueError(f"at most {MAX_PLANES} planes in all, got {total}")
    sizes = (ctypes.c_int * len(groups))(*[len(g) for g in groups])
    return sizes, np.ascontiguousarray(np.concatenate(groups, axis=0))


@torch.no_grad()
def faces_in_halfspaces(verts: torch.Tensor, faces: torch.Tensor, groups) -> torch.Tensor:
    """[F] bool: the faces whose centre ((v0 + v1) + v2) / 3 (float64 from the f32 vertices) lies, for some group, strictly on
    the positive side (a x + b y) + c z + d > 0 of every plane (a, b, c, d) of that group: cut_gstar's OR of ANDs of linear
    tests on face centres (:81-102), as data.  groups: a list of [n,4] float64 plane sets, at most 16 groups and 64 planes in
    all.  One host read: the err word."""
    sizes, planes = _plane_groups(groups)
    verts, faces = _mesh(verts, faces)
    dev, F = faces.device, int(faces.shape[0])
    mask = torch.empty(F, dtype=torch.uint8, device=dev)
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_edit_faces_in_halfspaces(F, int(verts.shape[0]), _p(faces), _p(verts), len(sizes), sizes,
                                                            planes.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), _p(mask), _p(err),
                                                            _host.stream_of(faces)), "gsr_edit_faces_in_halfspaces")
    _ma.raise_if(int(err.cpu()))
    return mask.view(torch.bool)


def _gather_rows(kept: torch.Tensor, F: int, G: int, pairs: Sequence) -> None:
    """pairs of (src [F G, ...], dst [n G, ...]) f32: one launch of gsr_edit_gather_rows; err is read."""
    dev, n = kept.device, int(kept.shape[0])
    pairs = [(s, d) for s, d in pairs if s[:1].numel() or not s.shape[0]]      # (sh_levels 1: `_sh_coordinates_rest` has no columns)
    if not 1 <= len(pairs) <= MAX_TABLES:
        raise ValueError(f"between 1 and {MAX_TABLES} arrays in one gather")
    srcs = [s.detach().contiguous() for s, _ in pairs]
    dsts = [d.detach() for _, d in pairs]
    words = []
    for s, d in zip(srcs, dsts):
        w = s[0].numel() if s.shape[0] else int(np.prod(s.shape[1:]))
        if s.element_size() != 4 or d.element_size() != 4 or not d.is_contiguous() or s.shape[0] != F * G or d.shape[0] != n * G or \
                tuple(s.shape[1:]) != tuple(d.shape[1:]) or s.device != dev or d.device != dev:
            raise ValueError("a gathered array must be [F G, ...] of a 4-byte dtype on the model's GPU")
        words.append(int(w))
    k = len(pairs)
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_edit_gather_rows(n, F, _p(kept), G, k, (ctypes.c_void_p * k)(*[s.data_ptr() for s in srcs]),
                                                    (ctypes.c_void_p * k)(*[d.data_ptr() for d in dsts]), (ctypes.c_int * k)(*words),
                                                    _p(err), _host.stream_of(kept)), "gsr_edit_gather_rows")
    _ma.raise_if(int(err.cpu()))


@torch.no_grad()
def cut_model(model, keep_faces: torch.Tensor):
    """A new model of the faces with keep_faces [F] bool set (cut_gstar, :103-116): the mesh through regions.select_faces (the
    faces in their order, unreferenced vertices dropped), and the G rows per kept face of `_scales`, `_quaternions`,
    `all_densities`, `_sh_coordinates_dc`, `_sh_coordinates_rest` (and `_delta_t`, `_delta_r`) in one launch.  An empty
    selection raises ValueError."""
    from . import regions
    model = _model(model, gpu=False)
    F, G, dev = int(model._surface_mesh_faces.shape[0]), model.n_gaussians_per_surface_triangle, model.device
    if not torch.is_tensor(keep_faces) or tuple(keep_faces.shape) != (F,) or keep_faces.dtype not in (torch.bool, torch.uint8) or \
            keep_faces.device != dev:
        raise ValueError(f"keep_faces must be [{F}] bool on the model's GPU")
    _on_gpu(model)
    model._fence()
    cut = regions.select_faces(model._points.detach(), model._surface_mesh_faces, keep_faces)
    if int(cut.faces.shape[0]) == 0:
        raise ValueError("cut_model: no face is selected")
    kept = torch.nonzero(cut.face_mask).view(-1).to(torch.int32)
    new = _like(model, cut.verts, cut.faces)
    _gather_rows(kept, F, G, [(getattr(model, k), getattr(new, k)) for k in _params(model)])
    return new


# ------------------------------------------------------------------------------------------------ 4. merging and attaching
@torch.no_grad()
def merge_models(a, b):
    """One model of both (merge_gstar, :165-184): vertices and per-Gaussian parameters concatenated, b's faces behind a's and
    offset by a's vertex count.  G, sh_levels, the thickness and the loose state must agree, else ValueError."""
    a, b = _model(a, "a", gpu=False), _model(b, "b", gpu=False)
    for what, x, y in (("n_gaussians_per_surface_triangle", a.n_gaussians_per_surface_triangle, b.n_gaussians_per_surface_triangle),
                       ("sh_levels", a.sh_levels, b.sh_levels), ("surface_mesh_thickness", a._thickness(), b._thickness()),
                       ("loose binding", (a._loose_bind, _has_deltas(a)), (b._loose_bind, _has_deltas(b)))):
        if x != y:
            raise ValueError(f"merge_models: the models differ in {what}: {x} and {y}")
    if _on_gpu(a, "a").device != _on_gpu(b, "b").device:
        raise ValueError("the two models must be on one GPU")
    a._fence(); b._fence()
    verts = torch.cat([a._points.detach(), b._points.detach()])
    faces = torch.cat([a._surface_mesh_faces, b._surface_mesh_faces + int(a._points.shape[0])])
    new = _like(a, verts, faces)
    for k in _params(a):
        getattr(new, k).copy_(torch.cat([getattr(a, k).detach(), getattr(b, k).detach()]))
    return new


def attach(a, b, R, t, rotate_sh: bool = True):
    """merge_models(a, a copy of b moved by transform_model(R, t, rotate_sh)): b itself is left as it is."""
    a, b = _model(a, "a"), _model(b, "b")
    return merge_models(a, transform_model(copy.deepcopy(b), R, t, rotate_sh))


# ------------------------------------------------------------------------------------------------ 5. painting
def _texture(texture) -> torch.Tensor:
    tex = texture if torch.is_tensor(texture) else torch.from_numpy(np.ascontiguousarray(np.asarray(texture)))
    if tex.dtype != torch.uint8:
        raise ValueError("texture must be uint8")
    if tex.dim() == 2:
        tex = tex[:, :, None]
    if tex.dim() != 3 or tex.shape[2] not in (1, 3, 4) or tex.shape[0] < 1 or tex.shape[1] < 1:
        raise ValueError(f"texture must be [h,w,C] with C = 1, 3 or 4, got {list(tex.shape)}")
    if tex.shape[0] * tex.shape[1] * 4 > 2 ** 31 - 1:
        raise ValueError("texture too large")
    return tex


@torch.no_grad()
def paint_decal(model, anchors, uv, triangles, texture, mode: str = "multiply", bary_slack: float = 0.03, max_dist: float = 0.05,
                shrink_scale: Optional[float] = -6.0, alpha_min: int = 50) -> PaintResult:
    """edit_gs_color's inner loop (:316-385), in place on the model's `_scales` and `_sh_coordinates_dc`.  anchors [K,3] and uv
    [K,2] float64: tracked points and their texture coordinates (u down the rows, v along the columns, as the reference);
    triangles [n,3] int, n <= 64, into them, walked in order; texture [h,w,C] uint8, C = 1, 3 or 4, (r, g, b[, a]).  A
    Gaussian is inside a triangle iff every barycentric of its centre is >= -bary_slack and its signed distance to the
    triangle's plane lies within (-max_dist, max_dist); an inside Gaussian's scales become shrink_scale (None: left), and its
    colour is multiplied by the texel's first channel / 255 ("multiply") or, where C = 3 or alpha > alpha_min, replaced by
    the texel ("replace").  The rules, operation by operation: include/gsr.h, gsr_edit_paint.  A triangle with a NaN anchor
    (a lost point) holds no Gaussian.  One host read: the err word and the counters."""
    model = _model(model, gpu=False)
    if mode not in _MODES:
        raise ValueError(f"mode must be 'multiply' or 'replace', got {mode!r}")
    anchors = _host_f64(anchors, (None, 3), "anchors")
    K = int(anchors.shape[0])
    uv = _host_f64(uv, (K, 2), "uv")
    tri = np.asarray(triangles.cpu().numpy() if torch.is_tensor(triangles) else triangles)
    if tri.ndim != 2 or tri.shape[1] != 3 or tri.dtype.kind not in "iu":
        raise ValueError("triangles must be [n,3] integers")
    n = int(tri.shape[0])
    if not 1 <= n <= MAX_TRIANGLES:
        raise ValueError(f"between 1 and {MAX_TRIANGLES} triangles, got {n}")
    if tri.min() < 0 or tri.max() >= K:
        raise ValueError(f"a triangle names an anchor outside [0, {K})")
    dev = model.device
    tex = _texture(texture)
    h, w, C = (int(s) for s in tex.shape)
    if mode == "replace" and C == 1:
        raise ValueError("replace needs a texture of 3 or 4 channels")
    if not np.isfinite([bary_slack, max_dist]).all() or (shrink_scale is not None and not np.isfinite(shrink_scale)):
        raise ValueError("bary_slack, max_dist and shrink_scale must be finite")
    _on_gpu(model)
    tex = tex.to(dev).contiguous()
    table = torch.from_numpy(np.concatenate([anchors[tri].reshape(n, 9), uv[tri].reshape(n, 6)], axis=1)).to(dev)
    G, F, N = model.n_gaussians_per_surface_triangle, int(model._surface_mesh_faces.shape[0]), model.n_points
    model._fence()
    verts, faces = _ma.mesh_f32(model._points.detach(), model._surface_mesh_faces)
    bary = model.surface_triangle_bary_coords[..., 0].contiguous()
    scales, dc = model._scales.data, model._sh_coordinates_dc.data
    if not (scales.is_contiguous() and dc.is_contiguous()):
        raise ValueError("a model's arrays are contiguous")
    status = torch.zeros(3 + n, dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_edit_paint(N, G, F, int(verts.shape[0]), _p(faces), _p(verts), _p(bary), n, _p(table), h, w, C, _p(tex),
                                              _MODES[mode], float(bary_slack), float(max_dist), int(shrink_scale is not None),
                                              float(shrink_scale or 0.0), int(alpha_min), _p(scales), _p(dc), _p(status[1:]), _p(status),
                                              _host.stream_of(status)), "gsr_edit_paint")
    host = status.cpu().tolist()
    model._geom_cache = None
    _ma.raise_if(host[0])
    return PaintResult(n_inside=host[3:], n_painted=host[1], n_outside=host[2])


# ------------------------------------------------------------------------------------------------ 6. a sequence
class CutOp:
    """Removes the faces faces_in_halfspaces(groups) selects, as cut_gstar does (:102); keep=True keeps them instead."""
    keeps_mesh = False

    def __init__(self, groups, keep: bool = False):
        _plane_groups(groups)
        self.groups, self.keep = groups, bool(keep)

    def __call__(self, model, frame_index, anchors_t):
        sel = faces_in_halfspaces(model._points.detach(), model._surface_mesh_faces, self.groups)
        return cut_model(model, sel if self.keep else ~sel)


class AttachOp:
    """Attaches other_model, moved so that anchors0 [K,3] (where the anchors are in other_model's frame of rest) land on the
    frame's tracked anchors (merge_gstar, :142-146).  edit_sequence calls prepare() with every frame's anchors: one fit_rigid
    call for the sequence; without it a frame is fitted when it comes.  A frame whose fit is not ok raises ValueError."""
    keeps_mesh = False

    def __init__(self, other_model, anchors0, rotate_sh: bool = True):
        self.other, self.rotate_sh = _model(other_model, "other_model"), bool(rotate_sh)
        self.anchors0 = _host_f64(anchors0, (None, 3), "anchors0")
        self.fit = None

    def prepare(self, anchors_all) -> None:
        self.fit = fit_rigid(self.anchors0, anchors_all, self.other.device)

    def __call__(self, model, frame_index, anchors_t):
        if anchors_t is None:
            raise ValueError("AttachOp needs the frame's tracked anchors: pass a trajectory")
        fit, i = (self.fit, frame_index) if self.fit is not None else (fit_rigid(self.anchors0, anchors_t, self.other.device), 0)
        if not fit.ok[i]:
            raise ValueError(f"frame {frame_index}: {int(fit.n[i])} anchors, fewer than three or collinear: no rigid fit")
        return attach(model, self.other, fit.R[i], fit.t[i], self.rotate_sh)


class PaintOp:
    """paint_decal(model, the frame's anchors, uv, triangles, texture, **kw)."""
    keeps_mesh = True

    def __init__(self, texture, uv, triangles, **kw):
        self.texture, self.uv, self.triangles, self.kw = texture, uv, triangles, kw
        self.results: List[PaintResult] = []

    def __call__(self, model, frame_index, anchors_t):
        if anchors_t is None:
            raise ValueError("PaintOp needs the frame's tracked anchors: pass a trajectory")
        self.results.append(paint_decal(model, anchors_t, self.uv, self.triangles, self.texture, **self.kw))
        return model


def _frame_anchors(trajectory, frames: Sequence[int]) -> Optional[np.ndarray]:
    """[len(frames),K,3] f64: row i of a [T,K,3] array is frames[i]; a tracking npz (tracking.track_faces: face_trajectory and
    frames = [frame_0, frame_end, interval]) is indexed by (f - frame_0) // interval (:137)."""
    if trajectory is None:
        return None
    if isinstance(trajectory, (str, os.PathLike)):
        with np.load(trajectory) as z:
            trajectory = {"face_trajectory": z["face_trajectory"], "frames": z["frames"]}
    if isinstance(trajectory, dict) or hasattr(trajectory, "files"):
        rows, (f0, f_end, step) = np.asarray(trajectory["face_trajectory"], np.float64), (int(x) for x in trajectory["frames"])
        idx = [(f - f0) // step for f in frames]
        if any(f < f0 or (f - f0) % step or i >= len(rows) for f, i in zip(frames, idx)):
            raise ValueError(f"a frame is not among the tracked ones ({f0} to {f_end} by {step})")
        return np.ascontiguousarray(rows[idx])
    rows = _host_f64(trajectory, (len(frames), None, 3), "trajectory")
    return rows


def edit_sequence(work_dir: str, out_dir: str, frames: Sequence[int], iteration: int, ops: Sequence[Callable], trajectory=None,
                  device="cuda") -> List[str]:
    """The loops of gstar_edit.py over a sequence's frames.  Per frame f: {work_dir}/{f:04d}/{iteration}.pt is loaded
    (formats.load_sugar_checkpoint), every op is applied in order -- op(model, i, anchors_t) -> model, with i the frame's
    place in `frames` and anchors_t [K,3] its row of `trajectory` ([len(frames),K,3] float64, or a tracking npz / its path, whose
    `frames` triple places the rows; None without one) -- and {out_dir}/{f:04d}/{iteration}.pt is written without the
    optimiser's state (:118).  color_mesh.obj is copied when every op keeps the mesh (PaintOp; :390) and the source has one,
    else exported from the edited model (:106, :172).  -> the checkpoints' paths."""
    from . import formats
    from .harness import SurfaceGaussians
    dev = _host.resolve_device(device, what="gaustar_amd.edit", exc=ValueError)
    frames = [int(f) for f in frames]
    anchors = _frame_anchors(trajectory, frames)
    for op in ops:
        if anchors is not None and hasattr(op, "prepare"):
            op.prepare(anchors)
    written = []
    for i, f in enumerate(frames):
        src_dir, dst_dir = os.path.join(work_dir, f"{f:04d}"), os.path.join(out_dir, f"{f:04d}")
        ckpt = formats.load_sugar_checkpoint(os.path.join(src_dir, f"{int(iteration)}.pt"))
        model = SurfaceGaussians.from_checkpoint(ckpt, dev)
        for op in ops:
            model = op(model, i, None if anchors is None else anchors[i])
        os.makedirs(dst_dir, exist_ok=True)
        extra = {k: v for k, v in ckpt["extra"].items() if k != "optimizer_state_dict"}
        deltas = _has_deltas(model)
        path = os.path.join(dst_dir, f"{int(iteration)}.pt")
        formats.save_sugar_checkpoint(path, model._points.detach(), model._surface_mesh_faces, model._scales.detach(),
                                      model._quaternions.detach(), model.all_densities.detach(), model.sh_coordinates.detach(),
                                      model._thickness(), model._delta_t.detach() if deltas else None,
                                      model._delta_r.detach() if deltas else None, **extra)
        obj = os.path.join(src_dir, "color_mesh.obj")
        if all(getattr(op, "keeps_mesh", False) for op in ops) and os.path.exists(obj):
            shutil.copy(obj, os.path.join(dst_dir, "color_mesh.obj"))
        else:
            model.save_color_mesh(os.path.join(dst_dir, "color_mesh.obj"))
        written.append(path)
    return written


__all__ = ["RigidFit", "PaintResult", "fit_sums", "rigid_from_sums", "fit_rigid", "sh_basis", "fibonacci_sphere", "sh_rotation_matrices",
           "rotate_sh_rest", "transform_model", "faces_in_halfspaces", "cut_model", "merge_models", "attach", "paint_decal", "CutOp",
           "AttachOp", "PaintOp", "edit_sequence"]
