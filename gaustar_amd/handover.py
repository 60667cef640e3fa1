"""The colours a frame hands to the next one (include/gsr.h, gsr_handover.hip): five memory-bound passes on device tensors.

    rgba = sh_face_colors(sh_dc, G)                                   # get_color_mesh's face colours (sugar_model.py:578-588)
    rgba = vertex_to_face_colors(faces, vertex_colors)                # trimesh's vertex -> face conversion (the fusion patch)
    vrgba = face_to_vertex_colors(faces, face_rgba, n_verts)          # trimesh's face -> vertex conversion (OBJ export)
    dc = sh_dc_from_vertex_colors(faces, vertex_colors, bary)         # the SH dc of a model built from a coloured mesh (:235-240, :386)
    rgba = gather_face_colors(origin, base_rgba, fusion_faces, fusion_vertex_colors)   # regions.TopologyUpdate.with_colors

A colour is a row of four uint8, (r, g, b, a).  Every output is an integer or an exactly defined f32: the same inputs give the
same bits, and tests/handover_ref.py restates each in numpy.

Two departures from trimesh, on purpose:
  * The roundings -- a vertex colour in [0,1] becomes clip(rint(255 c), 0, 255); a face's colour is the floor of the integer
    mean of its three vertices; a vertex's colour is the floor of the integer mean of its incident faces -- are this project's
    statement of trimesh's conversions.  trimesh is not among this project's dependencies, so parity with it is not pinned.
  * A face made by regions.fill_small_holes carries (0, 0, 0, 0) and is left out of the vertex means, where trimesh's
    fill_holes gives new faces a library default colour, which would tint the vertices of every filled rim.
"""
from __future__ import annotations

import torch

from . import _host, _lib, _meshargs as _ma
from ._lib import ptr as _p

FILLED = -2 ** 31            # a face_origin entry: the face was made by fill_small_holes
SH_C0 = 0.28209479177387814


def _rgba(x: torch.Tensor, dev, what: str) -> torch.Tensor:
    if x.dim() != 2 or x.shape[1] != 4 or x.dtype != torch.uint8 or x.device != dev:
        raise ValueError(f"{what} must be [n,4] uint8 on the mesh's GPU")
    return x.contiguous()


def _vertex_colors(c: torch.Tensor, dev) -> torch.Tensor:
    if c.dim() != 2 or c.shape[1] < 3 or c.device != dev:
        raise ValueError("vertex colours must be [V,>=3] on the mesh's GPU")
    return c.detach().to(torch.float32).contiguous()


@torch.no_grad()
def sh_face_colors(sh_dc: torch.Tensor, G: int) -> torch.Tensor:
    """[F,4] uint8 from the SH dc of each face's G Gaussians (sh_dc [F G,3] or [F G,1,3] f32, face-major):
    np.clip(np.int32(SH2RGB(np.average(dc, axis=1)) * 255), 0, 255) on f32 (sugar_model.py:583-586), alpha 255.  Nothing is read."""
    G = int(G)
    if sh_dc.device.type != "cuda":
        raise RuntimeError("sh_dc must be on a GPU")
    if sh_dc.dtype != torch.float32 or sh_dc.numel() % (3 * G) or sh_dc.shape[-1] != 3:
        raise ValueError("sh_dc must be [F G,3] float32")
    x = sh_dc.detach().contiguous()
    F = x.numel() // (3 * G)
    out = torch.empty(F, 4, dtype=torch.uint8, device=x.device)
    with _host.on_device(x.device):
        _lib.check(_lib.load().gsr_handover_face_colors(F, G, _p(x), _p(out), _host.raw_stream(x.device.index)), "gsr_handover_face_colors")
    return out


@torch.no_grad()
def vertex_to_face_colors(faces: torch.Tensor, vertex_colors: torch.Tensor) -> torch.Tensor:
    """[F,4] uint8: per vertex clip(rint(255 c), 0, 255), per face and channel the floor of the integer mean of its three
    vertices, alpha 255.  An index outside the vertices raises ValueError.  One host read: the err word."""
    faces = _ma.faces_i32(faces)
    dev, F = faces.device, int(faces.shape[0])
    c = _vertex_colors(vertex_colors, dev)
    out = torch.empty(F, 4, dtype=torch.uint8, device=dev)
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_handover_vertex_to_face(F, int(c.shape[0]), _p(faces), _p(c), int(c.shape[1]), _p(out), _p(err),
                                                           _host.raw_stream(dev.index)), "gsr_handover_vertex_to_face")
    _ma.raise_if(int(err.cpu()))
    return out


@torch.no_grad()
def face_to_vertex_colors(faces: torch.Tensor, face_rgba: torch.Tensor, n_verts: int) -> torch.Tensor:
    """[n_verts,4] uint8: per vertex and channel the floor of the integer mean over its incident faces whose alpha is not 0,
    alpha 255; a vertex without such a face gets (0, 0, 0, 0).  Integer sums: the same bytes every call.  One host read."""
    faces = _ma.faces_i32(faces)
    dev, F, V = faces.device, int(faces.shape[0]), int(n_verts)
    rgba = _rgba(face_rgba, dev, "face_rgba")
    if rgba.shape[0] != F or V < 0:
        raise ValueError("face_rgba must have one row per face, and n_verts must not be negative")
    sums = torch.empty(max(V, 1), 4, dtype=torch.int32, device=dev)
    out = torch.empty(V, 4, dtype=torch.uint8, device=dev)
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_handover_face_to_vertex(F, V, _p(faces), _p(rgba), _p(sums), _p(out), _p(err), _host.raw_stream(dev.index)),
                   "gsr_handover_face_to_vertex")
    if V == 0 and F:
        _ma.raise_if(1)                                               # (faces without vertices)
    _ma.raise_if(int(err.cpu()))
    return out


@torch.no_grad()
def sh_dc_from_vertex_colors(faces: torch.Tensor, vertex_colors: torch.Tensor, bary: torch.Tensor) -> torch.Tensor:
    """[F G,3] f32: RGB2SH of the barycentric blend of each face's vertex colours (sugar_model.py:237-240, :386): per Gaussian g
    and channel c = (b_g0 v0 + b_g1 v1) + b_g2 v2, dc = (c - 0.5) / C0 in f32, nothing contracted.  bary: [G,3] f32.  One host
    read: the err word."""
    faces = _ma.faces_i32(faces)
    dev, F = faces.device, int(faces.shape[0])
    c = _vertex_colors(vertex_colors, dev)
    if bary.dim() != 2 or bary.shape[1] != 3 or bary.dtype != torch.float32 or bary.device != dev:
        raise ValueError("bary must be [G,3] float32 on the mesh's GPU")
    bary = bary.detach().contiguous()
    G = int(bary.shape[0])
    out = torch.empty(F * G, 3, dtype=torch.float32, device=dev)
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_handover_sh_dc(F, G, int(c.shape[0]), _p(faces), _p(c), int(c.shape[1]), _p(bary), _p(out), _p(err),
                                                  _host.raw_stream(dev.index)), "gsr_handover_sh_dc")
    _ma.raise_if(int(err.cpu()))
    return out


@torch.no_grad()
def gather_face_colors(origin: torch.Tensor, base_rgba: torch.Tensor, fusion_faces: torch.Tensor,
                       fusion_vertex_colors: torch.Tensor) -> torch.Tensor:
    """[n,4] uint8 from origin [n] int32 (regions.TopologyUpdate.face_origin): k >= 0 takes base_rgba[k]; -1 - k the colour
    vertex_to_face_colors gives face k of the fusion mesh; FILLED gives (0, 0, 0, 0).  One host read: the err word."""
    if origin.dim() != 1 or origin.dtype != torch.int32 or origin.device.type != "cuda":
        raise ValueError("origin must be [n] int32 on a GPU")
    dev, n = origin.device, int(origin.shape[0])
    origin = origin.contiguous()
    base = _rgba(base_rgba, dev, "base_rgba")
    ff = _ma.faces_i32(fusion_faces)
    if ff.device != dev:
        raise RuntimeError("the fusion mesh must be on the same GPU")
    c = _vertex_colors(fusion_vertex_colors, dev)
    out = torch.empty(n, 4, dtype=torch.uint8, device=dev)
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_handover_gather(n, _p(origin), int(base.shape[0]), _p(base), int(ff.shape[0]), int(c.shape[0]), _p(ff),
                                                   _p(c), int(c.shape[1]), _p(out), _p(err), _host.raw_stream(dev.index)), "gsr_handover_gather")
    _ma.raise_if(int(err.cpu()))
    return out


__all__ = ["FILLED", "SH_C0", "sh_face_colors", "vertex_to_face_colors", "face_to_vertex_colors", "sh_dc_from_vertex_colors",
           "gather_face_colors"]
