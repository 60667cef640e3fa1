"""What the Python mirrors of the mesh kernels share around their launches: the checks of a mesh argument and the err word
(csrc/gsr_mesh.h; a call chain may pass one word through kernels of several files before it is read), and the way a mesh given
as numpy or torch gets onto the device.  No feature imports."""
from __future__ import annotations

from typing import Optional, Tuple

import numpy as np
import torch

MESH_ERR_INDEX, MESH_ERR_NAN, MESH_ERR_DUP, MESH_ERR_DEGENERATE = 1, 2, 4, 8      # csrc/gsr_mesh.h
MAX_FACES = (2 ** 31 - 1) // 3      # 3 F face-edges are counted in an int32

INDEX = "a vertex index, or another index into the mesh, lies outside its array"
DUP = "a boundary list names a vertex twice"
NAN_BOX = "a vertex or Gaussian centre of a kept region is NaN: its box is not defined"
NAN_BOUNDARY = "a boundary position is NaN or infinite: its nearest vertex is not defined"


def tensor_of(x) -> torch.Tensor:
    """numpy (or what numpy reads) or torch -> a tensor where the data is; numpy memory is shared when it is contiguous."""
    return x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))


def upload(x, dev, dtype: torch.dtype) -> torch.Tensor:
    """numpy or torch -> `dtype` on `dev`; a tensor that is both already is passed through."""
    return tensor_of(x).to(dev, dtype)


def verts_on(verts, dev) -> torch.Tensor:
    """numpy or torch -> [V,3] f64 contiguous on `dev`: what the f64 rig passes (mesh_depth, warp, dataprep) read."""
    v = upload(verts, dev, torch.float64).detach().contiguous()
    if v.dim() != 2 or v.shape[1] != 3:
        raise ValueError(f"verts must be [V,3], got {tuple(v.shape)}")
    return v


def mesh_on(verts, faces, dev) -> Tuple[torch.Tensor, torch.Tensor]:
    """(verts_on, faces [F,3] int32 contiguous on `dev`) from numpy or torch, the vertices first."""
    v = verts_on(verts, dev)
    f = upload(faces, dev, torch.int32).contiguous()
    if f.dim() != 2 or f.shape[1] != 3:
        raise ValueError(f"faces must be [F,3], got {tuple(f.shape)}")
    return v, f


def new_err(dev) -> torch.Tensor:
    return torch.zeros(1, dtype=torch.int32, device=dev)


def raise_if(err: int, nan: Optional[str] = NAN_BOX, *, index: str = INDEX, dup: Optional[str] = DUP,
             degenerate: Optional[str] = None, degenerate_first: bool = False) -> None:
    """ValueError with the text of the first bit of `err` that is set and has one: MESH_ERR_INDEX, then MESH_ERR_DUP, then
    MESH_ERR_NAN -- what a NaN leaves undefined is the caller's `nan` -- and MESH_ERR_DEGENERATE, the feature's own bit, either
    last or (degenerate_first) right behind the index.  A bit whose text is None is not this caller's and raises nothing."""
    ranked = [(MESH_ERR_INDEX, index), (MESH_ERR_DUP, dup), (MESH_ERR_NAN, nan)]
    ranked.insert(1 if degenerate_first else 3, (MESH_ERR_DEGENERATE, degenerate))
    for bit, text in ranked:
        if err & bit and text is not None:
            raise ValueError(text)


def faces_i32(faces: torch.Tensor) -> torch.Tensor:
    if faces.dim() != 2 or faces.shape[1] != 3:
        raise ValueError("faces must be [F,3]")
    if faces.shape[0] > MAX_FACES:
        raise ValueError(f"{faces.shape[0]} faces: more than 2^31 / 3, the face-edges cannot be indexed in int32")
    if faces.dtype not in (torch.int32, torch.int64):
        raise ValueError("faces must be int32 or int64")
    if faces.device.type != "cuda":
        raise RuntimeError("the mesh must be on a GPU")
    return faces.to(torch.int32).contiguous()


def verts_f32(verts: torch.Tensor, dev) -> torch.Tensor:
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype != torch.float32:
        raise ValueError("verts must be [V,3] float32")
    if verts.device != dev:
        raise RuntimeError("verts and faces must be on the same GPU")
    return verts.detach().contiguous()


def mesh_f32(verts: torch.Tensor, faces: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """(verts_f32, faces_i32) of one mesh, the faces checked first."""
    faces = faces_i32(faces)
    return verts_f32(verts, faces.device), faces


def mask_u8(mask: Optional[torch.Tensor], F: int, dev) -> Optional[torch.Tensor]:
    if mask is None:
        return None
    if tuple(mask.shape) != (F,) or mask.dtype not in (torch.bool, torch.uint8):
        raise ValueError("mask must be [F] bool or uint8")
    if mask.device != dev:
        raise RuntimeError("mask and faces must be on the same GPU")
    return mask.contiguous().view(torch.uint8) if mask.dtype == torch.bool else mask.contiguous()


def mesh_f64(verts: torch.Tensor, faces: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    if not torch.is_tensor(faces) or not torch.is_tensor(verts) or faces.device.type != "cuda":
        raise ValueError("verts and faces must be tensors on a GPU")
    faces = faces_i32(faces)
    if verts.dim() != 2 or verts.shape[1] != 3 or verts.dtype not in (torch.float32, torch.float64):
        raise ValueError("verts must be [V,3] float64 (or float32, which is widened)")
    if verts.device != faces.device:
        raise ValueError("verts and faces must be on the same GPU")
    return verts.detach().to(torch.float64).contiguous(), faces


def points_f64(x: torch.Tensor, dev, what: str) -> torch.Tensor:
    if x.dim() != 2 or x.shape[1] != 3 or x.dtype != torch.float64 or x.device != dev:
        raise ValueError(f"{what} must be [K,3] float64 on the tracker's GPU")
    return x.detach().contiguous()
