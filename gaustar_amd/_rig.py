"""The calibrated rig that the per-camera passes walk (topology, warp, mesh_depth, dataprep, hull): the reference's `cmr` dict,
checked once on the host, and what every pass derives from a camera of it.  No feature imports.

The dict (rgb_cameras.npz's arrays, topology.rig_from_cameras for NerfCameras) holds `intrinsics` [C,3,3] (fx, fy and the
principal point in pixels), `extrinsics` [C,4,4] or [C,3,4], COLMAP world-to-camera, and `shape` [C,2] = (H, W).  The images
of a rig are rectified ones: the principal point is (W / 2, H / 2) -- what gsr_rig.h's rig_project assumes -- unless a caller
asks for the one in the intrinsics (use_principal_point, the reference's wo_cxcy=False)."""
from __future__ import annotations

import ctypes
import os
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np
import torch

from ._meshargs import tensor_of


def principal_point(H: int, W: int, given=None) -> Tuple[float, float]:
    """(cx, cy) in pixels: `given`, or the image's centre."""
    return (W / 2, H / 2) if given is None else (float(given[0]), float(given[1]))


def camera_block(extr, intr, principal=None):
    """The [host] camera block of the C ABI from one camera: the rotation (row-major) and translation of extr[:3], fx, fy
    (gsr_rig.h's RigCamera, 14 doubles), and with `principal` = (cx, cy) those two behind them (RigPinhole, 16 doubles)."""
    extr, intr = np.asarray(extr), np.asarray(intr)
    vals = list(np.asarray(extr[:3, :3], np.float64).reshape(-1)) + list(np.asarray(extr[:3, 3], np.float64)) + \
        [float(intr[0, 0]), float(intr[1, 1])] + ([] if principal is None else [float(principal[0]), float(principal[1])])
    return (ctypes.c_double * len(vals))(*vals)


@dataclass(frozen=True)
class Rig:
    """shape [C,2] as given, intr [C,3,3] and extr [C,>=3,4] float64, C cameras."""
    shape: np.ndarray
    intr: np.ndarray
    extr: np.ndarray
    C: int

    @classmethod
    def of(cls, rig, *, min_side: int = 1, finite: bool = False, positive_focal: bool = False,
           max_cameras: Optional[int] = None) -> "Rig":
        """The dict as a Rig (a Rig is returned as it is).  ValueError for a wrong layout and, as the options ask, for an image
        side below min_side, a camera that is not finite, a focal length that is not positive, more than max_cameras cameras."""
        if isinstance(rig, cls):
            return rig
        shape = np.asarray(rig["shape"])
        intr, extr = np.asarray(rig["intrinsics"], np.float64), np.asarray(rig["extrinsics"], np.float64)
        C = int(shape.shape[0]) if shape.ndim == 2 else -1
        if C < 0 or shape.shape[1] != 2 or intr.shape != (C, 3, 3) or extr.ndim != 3 or extr.shape[0] != C or extr.shape[1] < 3 \
                or extr.shape[2] != 4:
            raise ValueError("rig must hold intrinsics [C,3,3], extrinsics [C,4,4] (or [C,3,4]) and shape [C,2]")
        if max_cameras is not None and C > max_cameras:
            raise ValueError(f"{C} cameras: more than {max_cameras}, a channel's sum would not fit an int32")
        if C and (shape < min_side).any():
            raise ValueError("rig['shape'] must be positive" if min_side <= 1 else f"rig['shape'] must be at least {min_side} x {min_side}")
        if finite and not (np.isfinite(intr).all() and np.isfinite(extr).all()):
            raise ValueError("the rig's cameras must be finite")
        if positive_focal and C and not ((intr[:, 0, 0] > 0).all() and (intr[:, 1, 1] > 0).all()):
            raise ValueError("the rig's focal lengths must be positive")
        return cls(shape, intr, extr, C)

    @classmethod
    def load(cls, source, **checks) -> Tuple["Rig", dict]:
        """(Rig.of(..., **checks), info) from an `rgb_cameras.npz`'s path or a mapping of its arrays; info is that mapping
        (for a path: a dict of the file's arrays), so `ids` and `dist_coeffs` stay at hand."""
        info = dict(np.load(os.fspath(source))) if isinstance(source, (str, os.PathLike)) else source
        return cls.of({k: info[k] for k in ("intrinsics", "extrinsics", "shape")}, **checks), info

    def as_dict(self) -> dict:
        return {"intrinsics": self.intr, "extrinsics": self.extr, "shape": self.shape}

    def hw(self, i: int) -> Tuple[int, int]:
        return int(self.shape[i][0]), int(self.shape[i][1])

    def principal(self, i: int, use_principal_point: bool = False) -> Tuple[float, float]:
        return principal_point(*self.hw(i), (self.intr[i][0, 2], self.intr[i][1, 2]) if use_principal_point else None)

    def cam14(self, i: int):
        return camera_block(self.extr[i], self.intr[i])

    def cam16(self, i: int, use_principal_point: bool = False, principal_point=None):
        pp = self.principal(i, use_principal_point) if principal_point is None else principal_point
        return camera_block(self.extr[i], self.intr[i], pp)


# ---------------------------------------------------------------------------------------------- one image per camera
def _check_one(x, i, want: tuple, dtypes: tuple, what: str) -> None:
    names = [str(d)[6:] for d in dtypes]          # "torch.uint8" -> "uint8", which is how numpy prints its own
    if str(x.dtype).replace("torch.", "") not in names or tuple(x.shape) != want:
        raise ValueError(f"{what} {i} must be {want} {' or '.join(names)}, got {x.dtype} {tuple(x.shape)}")


def check_images(src, rig: Rig, tail: tuple, dtypes: tuple, what: str, *, stack_only: bool = False, on_gpu: bool = False) -> None:
    """Before a pass starts: `src` holds per camera of the rig one [H,W,*tail] array (H, W that camera's) of one of the torch
    `dtypes` or numpy's of the same name -- or is a callable i -> image, which fetch_image checks view by view.  stack_only:
    `src` must be one array [C,H,W,*tail], not a list.  on_gpu: a torch image must be on a GPU."""
    if callable(src):
        return
    if stack_only:
        if not isinstance(src, (np.ndarray, torch.Tensor)) or src.ndim != 3 + len(tail):
            raise ValueError(f"{what}s must be an array [C,H,W{''.join(f',{n}' for n in tail)}] or a callable")
        _check_one(src, "stack", (rig.C, *src.shape[1:3], *tail), dtypes, f"the {what}")
    elif not hasattr(src, "__len__") or len(src) != rig.C:
        raise ValueError(f"need one {what} per camera of the rig ({rig.C})")
    for i in range(rig.C):
        _check_one(src[i], i, (*rig.hw(i), *tail), dtypes, what)
        if on_gpu and isinstance(src[i], torch.Tensor) and src[i].device.type != "cuda":
            raise ValueError(f"{what} {i}: a torch tensor must be on a GPU (pass numpy for host data)")


def fetch_image(src, i: int, hw: Tuple[int, int], tail: tuple, dtypes: tuple, dev, what: str) -> torch.Tensor:
    """Camera i's image of `src` (a callable i -> image, or indexable; numpy or torch), checked as above, contiguous on `dev`."""
    t = tensor_of(src(i) if callable(src) else src[i])
    _check_one(t, i, (*hw, *tail), dtypes, what)
    return t.to(dev).contiguous()
