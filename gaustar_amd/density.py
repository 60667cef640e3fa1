"""The Gaussians' density field on the GPU (include/gsr.h, gsr_density.hip): SuGaR's `compute_density`
(gaustar_scene/sugar_model.py:1017-1040), `get_covariance` (:619-639) and `get_gaussians_closest_to_samples` (:1007-1015).

    d = compute_density(x, points, scaling, quaternions, strengths, K=16)            # [Q] f32
    d, t = compute_density(x, ..., closest_gaussians_idx=idx, return_closest_gaussian_opacities=True)

The density of a point is the sum over its K nearest Gaussians of density_factor strength exp(-1/2 |(R diag(1/s))^T (x - c)|^2).
The inputs are f32; each term is formed in float64 in the order include/gsr.h states (tests/density_ref.py restates it), a
row's terms are summed by a fixed balanced tree, and the sum is rounded to f32 once: the same bits in every call.  The
reference works in f32 throughout; the two differ by f32 rounding.  Without indices the neighbours come from gaustar_amd.knn's
exact search, whose rows hold -1 where there are fewer than K Gaussians; such a slot adds nothing (pytorch3d pads with
index 0, whose term the reference then adds).  Nothing here reads the device on the host unless indices are given: then one
read, the err word, and an index outside [-1, P) raises ValueError.
"""
from __future__ import annotations

from typing import Optional

import torch

from . import _host, _lib, _meshargs as _ma, knn, producers
from ._lib import ptr as _p

RECORD_FLOATS = 12      # 48 bytes: {cx, cy, cz, strength}, {qr, qi, qj, qk}, {s0, s1, s2, 0}
ERR_TEXTS = dict(index="compute_density: closest_gaussians_idx holds an index outside [-1, number of Gaussians)", dup=None, nan=None)


def _f32(t, name: str, shape_tail) -> torch.Tensor:
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError(f"compute_density: {name} must be a tensor on the GPU")
    if t.dtype != torch.float32:
        raise ValueError(f"compute_density: {name} must be float32, got {t.dtype}")
    if t.dim() != 1 + len(shape_tail) or tuple(t.shape[1:]) != tuple(shape_tail):
        raise ValueError(f"compute_density: {name} must be [n{''.join(',%d' % s for s in shape_tail)}], got {tuple(t.shape)}")
    t = t.detach().contiguous()
    return t.clone() if t.data_ptr() & 15 else t      # (a view into the middle of an array: the kernels move 16 bytes at a time)


@torch.no_grad()
def pack_records(points, scaling, quaternions, strengths) -> torch.Tensor:
    """gsr_density_pack: [P,3], [P,3], [P,4] and [P] or [P,1] f32 -> records [P,12] f32, the inputs' bits verbatim."""
    pts = _f32(points, "points", (3,))
    P = int(pts.shape[0])
    s = _f32(scaling, "scaling", (3,))
    q = _f32(quaternions, "quaternions", (4,))
    if isinstance(strengths, torch.Tensor) and strengths.dim() == 2 and strengths.shape[1] == 1:
        strengths = strengths[:, 0]
    w = _f32(strengths, "strengths", ())
    if not (s.shape[0] == q.shape[0] == w.shape[0] == P):
        raise ValueError(f"compute_density: {P} points, {int(s.shape[0])} scalings, {int(q.shape[0])} quaternions, "
                         f"{int(w.shape[0])} strengths")
    if not (s.device == q.device == w.device == pts.device):
        raise ValueError("compute_density: the Gaussians' tensors are on different devices")
    rec = torch.empty(P, RECORD_FLOATS, dtype=torch.float32, device=pts.device)
    with _host.on_device(pts.device):
        _lib.check(_lib.load().gsr_density_pack(P, _p(pts), _p(s), _p(q), _p(w), _p(rec), _host.stream_of(pts)), "gsr_density_pack")
    return rec


@torch.no_grad()
def eval_records(x: torch.Tensor, idx: torch.Tensor, records: torch.Tensor, density_factor: float, opacities: bool, err: torch.Tensor):
    """gsr_density_eval: x [Q,3] f32, idx [Q,K] int32, records of pack_records, err [1] int32 (zero before; not read here) ->
    (density [Q] f32, neighbor_opacities [Q,K] f32 or None)."""
    Q, K, P = int(x.shape[0]), int(idx.shape[1]), int(records.shape[0])
    dens = torch.empty(Q, dtype=torch.float32, device=x.device)
    opac = torch.empty(Q, K, dtype=torch.float32, device=x.device) if opacities else None
    with _host.on_device(x.device):
        _lib.check(_lib.load().gsr_density_eval(Q, P, K, _p(x), _p(idx), _p(records), float(density_factor), _p(dens), _p(opac),
                                                _p(err), _host.stream_of(x)), "gsr_density_eval")
    return dens, opac


@torch.no_grad()
def closest_gaussians(x: torch.Tensor, points: torch.Tensor, K: int = 16) -> torch.Tensor:
    """The search's own rows: [Q,K] int32, ascending (d2, index), -1 beyond the Gaussians there are."""
    return knn._search(x, points, K, False, True, False)[0]


@torch.no_grad()
def compute_density(x, points, scaling, quaternions, strengths, closest_gaussians_idx: Optional[torch.Tensor] = None, K: int = 16,
                    density_factor: float = 1.0, return_closest_gaussian_opacities: bool = False):
    """sugar_model.py:1017-1040 for x [Q,3] against P Gaussians (points [P,3], scaling [P,3] activated, quaternions [P,4] real
    part first and of any norm, strengths [P] or [P,1]; f32 tensors on one GPU) -> density [Q] f32, or (density,
    neighbor_opacities [Q,K]).  closest_gaussians_idx: [Q,K'] int32 or int64 with -1 for an empty slot, 1 <= K' <= 32 (K is
    then ignored); None: the K nearest by gaustar_amd.knn's exact search."""
    xq = _f32(x, "x", (3,))
    records = pack_records(points, scaling, quaternions, strengths)
    P = int(records.shape[0])
    if records.device != xq.device:
        raise ValueError("compute_density: x and the Gaussians are on different devices")
    err = _ma.new_err(xq.device)
    given = closest_gaussians_idx is not None
    if given:
        idx = closest_gaussians_idx
        if not isinstance(idx, torch.Tensor) or idx.device != xq.device or idx.dim() != 2 or idx.shape[0] != xq.shape[0]:
            raise ValueError("compute_density: closest_gaussians_idx must be [Q,K] on x's device")
        if idx.dtype == torch.int64:      # narrowed; what int32 cannot hold must not wrap into the valid range
            idx = torch.where((idx < -1) | (idx >= P), torch.full_like(idx, -2), idx).to(torch.int32)
        elif idx.dtype != torch.int32:
            raise ValueError(f"compute_density: closest_gaussians_idx must be int32 or int64, got {idx.dtype}")
        idx = idx.contiguous()
    else:
        idx = closest_gaussians(xq, _f32(points, "points", (3,)), K)
    Kk = int(idx.shape[1])
    if not 1 <= Kk <= knn.max_k():
        raise ValueError(f"compute_density: K = {Kk} is not implemented (1 <= K <= {knn.max_k()})")
    if xq.shape[0] > 0 and P < 1:
        raise ValueError("compute_density: there are no Gaussians")
    dens, opac = eval_records(xq, idx, records, density_factor, return_closest_gaussian_opacities, err)
    if given and xq.shape[0] > 0:
        _ma.raise_if(int(err.cpu()), **ERR_TEXTS)
    return (dens, opac) if return_closest_gaussian_opacities else dens


def get_covariance(scaling: torch.Tensor, quaternions: torch.Tensor, return_full_matrix: bool = False, return_sqrt: bool = False,
                   inverse_scales: bool = False) -> torch.Tensor:
    """sugar_model.py:619-639 in the reference's own f32 torch operations: R diag(s) [P,3,3] with return_sqrt (whatever
    return_full_matrix says, as there), else (R diag(s)) (R diag(s))^T [P,3,3] with return_full_matrix, else its upper
    triangle [P,6] {xx, xy, xz, yy, yz, zz}.  inverse_scales: s -> 1 / max(s, 1e-8)."""
    if inverse_scales:
        scaling = 1. / scaling.clamp(min=1e-8)
    scaled_rotation = producers.quaternion_to_matrix(quaternions) * scaling[:, None]
    if return_sqrt:
        return scaled_rotation
    cov = scaled_rotation @ scaled_rotation.transpose(-1, -2)
    if return_full_matrix:
        return cov
    return torch.stack((cov[:, 0, 0], cov[:, 0, 1], cov[:, 0, 2], cov[:, 1, 1], cov[:, 1, 2], cov[:, 2, 2]), dim=-1)


__all__ = ["compute_density", "get_covariance", "closest_gaussians", "pack_records", "eval_records"]
