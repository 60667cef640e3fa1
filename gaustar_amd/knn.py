"""Exact K-nearest-neighbour search on the GPU (include/gsr.h, gsr_knn.hip): the one primitive the reference takes from
pytorch3d (`knn_points`: gaustar_scene/sugar_model.py:49, :253, :862, :877, :1014, gaustar_tools/warp_mesh.py:199-213) and
from simple-knn (`distCUDA2`: sugar_model.py:9, gaussian_splatting/scene/gaussian_model.py:20, :134).

    idx, d2 = nearest_neighbors(queries, candidates, K=8)         # native: device tensors, idx -1 / d2 inf in empty slots
    knn = knn_points(p1[None], p2[None], K=16)                      # pytorch3d's signature and (dists, idx, knn) tuple
    d = dist_cuda2(points)                                          # simple_knn._C.distCUDA2

The rules (tests/knn_ref.py restates them): f32 points, d2 = (dx dx + dy dy) + dz dz in f32 with d = query - candidate, rows in
ascending (d2, index) order, a point with a non-finite coordinate is never a neighbour and has an empty row as a query.  The
result is the exhaustive search's bit for bit.  What makes it fast is order, and the order is plumbing done here with torch:
a 30-bit Morton code over the finite candidates' bounding box (an axis of zero extent maps to cell 0, non-finite points sort
last), one torch.sort of the candidates and one of the queries by the same code, and a searchsorted for where each query
stands among the candidates.  No result depends on the codes.  Nothing here reads the device on the host except
return_stats=True.
"""
from __future__ import annotations

from collections import namedtuple
from typing import Optional

import torch

from . import _host, _lib
from ._lib import ptr as _p

KNN = namedtuple("KNN", "dists idx knn")      # pytorch3d.ops.knn._KNN
MORTON_BITS = 10


def max_k() -> int:
    return int(_lib.load().gsr_knn_max_k())


def _spread(v: torch.Tensor) -> torch.Tensor:
    """The 10 low bits of v, two zero bits between each."""
    v = (v | (v << 16)) & 0x030000FF
    v = (v | (v << 8)) & 0x0300F00F
    v = (v | (v << 4)) & 0x030C30C3
    return (v | (v << 2)) & 0x09249249


def _box(points: torch.Tensor):
    """(lo, cells per unit) [3] of the finite points' bounding box; 0 cells per unit on an axis of zero (or no) extent."""
    finite = torch.isfinite(points).all(1, keepdim=True)
    inf = torch.full_like(points, float("inf"))
    lo = torch.where(finite, points, inf).amin(0)
    hi = torch.where(finite, points, -inf).amax(0)
    ext = hi - lo
    scale = torch.where(ext > 0, float(1 << MORTON_BITS) / ext, torch.zeros_like(ext))
    return lo, torch.nan_to_num(scale, nan=0.0, posinf=0.0, neginf=0.0)


def _morton(points: torch.Tensor, lo: torch.Tensor, scale: torch.Tensor) -> torch.Tensor:
    """[n] int64: the 30-bit code of every point's cell (clamped into the box), 2^30 for a non-finite point."""
    finite = torch.isfinite(points).all(1)
    cell = torch.nan_to_num((points - lo) * scale, nan=0.0, posinf=0.0, neginf=0.0).clamp_(0, (1 << MORTON_BITS) - 1).long()
    code = (_spread(cell[:, 0]) << 2) | (_spread(cell[:, 1]) << 1) | _spread(cell[:, 2])
    return torch.where(finite, code, torch.full_like(code, 1 << (3 * MORTON_BITS)))


def _points(x, name: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or not x.is_cuda:
        raise ValueError(f"nearest_neighbors: {name} must be a tensor on the GPU")
    if x.dtype != torch.float32:
        raise ValueError(f"nearest_neighbors: {name} must be float32, got {x.dtype} (the search is defined in f32; "
                         "round it yourself with .float() if that is what you want)")
    if x.dim() != 2 or x.shape[1] != 3:
        raise ValueError(f"nearest_neighbors: {name} must be [n,3], got {tuple(x.shape)}")
    return x.detach().contiguous()


@torch.no_grad()
def _search(queries: torch.Tensor, candidates: Optional[torch.Tensor], K: int, exclude_self: bool, cull: bool, stats: bool):
    """-> (idx [N,K] int32 with -1, d2 [N,K] f32 with inf, stats [2] int64 on the device or None)."""
    lib = _lib.load()
    q = _points(queries, "queries")
    same = candidates is None or candidates is queries
    c = q if same else _points(candidates, "candidates")
    if c.device != q.device:
        raise ValueError("nearest_neighbors: queries and candidates are on different devices")
    K = int(K)
    if not 1 <= K <= max_k():
        raise ValueError(f"nearest_neighbors: K = {K} is not implemented (1 <= K <= {max_k()})")
    N, M = int(q.shape[0]), int(c.shape[0])
    if exclude_self and N != M:
        raise ValueError("nearest_neighbors: exclude_self needs the queries to be the candidates")
    dev = q.device
    with _host.on_device(dev):
        idx = torch.empty(N, K, dtype=torch.int32, device=dev)
        d2 = torch.empty(N, K, dtype=torch.float32, device=dev)
        st = torch.zeros(2, dtype=torch.int64, device=dev) if stats else None
        if N == 0:
            return idx, d2, st
        stream = _host.stream_of(q)
        if M > 0:
            lo, scale = _box(c)
            ccode, corder = torch.sort(_morton(c, lo, scale), stable=True)
            ws = torch.empty(int(lib.gsr_knn_workspace_bytes(N, M, K)) // 4, dtype=torch.float32, device=dev)
            _lib.check(lib.gsr_knn_prepare(M, _p(c), _p(corder), _p(ws), stream), "gsr_knn_prepare")
            if same:
                qorder, qpos = corder, torch.arange(M, dtype=torch.int64, device=dev)
            else:
                qcode, qorder = torch.sort(_morton(q, lo, scale), stable=True)
                qpos = torch.searchsorted(ccode, qcode)
        else:
            ws, qpos = None, None
            qorder = torch.arange(N, dtype=torch.int64, device=dev)
        _lib.check(lib.gsr_knn_search(N, M, K, _p(q), _p(qorder), _p(qpos), _p(ws), int(bool(exclude_self)), int(bool(cull)),
                                      _p(idx), _p(d2), _p(st), stream), "gsr_knn_search")
    return idx, d2, st


def nearest_neighbors(queries, candidates=None, K: int = 1, exclude_self: bool = False, cull: bool = True,
                      return_stats: bool = False):
    """The K nearest candidates [M,3] of every query [N,3] (f32 tensors on the GPU; candidates=None: the queries themselves)
    -> (idx [N,K] int64, d2 [N,K] f32), rows in ascending (d2, index) order, (-1, inf) in the slots beyond the eligible
    candidates.  exclude_self: candidate i is skipped for query i (the queries are the candidates); a duplicate of the point
    at another index is not.  cull=False visits every pair (the exhaustive mode; same result).  return_stats: a third value,
    {'pairs': distances evaluated, 'tiles_skipped': ...} (a host read)."""
    idx, d2, st = _search(queries, candidates, K, exclude_self, cull, return_stats)
    if return_stats:
        a = st.cpu()
        return idx.long(), d2, {"pairs": int(a[0]), "tiles_skipped": int(a[1])}
    return idx.long(), d2


def knn_points(p1, p2, lengths1=None, lengths2=None, norm: int = 2, K: int = 1, version: int = -1, return_nn: bool = False,
               return_sorted: bool = True):
    """pytorch3d.ops.knn_points: p1 [B,N,D], p2 [B,M,D] -> KNN(dists [B,N,K], idx [B,N,K] int64, knn [B,N,K,D] or None), for
    D = 3, and D = 2 by zero padding (refined_mesh.py:1173).  Slots beyond M hold (0, 0) (and a zero point in `knn`), as
    pytorch3d pads.  `version` is ignored and the rows are always sorted.  p1 / p2 that require grad get gradients through
    `dists` and `knn`, which are then recomputed from idx with torch operations (the same f32 operations in the same order:
    the same bits).  Raises ValueError for what is not implemented: lengths1 / lengths2, norm != 2, other D."""
    if lengths1 is not None or lengths2 is not None:
        raise ValueError("knn_points: lengths1 / lengths2 are not implemented")
    if norm != 2:
        raise ValueError(f"knn_points: norm={norm} is not implemented (only 2)")
    if p1.dim() != 3 or p2.dim() != 3 or p1.shape[0] != p2.shape[0] or p1.shape[2] != p2.shape[2]:
        raise ValueError(f"knn_points: p1 / p2 must be [B,N,D] / [B,M,D], got {tuple(p1.shape)} / {tuple(p2.shape)}")
    D = int(p1.shape[2])
    if D not in (2, 3):
        raise ValueError(f"knn_points: D={D} is not implemented (only 3, and 2 by zero padding)")
    B, N = int(p1.shape[0]), int(p1.shape[1])
    grad = torch.is_grad_enabled() and (p1.requires_grad or p2.requires_grad)
    pad = (lambda x: torch.nn.functional.pad(x, (0, 1))) if D == 2 else (lambda x: x)
    dists, idxs, nns = [], [], []
    for b in range(B):
        a, c = pad(p1[b]), pad(p2[b])
        idx, d2, _ = _search(a, None if p2 is p1 else c, K, False, True, False)
        have = idx >= 0
        idx = idx.long().clamp_(min=0)
        if int(p2.shape[1]) == 0:
            d2 = torch.zeros_like(d2)
            nn = torch.zeros(N, K, D, dtype=p2.dtype, device=p2.device) if return_nn else None
        elif grad or return_nn:
            near = p2[b][idx] * have[..., None]
            if grad:
                d = p1[b][:, None, :] - near
                sq = d * d
                d2 = (sq[..., 0] + sq[..., 1]) + sq[..., 2] if D == 3 else sq[..., 0] + sq[..., 1]
                d2 = d2 * have
            else:
                d2 = torch.where(have, d2, torch.zeros_like(d2))
            nn = near if return_nn else None
        else:
            d2 = torch.where(have, d2, torch.zeros_like(d2))
            nn = None
        dists.append(d2); idxs.append(idx); nns.append(nn)
    return KNN(dists=torch.stack(dists) if B else p1.new_zeros(0, N, K), idx=torch.stack(idxs) if B else
               torch.zeros(0, N, K, dtype=torch.long, device=p1.device), knn=(torch.stack(nns) if B else
                                                                              p1.new_zeros(0, N, K, D)) if return_nn else None)


@torch.no_grad()
def dist_cuda2(points: torch.Tensor) -> torch.Tensor:
    """simple_knn._C.distCUDA2: [P,3] f32 on the GPU -> [P] f32, per point the mean of the squared distances to its three
    nearest other points, ((d0 + d1) + d2) / 3.0f (simple_knn.cu:182).  A duplicate of the point counts at distance 0; a
    missing neighbour counts as FLT_MAX, as the reference's initial `best` does (P <= 2: inf)."""
    lib = _lib.load()
    idx, d2, _ = _search(points, None, 3, True, True, False)
    P = int(d2.shape[0])
    out = torch.empty(P, dtype=torch.float32, device=d2.device)
    with _host.on_device(d2.device):
        _lib.check(lib.gsr_knn_mean_d2(P, 3, _p(d2), _p(out), _host.stream_of(d2)), "gsr_knn_mean_d2")
    return out


@torch.no_grad()
def voxel_groups(lib, pts: torch.Tensor, voxel_size: float, stream):
    """pts [n,3] f32 contiguous, n >= 1, binned into voxels from their minimum corner (gsr_topo_voxel_keys: Open3D's VoxelGrid
    rule) and grouped by a stable sort -> (vmin [3] f32, skeys [n] int64 ascending, order [n] int64, vid [n] int64: each sorted
    point's dense voxel id, head [n] bool: a voxel's first point, flags [1] int32: set when an axis spans too many voxels for a
    key).  Nothing is read back: vid[-1] + 1 voxels, and flags, are the caller's to read."""
    n, dev = int(pts.shape[0]), pts.device
    vmin = pts.amin(0).contiguous()
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    flags = torch.zeros(1, dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_topo_voxel_keys(n, _p(pts), _p(vmin), float(voxel_size), _p(keys), _p(flags), stream), "gsr_topo_voxel_keys")
    skeys, order = torch.sort(keys, stable=True)
    head = torch.ones(n, dtype=torch.bool, device=dev)
    head[1:] = skeys[1:] != skeys[:-1]
    vid = torch.cumsum(head.long(), 0) - 1
    return vmin, skeys, order, vid, head, flags


@torch.no_grad()
def segment_mean(sorted_ids: torch.Tensor, order: torch.Tensor, values: torch.Tensor, S: int):
    """gsr_knn_segment_mean: sorted_ids [n] int64 ascending and dense in [0, S), order [n] int64, values [n,C] f64 by element
    -> (mean [S,C] f64 summed in sorted order, count [S] int32)."""
    lib = _lib.load()
    n, C = int(values.shape[0]), int(values.shape[1])
    dev = values.device
    out = torch.zeros(S, C, dtype=torch.float64, device=dev)
    count = torch.zeros(S, dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        _lib.check(lib.gsr_knn_segment_mean(n, int(S), C, _p(sorted_ids.contiguous()), _p(order.contiguous()),
                                            _p(values.contiguous()), _p(out), _p(count), _host.stream_of(out)), "gsr_knn_segment_mean")
    return out, count


@torch.no_grad()
def weighted_mean(idx: torch.Tensor, d2: torch.Tensor, values: torch.Tensor, inv_scale: float) -> torch.Tensor:
    """gsr_knn_weighted_mean: idx [N,K] int32 (-1: empty), d2 [N,K] f32, values [M,C] f64 -> [N,C] f64 with the weights
    exp(-d2 inv_scale) + 1e-8 in f64; an empty slot counts as (index 0, distance 0)."""
    lib = _lib.load()
    N, K = int(idx.shape[0]), int(idx.shape[1])
    M, C = int(values.shape[0]), int(values.shape[1])
    out = torch.empty(N, C, dtype=torch.float64, device=values.device)
    with _host.on_device(values.device):
        _lib.check(lib.gsr_knn_weighted_mean(N, K, C, M, _p(idx.contiguous()), _p(d2.contiguous()), _p(values.contiguous()),
                                             float(inv_scale), _p(out), _host.stream_of(out)), "gsr_knn_weighted_mean")
    return out


__all__ = ["KNN", "nearest_neighbors", "knn_points", "dist_cuda2", "segment_mean", "weighted_mean", "max_k"]
