"""Points followed on the surface from frame to frame, through topology updates (include/gsr.h, gsr_track.hip): the
trajectories of tracking_face (gaustar_tools/tracking_util.py:34-148) and the binding step of find_face_of_tags (:20-27).

    tracker = SurfaceTracker.dense(n_faces, device=dev)               # or .sample(n_faces): the reference's one face in 200
    pos = tracker.positions(verts, faces)                             # [K,3] f64, every frame (:70); nothing is read back
    stats = tracker.rebind(pos, track_face_mask, new_verts, new_faces)   # after an update (:79-125); one host read
    stats = tracker.rebind_update(pos, upd)                           # the same from a regions.TopologyUpdate
    ids, bary = bind_points(verts, faces, points)                     # find_face_of_tags' inner step, for any points
    path, step = track_faces(base_dir, frame_0=0, frame_end=n)        # tracking_face's files, from disk to disk

A tracked point is a face id and three barycentric weights.  All arithmetic is float64, operation by operation as
include/gsr.h states it and tests/tracking_ref.py restates it in numpy: the same inputs give the same bits.  f32 vertices
(a model's) are widened, which is exact.

Two departures from the reference, on purpose:
  * point_to_bary is this project's statement of trimesh's points_to_barycentric (method "cramer").  trimesh forms its dot
    products through a BLAS call whose summation order is not defined, and trimesh is not among this project's dependencies,
    so parity with it is not pinned.
  * tracking_debug.ply, the reference's point cloud of every trajectory sample (:138-139), is not written.
"""
from __future__ import annotations

import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import _host, _lib, _meshargs as _ma
from ._lib import ptr as _p

_NAN = "a vertex or a tracked position is NaN or infinite"
_ERR = dict(nan=_NAN, degenerate="a re-bound barycentric is not >= 0: the nearest face of a point is degenerate")   # (bit 3 ranks last)
_STATUS_WORDS = 8          # err, kept, moved, lost, the to-do list's length


class RebindStats(NamedTuple):
    """The points of a re-bind by branch: n_kept stayed on their surviving face (:104-107); n_moved left a surviving face
    (its barycentrics went negative) and n_lost had their face removed -- both took the nearest face centre (:109-121)."""
    n_kept: int
    n_moved: int
    n_lost: int


def _nearest_and_bind(K: int, todo, n_todo, pos, verts, faces, ids, bary, clamp: bool, err):
    """centres -> nearest centre of every listed point -> its barycentrics on that face, all on the current stream."""
    lib, st, dev = _lib.load(), _host.stream_of(pos), pos.device
    F1, V1 = int(faces.shape[0]), int(verts.shape[0])
    centres = torch.empty(F1, 3, dtype=torch.float64, device=dev)
    idx = torch.empty(max(K, 1), dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_track_centres(F1, V1, _p(faces), _p(verts), _p(centres), _p(err), st), "gsr_track_centres")
    _lib.check(lib.gsr_track_nearest(K, _p(todo), _p(n_todo), F1, _p(pos), _p(centres), _p(idx), st), "gsr_track_nearest")
    _lib.check(lib.gsr_track_rebind_displaced(K, _p(todo), _p(n_todo), _p(idx), F1, V1, _p(faces), _p(verts), _p(pos), _p(ids),
                                              _p(bary), int(clamp), _p(err), st), "gsr_track_rebind_displaced")


class SurfaceTracker:
    """K points on a mesh, on the device: face_ids [K] int32, face_bary [K,3] f64, and face_ids_ori, the ids they started
    with (tracking_util.py:48).  face_bary=None puts every point at its face's centre, np.ones(3) / 3 (:50)."""

    def __init__(self, face_ids, face_bary=None, device="cuda"):
        dev = _host.resolve_device(device, what="a SurfaceTracker", exc=ValueError)
        ids = torch.as_tensor(np.array(face_ids) if isinstance(face_ids, np.ndarray) else face_ids)      # (a copy: it may be read-only)
        if ids.dim() != 1 or ids.dtype not in (torch.int32, torch.int64):
            raise ValueError("face_ids must be [K] int32 or int64")
        if ids.numel() and (int(ids.min()) < 0 or int(ids.max()) > 2 ** 31 - 1):
            raise ValueError("face_ids must lie in [0, 2^31)")
        self.face_ids = ids.to(dev, torch.int32).contiguous().clone()
        K = int(ids.shape[0])
        if face_bary is None:
            third = torch.from_numpy(np.ones((K, 3)) / 3)
            self.face_bary = third.to(dev)
        else:
            b = torch.as_tensor(np.array(face_bary) if isinstance(face_bary, np.ndarray) else face_bary)
            if tuple(b.shape) != (K, 3) or b.dtype != torch.float64:
                raise ValueError("face_bary must be [K,3] float64")
            self.face_bary = b.to(dev).contiguous().clone()
        self.face_ids_ori = self.face_ids.clone()
        self._err = _ma.new_err(dev)                                      # what positions() found since the last rebind()
        self._n_faces = None                                           # the faces of the mesh positions() last saw

    @classmethod
    def sample(cls, n_faces: int, first: int = 10, step: int = 200, device="cuda") -> "SurfaceTracker":
        """The reference's rule, np.arange(first, n_faces, step)[:-1] (:44-46): its last entry is dropped, so a mesh of at
        most first + step faces gives no point."""
        return cls(np.arange(int(first), int(n_faces), int(step))[:-1].astype(np.int32), device=device)

    @classmethod
    def dense(cls, n_faces: int, device="cuda") -> "SurfaceTracker":
        """Every face of a mesh of n_faces faces."""
        return cls(np.arange(int(n_faces), dtype=np.int32), device=device)

    @property
    def device(self) -> torch.device:
        return self.face_ids.device

    def __len__(self) -> int:
        return int(self.face_ids.shape[0])

    @torch.no_grad()
    def positions(self, verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
        """[K,3] f64 = bary_to_point(verts[faces[face_ids]], face_bary) (:70).  Nothing is read back: a point whose id, face or
        vertices are not valid gets a NaN row, and the next rebind() raises for it."""
        verts, faces = _ma.mesh_f64(verts, faces)
        if faces.device != self.device:
            raise ValueError("the mesh must be on the tracker's GPU")
        K = len(self)
        self._n_faces = int(faces.shape[0])
        pos = torch.empty(K, 3, dtype=torch.float64, device=self.device)
        with _host.on_device(self.device):
            _lib.check(_lib.load().gsr_track_positions(K, int(faces.shape[0]), int(verts.shape[0]), _p(faces), _p(verts), _p(self.face_ids),
                                                       _p(self.face_bary), _p(pos), _p(self._err), _host.stream_of(pos)), "gsr_track_positions")
        return pos

    @torch.no_grad()
    def rebind(self, pos: torch.Tensor, track_face_mask: torch.Tensor, new_verts: torch.Tensor, new_faces: torch.Tensor) -> RebindStats:
        """Move the points from a mesh of F0 faces to its update (:79-125).  pos [K,3] f64: positions() on the old mesh;
        track_face_mask [F0] bool: the old faces that survive, which are the first faces of the new mesh in their old order.
        A point on a surviving face keeps it if its barycentrics on the new face are all >= 0; every other point takes the
        face of the nearest centre, its barycentrics clamped at 0 and renormalised.  One host read: the err word and the three
        counts together.  A ValueError (a mask of another length than the old mesh's faces, an empty new mesh, a bad index, a
        coordinate that is not finite, a degenerate nearest face) leaves the tracker as it was."""
        dev, K = self.device, len(self)
        new_verts, new_faces = _ma.mesh_f64(new_verts, new_faces)
        if new_faces.device != dev:
            raise ValueError("the new mesh must be on the tracker's GPU")
        pos = _ma.points_f64(pos, dev, "pos")
        mask = track_face_mask
        if not torch.is_tensor(mask) or mask.dim() != 1 or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
            raise ValueError("track_face_mask must be [F0] bool on the tracker's GPU")
        if pos.shape[0] != K:
            raise ValueError("pos must have one row per tracked point")
        F0, F1, V1 = int(mask.shape[0]), int(new_faces.shape[0]), int(new_verts.shape[0])
        if self._n_faces is not None and F0 != self._n_faces:
            raise ValueError(f"track_face_mask has {F0} entries, the mesh the positions were taken on has {self._n_faces} faces")
        if F1 == 0:
            raise ValueError("the new mesh has no faces")
        lib, st = _lib.load(), _host.stream_of(pos)
        mask = mask.to(torch.uint8).contiguous()
        ones = (mask != 0).to(torch.int32)
        rank = torch.cumsum(ones, 0, dtype=torch.int32) - ones                    # np.sum(mask[:i]) (:94)
        ids, bary = self.face_ids.clone(), self.face_bary.clone()
        status = torch.zeros(_STATUS_WORDS, dtype=torch.int32, device=dev)
        status[:1] = self._err
        err, stats, n_todo = status[0:], status[1:], status[4:]
        flag = torch.empty(K, dtype=torch.int32, device=dev)
        todo = torch.empty(max(K, 1), dtype=torch.int32, device=dev)
        with _host.on_device(dev):
            _lib.check(lib.gsr_track_rebind_survivors(K, F0, F1, V1, _p(mask), _p(rank), _p(new_faces), _p(new_verts), _p(pos), _p(ids),
                                                      _p(bary), _p(flag), _p(stats), _p(err), st), "gsr_track_rebind_survivors")
            scan = torch.cumsum(flag, 0, dtype=torch.int32)
            _lib.check(lib.gsr_track_todo(K, _p(flag), _p(scan), _p(todo), _p(n_todo), st), "gsr_track_todo")
            _nearest_and_bind(K, todo, n_todo, pos, new_verts, new_faces, ids, bary, True, err)
        host = status.cpu().tolist()                                              # the one read
        self._err.zero_()
        if host[0] & 1 and F0 and K and int(self.face_ids.max()) >= F0:
            raise ValueError(f"a tracked face id is not below {F0}, the length of track_face_mask")
        _ma.raise_if(host[0], **_ERR)
        self.face_ids, self.face_bary, self._n_faces = ids, bary, None
        return RebindStats(host[1], host[2], host[3])

    def rebind_update(self, pos: torch.Tensor, upd) -> RebindStats:
        """rebind() from an in-memory regions.TopologyUpdate: its track_face_mask, verts and faces."""
        if upd.nothing_to_update:
            raise ValueError("nothing was updated: the points stay on their faces")
        return self.rebind(pos, upd.track_face_mask, upd.verts, upd.faces)


@torch.no_grad()
def bind_points(verts: torch.Tensor, faces: torch.Tensor, points: torch.Tensor, exact: bool = False):
    """(face_ids [K] int32, face_bary [K,3] f64) for any points [K,3] f64: per point the face of the nearest centre (np.argmin
    of np.linalg.norm, the lowest index among equals) and point_to_bary on it, UNCLAMPED as find_face_of_tags leaves it
    (:20-27): a point beside its face has a negative weight.  One host read: the err word.
    exact=True: a true projection instead of the reference's approximation -- the face and the barycentrics (all >= 0) of the
    closest point of the SURFACE, evaluate.surface_distance's."""
    if exact:
        from . import evaluate
        hit = evaluate.surface_distance(points, verts, faces)
        return hit.face, hit.bary
    verts, faces = _ma.mesh_f64(verts, faces)
    dev = faces.device
    pts = _ma.points_f64(points, dev, "points")
    K = int(pts.shape[0])
    if int(faces.shape[0]) == 0:
        raise ValueError("the mesh has no faces")
    if K and not bool(torch.isfinite(pts).all()):
        raise ValueError(_NAN)
    ids = torch.zeros(K, dtype=torch.int32, device=dev)
    bary = torch.empty(K, 3, dtype=torch.float64, device=dev)
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        _nearest_and_bind(K, None, None, pts, verts, faces, ids, bary, False, err)
    _ma.raise_if(int(err.cpu()), **_ERR)
    return ids, bary


def track_faces(base_dir: str, tracking_file: Optional[str] = None, frame_0: int = 0, frame_end: int = 0, interval: int = 1,
                sample_points: bool = True, dense: bool = False, device="cuda") -> Tuple[str, float]:
    """tracking_face (tracking_util.py:34-148) with its signature and files.  For f in range(frame_0, frame_end, interval) it
    reads {f:04d}/color_mesh.obj and, where {f:04d}/face_corr.npz exists, that file's track_face_mask and
    {f:04d}_update/color_mesh.obj; the position of frame f is appended BEFORE the re-bind (:70-128).  The points are every face
    of the first mesh (dense=True), else the reference's sample (sample_points=True), else face_ids / face_bary of
    tracking/{tracking_file}.  It writes tracking/tracking_{K}faces_{frame_0}to{frame_end}.npz, or tracking/tracking_{tracking_file}
    when the points came from that file, by np.savez_compressed: face_ids_ori [K], frames = [frame_0, frame_end, interval] and
    face_trajectory [n_frames, K, 3] float64.  -> (the path, the largest distance any point moved between two consecutive
    frames; 0.0 with fewer than two frames).  The reference prints the steps above 0.2; this returns the value and prints
    nothing.  tracking_debug.ply is not written.  base_dir is joined with os.path.join, so it needs no trailing slash."""
    from . import formats
    from .regions import load_tracking
    out_dir = os.path.join(base_dir, "tracking")
    os.makedirs(out_dir, exist_ok=True)
    frame_dir = lambda f, tail="": os.path.join(base_dir, f"{f:04d}{tail}")
    dev = torch.device(device)

    def mesh(path):
        v, f, _c = formats.load_obj(path)
        return torch.from_numpy(v).to(dev), torch.from_numpy(f).to(dev)

    from_file = False
    n_faces = int(formats.load_obj(os.path.join(frame_dir(frame_0), "color_mesh.obj"))[1].shape[0])
    if dense:
        tracker = SurfaceTracker.dense(n_faces, device=dev)
    elif sample_points:
        tracker = SurfaceTracker.sample(n_faces, device=dev)
    else:
        if not tracking_file:
            raise ValueError("sample_points=False needs the tracking_file that holds face_ids and face_bary")
        with np.load(os.path.join(out_dir, tracking_file)) as z:
            tracker = SurfaceTracker(z["face_ids"].astype(np.int64), z["face_bary"].astype(np.float64), device=dev)
        from_file = True
    K = len(tracker)
    rows, largest, before = [], 0.0, None
    for f in range(frame_0, frame_end, interval):
        verts, faces = mesh(os.path.join(frame_dir(f), "color_mesh.obj"))
        pos = tracker.positions(verts, faces)
        corr = os.path.join(frame_dir(f), "face_corr.npz")
        if os.path.exists(corr):
            mask, _area = load_tracking(corr)
            new_verts, new_faces = mesh(os.path.join(frame_dir(f, "_update"), "color_mesh.obj"))
            tracker.rebind(pos, torch.from_numpy(mask).to(dev), new_verts, new_faces)
        if before is not None and K:
            largest = max(largest, float(torch.linalg.vector_norm(pos - before, dim=-1).max()))
        before = pos
        rows.append(pos.cpu().numpy())
    trajectory = np.array(rows, np.float64).reshape(len(rows), K, 3)
    if not np.isfinite(trajectory).all():
        raise ValueError("a tracked face id or a face's vertex index lies outside its mesh, or a vertex is not finite")
    name = "tracking_" + tracking_file if from_file else f"tracking_{K}faces_{frame_0}to{frame_end}.npz"
    path = os.path.join(out_dir, name)
    np.savez_compressed(path, face_ids_ori=tracker.face_ids_ori.cpu().numpy(), frames=np.array([frame_0, frame_end, interval]),
                        face_trajectory=trajectory)
    return path, largest


__all__ = ["RebindStats", "SurfaceTracker", "bind_points", "track_faces"]
