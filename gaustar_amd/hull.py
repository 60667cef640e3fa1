"""Shape from silhouettes on the GPU: the visual hull of a calibrated rig's alpha masks as a mesh, and with it the per-frame
meshes a sequence's depth maps, masks and first mesh are rendered from.

The reference renders `{f:04d}/depth*/img_{c:04d}_depth.npz`, `masks*/img_{c:04d}_alpha.png` and `init_mesh_{res}.obj` from
per-frame HumanRF meshes ("ActorsHQ does not provide depth images, we use HumanRF to first reconstruct 3D meshes",
README.md:38-39).  HumanRF is CUDA-only.  What a capture does ship is 160 calibrated cameras with an alpha mask each, and
with that many views the visual hull is a tight, robust and deterministic surface:

    d2 = mask_distance(mask, threshold=128, radius=R)          # [H,W] int16: capped signed squared distance to the edge
    vol = HullVolume(lo, hi, 0.008, 0.02)                      # a fusion.TSDFVolume plus field (+inf) and count (0)
    carve_views(vol, rig, masks); finish(vol, min_views=...)   # the rig carves; field / count -> tsdf / weight / touched
    verts, faces, _ = fusion.extract_triangle_mesh(vol)        # the fusion's marching cubes, unchanged
    verts, faces = hull_mesh(rig, masks)                       # all of it, with hull_bounds, Taubin smoothing and decimation
    write_hull_meshes(gstar_dir, mask_path, mesh_dir, 0, 10, 1)   # mesh_{f:06d}_smooth_{res}.obj, the names that
        # mesh_depth.render_mesh_depth_files(from_humanrf=True) and dataprep.prepare_first_frame read

`rig` is the `cmr` dict (_rig.py); masks are rectified ones, the principal point the image's centre unless use_principal_point
reads it from the intrinsics.  The rules are stated in include/gsr.h and restated in tests/hull_ref.py.

What to know about the result:
  * a pixel beyond the image's border is unknown, neither inside nor outside: a silhouette that touches the border is not
    closed there;
  * a camera constrains a voxel only where the voxel projects onto its image (capture cameras crop the subject) and lies
    beyond znear = 0.01; a voxel needs min_views such cameras to carry a surface, elsewhere the volume has weight 0 and
    marching cubes makes no faces;
  * a visual hull over-fills concavities: no silhouette sees into them.  Depth maps rendered from it are too near there, and a
    depth loss against them is biased by as much;
  * the volume carries no colour: dataprep.color_mesh_from_views colours the mesh afterwards;
  * the state is a running minimum of values rounded to f32 and a count: the same bits for every order of the cameras, every
    split into calls, streams and ranks.
The photo-consistency refinement of the hull, which sees into those concavities: gaustar_amd.stereo (the RAFT flows:
gaustar_amd.flow).
"""
from __future__ import annotations

import os
import warnings
from typing import Callable, Optional, Tuple, Union

import numpy as np
import torch
import torch.distributed as tdist

from . import _host, _lib, _rig, formats, fusion, sweep
from ._lib import ptr as _p

ZNEAR = 0.01
MAX_RADIUS = 127
CAMERA_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"),
                         ("d2", "<u8"), ("H", "<i4"), ("W", "<i4")])      # gsr_hull.hip's HullCamera: Rig.cam16's 16 doubles, then its own
_RIG_CHECKS = dict(min_side=2, finite=True, positive_focal=True)      # what _rig.Rig.of checks beyond the layout
_IMAGE = ((), (torch.uint8, torch.int16))     # (tail, dtypes) of _rig.check_images / fetch_image: a mask, or its distance map


def _check_radius(radius) -> int:
    R = int(radius)
    if not 1 <= R <= MAX_RADIUS:
        raise ValueError(f"radius must be between 1 and {MAX_RADIUS}, got {radius}")
    return R


def _check_threshold(threshold) -> int:
    t = int(threshold)
    if not 0 <= t <= 256:
        raise ValueError(f"threshold must be between 0 and 256, got {threshold}")
    return t


def _check_image(x, dtype: torch.dtype, what: str) -> None:
    if x.dim() != 2 or x.dtype != dtype:
        raise ValueError(f"{what} must be [H,W] {dtype}, got {x.dtype} {tuple(x.shape)}")
    if x.shape[0] < 2 or x.shape[1] < 2:
        raise ValueError(f"{what} must be at least 2 x 2, got {tuple(x.shape)}")


# ------------------------------------------------------------------------------------------------ distance
@torch.no_grad()
def mask_distance(mask, threshold: int = 128, radius: int = 8, device=None) -> torch.Tensor:
    """The capped, signed, exact squared Euclidean distance to the silhouette's edge: mask [H,W] uint8 (numpy, or a torch
    tensor, which must be on a GPU) -> d2 [H,W] int16 on the device.  A pixel is inside iff mask >= threshold; an inside pixel
    holds +min(radius^2, the squared distance to the nearest outside pixel), an outside one -min(radius^2, ... nearest inside
    pixel); only pixels of the image count, so a mask of one kind holds +-radius^2 throughout.  Runs on the current stream
    without a host read.  ValueError: not [H,W] uint8, smaller than 2 x 2, radius outside [1, 127], a CPU tensor."""
    R, t = _check_radius(radius), _check_threshold(threshold)
    if isinstance(mask, torch.Tensor):
        if not mask.is_cuda:
            raise ValueError("a torch mask must be on a GPU (pass numpy for host data)")
        _check_image(mask, torch.uint8, "mask")
        m = mask.contiguous()
    else:
        a = np.asarray(mask)
        if a.dtype != np.uint8:
            raise ValueError(f"mask must be uint8, got {a.dtype}")
        m = torch.from_numpy(np.ascontiguousarray(a))
        _check_image(m, torch.uint8, "mask")
        m = m.to(_host.resolve_device(device, what="gaustar_amd.hull"))
    H, W = int(m.shape[0]), int(m.shape[1])
    if H > 65535:
        raise ValueError(f"mask has {H} rows: more than 65535")
    lib = _lib.load()
    with _host.on_device(m.device):
        d2 = torch.empty(H, W, dtype=torch.int16, device=m.device)
        ws = torch.empty(int(lib.gsr_hull_mask_distance_workspace_bytes(H, W)), dtype=torch.uint8, device=m.device)
        _lib.check(lib.gsr_hull_mask_distance(H, W, _p(m), t, R, _p(ws), _p(d2), _host.stream_of(m)), "gsr_hull_mask_distance")
    return d2


def _rig_of(rig, need_camera: bool = False) -> _rig.Rig:
    rig = _rig.Rig.of(rig, **_RIG_CHECKS)
    if need_camera and not rig.C:
        raise ValueError("the rig has no camera")
    return rig


_warned_radius = False


def _radius_needed(rig: dict, lo, hi, sdf_trunc: float) -> Tuple[float, float]:
    """(z_min, the cap radius_for's rule asks for before it is limited to 127; inf when the box reaches behind znear)."""
    rig = _rig_of(rig, need_camera=True)
    intr, extr = rig.intr, rig.extr
    if not sdf_trunc > 0:
        raise ValueError("sdf_trunc must be positive")
    lo, hi = np.asarray(lo, np.float64).reshape(3), np.asarray(hi, np.float64).reshape(3)
    ends = (lo, hi)
    corners = np.array([[ends[i][0], ends[j][1], ends[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    z = np.einsum("cj,nj->cn", extr[:, 2, :3], corners) + extr[:, 2, 3:4]
    z_min, f_max = float(z.min()), float(max(intr[:, 0, 0].max(), intr[:, 1, 1].max()))
    return z_min, (float("inf") if not z_min > ZNEAR else float(np.ceil(float(sdf_trunc) * f_max / z_min + 0.5)))


def radius_for(rig: dict, lo, hi, sdf_trunc: float) -> int:
    """The distance cap that the truncation needs: the smallest R with (R - 0.5) z_min / f_max >= sdf_trunc, z_min the least
    depth of the box [lo, hi] in any camera (at one of its corners) and f_max the largest focal length -- then a capped
    distance is clamped by finish() anyway.  At most 127: a box that comes nearer to a camera than that allows (or reaches
    behind znear) gets 127, with one warning per process; the hull is then flattened to less than sdf_trunc there."""
    global _warned_radius
    z_min, need = _radius_needed(rig, lo, hi, sdf_trunc)
    if need > MAX_RADIUS:
        if not _warned_radius:
            _warned_radius = True
            warnings.warn(f"radius_for: the box comes as near as {z_min:.3g} to a camera, which needs a distance cap of {need:g} pixels; "
                          f"capped at {MAX_RADIUS}")
        return MAX_RADIUS
    return int(max(1, need))


# ------------------------------------------------------------------------------------------------ the volume
class HullVolume(fusion.TSDFVolume):
    """A fusion.TSDFVolume over the box [lo, hi] plus the carve's state per voxel: field [nz,ny,nx] f32, the least signed
    distance to a silhouette's edge over the cameras so far in metres, positive inside, +inf before the first; count
    [nz,ny,nx] int32, the cameras that constrained the voxel.  finish() turns them into tsdf / weight / touched;
    fusion.extract_triangle_mesh reads those.  color stays zero."""

    def __init__(self, lo, hi, voxel_size: float = 0.008, sdf_trunc: float = 0.02, device=None):
        super().__init__(lo, hi, voxel_size, sdf_trunc, _host.resolve_device(device, what="gaustar_amd.hull"))

    def _allocate(self, u0, nu, voxel_size, sdf_trunc, device):
        super()._allocate(u0, nu, voxel_size, sdf_trunc, device)
        self.field = torch.full_like(self.tsdf, float("inf"))
        self.count = torch.zeros(self.tsdf.shape, dtype=torch.int32, device=self.device)


@torch.no_grad()
def carve_views(volume: HullVolume, rig: dict, masks_or_distances, views_in_flight: int = 2, rank: Optional[int] = None,
                world: Optional[int] = None, *, threshold: int = 128, radius: Optional[int] = None, use_principal_point: bool = False,
                chunk: int = 32) -> list:
    """The cameras of this rank's shard (sweep.camera_shard) into volume.field / volume.count.  masks_or_distances: one image
    per camera of the rig, [C,H,W] or a list (shapes may differ) or a callable i -> image; uint8 = a mask, whose distance map
    is made here (threshold; radius, default radius_for the volume's box), int16 = a distance map of mask_distance, taken as it
    is.  The distance maps of up to `chunk` cameras are made `views_in_flight` at a time on as many streams (sweep.run_cameras),
    then one launch carves them; a rig of 160 cameras never holds 160 maps.  When the job has more than one rank
    (torch.distributed initialised and world > 1), field is all-reduced with MIN and count with SUM once, so every rank ends
    with the whole rig's state; with an explicit rank / world and no process group, the caller's shards simply accumulate in
    the volume they are given.  The state does not depend on the order of the cameras or on how they are split.  Returns the
    camera indices of the shard."""
    if not isinstance(volume, HullVolume):
        raise ValueError("volume must be a HullVolume")
    rig = _rig_of(rig)
    C = rig.C
    _rig.check_images(masks_or_distances, rig, *_IMAGE, "mask or distance map", on_gpu=True)
    t = _check_threshold(threshold)
    if int(chunk) < 1:
        raise ValueError("chunk must be at least 1")
    dev = volume.device
    lo = volume.origin
    hi = lo + np.asarray(volume.dims, np.float64) * volume.voxel_size
    R = _check_radius(radius) if radius is not None else (radius_for(rig, lo, hi, volume.sdf_trunc) if C else 1)
    lib = _lib.load()
    mine = sweep.camera_shard(C, rank, world)
    n_world = sweep.gdist.world_size() if world is None else int(world)
    for start in range(0, len(mine), int(chunk)):
        part = mine[start:start + int(chunk)]
        maps = [None] * len(part)

        def per_camera(j, i, maps=maps):
            img = _rig.fetch_image(masks_or_distances, i, rig.hw(i), *_IMAGE, dev, "mask or distance map")
            maps[j] = img if img.dtype == torch.int16 else mask_distance(img, t, R)

        sweep.run_cameras(part, per_camera, views_in_flight, dev)
        with _host.on_device(dev):
            table = np.zeros(len(part), CAMERA_DTYPE)
            table.view(np.float64).reshape(len(part), -1)[:, :16] = [rig.cam16(i, use_principal_point) for i in part]   # 128 bytes a row
            table["d2"] = [m.data_ptr() for m in maps]
            table["H"], table["W"] = np.array([rig.hw(i) for i in part]).T
            cams = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
            _lib.check(lib.gsr_hull_carve(len(part), table.ctypes.data, _p(cams), volume.voxel_size, volume.grid, _p(volume.field),
                                          _p(volume.count), _host.stream_of(volume.field)), "gsr_hull_carve")
            main = torch.cuda.current_stream(dev)
            for m in maps:                  # made on the workers' streams, read by the carve on this one
                m.record_stream(main)
    if n_world > 1 and tdist.is_available() and tdist.is_initialized() and tdist.get_world_size() > 1:
        tdist.all_reduce(volume.field, op=tdist.ReduceOp.MIN)
        tdist.all_reduce(volume.count, op=tdist.ReduceOp.SUM)
        volume.n_views += C
    else:
        volume.n_views += len(mine)
    return mine


@torch.no_grad()
def finish(volume: HullVolume, min_views: int = 2) -> HullVolume:
    """field / count -> the TSDF: weight = 1 where count >= min_views else 0; tsdf = clamp(-field / sdf_trunc, -1, 1) under
    weight 1 else 0 (negative inside); touched = the units with a voxel of weight 1 and |tsdf| < 1.  May be called again after
    more cameras.  Returns the volume."""
    if not isinstance(volume, HullVolume):
        raise ValueError("volume must be a HullVolume")
    if int(min_views) < 1:
        raise ValueError("min_views must be at least 1")
    with _host.on_device(volume.device):
        _lib.check(_lib.load().gsr_hull_finish(volume.grid, _p(volume.field), _p(volume.count), int(min_views), volume.sdf_trunc,
                                               _p(volume.tsdf), _p(volume.weight), _p(volume.touched), _host.stream_of(volume.tsdf)),
                   "gsr_hull_finish")
    return volume


def default_min_views(n_cameras: int) -> int:
    """A quarter of the rig, at least 2 (1 for a rig of one): fewer cameras than that carve too little to call it a surface."""
    return max(min(2, int(n_cameras)), int(n_cameras) // 4, 1)


def _voxel_centres(volume: fusion.TSDFVolume, a: int) -> np.ndarray:
    n = volume.dims[a]
    k = np.arange(n)
    L = float(fusion.UNIT) * volume.voxel_size
    return (int(volume.u0[a]) + k // fusion.UNIT).astype(np.float64) * L + ((k % fusion.UNIT).astype(np.float64) + 0.5) * volume.voxel_size


def rig_box(rig: dict, shrink: float = 0.35) -> Tuple[np.ndarray, np.ndarray]:
    """Where a capture's subject stands: a cube around the point nearest to all optical axes (least squares), its half-size
    `shrink` times the distance from there to the nearest camera.  The cameras of a capture stand around the subject and look
    at it; a box that reached them would need an unbounded distance cap (radius_for)."""
    extr = _rig_of(rig, need_camera=True).extr
    if not 0 < shrink < 1:
        raise ValueError("shrink must be in (0, 1)")
    centres = -np.einsum("cji,cj->ci", extr[:, :3, :3], extr[:, :3, 3])
    axes = extr[:, 2, :3] / np.linalg.norm(extr[:, 2, :3], axis=1, keepdims=True)
    P = np.eye(3)[None] - axes[:, :, None] * axes[:, None, :]              # per camera: the projector off its axis
    focus = np.linalg.lstsq(P.sum(0), np.einsum("cij,cj->i", P, centres), rcond=None)[0]
    half = float(shrink) * float(np.linalg.norm(centres - focus, axis=1).min())
    return focus - half, focus + half


@torch.no_grad()
def hull_bounds(rig: dict, masks, lo=None, hi=None, coarse_voxel: float = 0.032, pad: Optional[float] = None, *, threshold: int = 128,
                min_views: Optional[int] = None, views_in_flight: int = 2, use_principal_point: bool = False,
                device=None) -> Tuple[np.ndarray, np.ndarray]:
    """A tight box around the hull from a coarse carve with the same kernels: voxels of coarse_voxel over [lo, hi] (default:
    rig_box), truncation 2 coarse_voxel; the box of the centres of the voxels with weight 1 and tsdf < 1 -- inside the hull or
    within the truncation of it, so that a part thinner than a coarse voxel, which may hold no centre, is kept -- padded by
    `pad` (default: one coarse voxel).  One host read (the six extremes).  min_views: as finish() takes it, default
    default_min_views -- a voxel that fewer cameras see lies in the cone of every one of them that sees the subject at all, so
    it must not count here any more than it will carry a surface later.  ValueError when nothing is inside."""
    if not coarse_voxel > 0:
        raise ValueError("coarse_voxel must be positive")
    if lo is None or hi is None:
        lo, hi = rig_box(rig)
    vol = HullVolume(lo, hi, coarse_voxel, 2.0 * coarse_voxel, device)
    top = vol.origin + np.asarray(vol.dims, np.float64) * vol.voxel_size
    R = int(min(MAX_RADIUS, max(1.0, _radius_needed(rig, vol.origin, top, vol.sdf_trunc)[1])))
    # (no warning where this is capped: a capped distance can only make a far voxel look near, and the box wider)
    carve_views(vol, rig, masks, views_in_flight, 0, 1, threshold=threshold, radius=R, use_principal_point=use_principal_point)
    finish(vol, default_min_views(_rig_of(rig).C) if min_views is None else min_views)
    with _host.on_device(vol.device):
        near = (vol.weight == 1) & (vol.tsdf < 1)
        ext = []
        for a in range(3):
            d1, d0 = (k for k in (2, 1, 0) if k != 2 - a)
            line = near.any(dim=d1).any(dim=d0)                                # [n_a] bool: axis a is array axis 2 - a
            idx = torch.arange(line.numel(), device=line.device)
            ext += [torch.where(line, idx, torch.full_like(idx, line.numel())).min(), torch.where(line, idx, torch.full_like(idx, -1)).max()]
        ext = [int(v) for v in torch.stack(ext).cpu()]
    if ext[1] < 0:
        raise ValueError("hull_bounds: no voxel is inside the hull (check the box, the masks and min_views)")
    pad = float(coarse_voxel) if pad is None else float(pad)
    out_lo, out_hi = np.zeros(3), np.zeros(3)
    for a in range(3):
        c = _voxel_centres(vol, a)
        out_lo[a], out_hi[a] = c[ext[2 * a]] - pad, c[ext[2 * a + 1]] + pad
    return out_lo, out_hi


@torch.no_grad()
def hull_mesh(rig: dict, masks, lo=None, hi=None, voxel_size: float = 0.008, sdf_trunc: float = 0.02, min_views: Optional[int] = None,
              taubin_iterations: int = 10, target_faces: int = 100_000, *, threshold: int = 128, views_in_flight: int = 2,
              use_principal_point: bool = False, coarse_voxel: float = 0.032, device=None) -> Tuple[torch.Tensor, torch.Tensor]:
    """The visual hull of the rig's masks as a mesh: (verts [V,3] f32, faces [F,3] int32) on the device.  Without lo / hi the
    box comes from hull_bounds (over rig_box); then HullVolume, carve_views, finish(min_views; default default_min_views),
    fusion.extract_triangle_mesh, remesh.smooth_taubin (taubin_iterations pairs; 0 = off) and remesh.simplify_mesh
    (target_faces; 0 = off, and a mesh that has no more faces is left alone).  Faces point outward.  This is the whole rig on
    one rank; for a sharded carve call carve_views yourself."""
    if int(taubin_iterations) < 0 or int(target_faces) < 0:
        raise ValueError("taubin_iterations and target_faces must not be negative")
    C = _rig_of(rig, need_camera=True).C
    kw = dict(threshold=threshold, use_principal_point=use_principal_point)
    if lo is None or hi is None:
        lo, hi = hull_bounds(rig, masks, lo, hi, coarse_voxel, min_views=min_views, views_in_flight=views_in_flight, device=device, **kw)
    vol = HullVolume(lo, hi, voxel_size, sdf_trunc, device)
    carve_views(vol, rig, masks, views_in_flight, 0, 1, **kw)
    finish(vol, default_min_views(C) if min_views is None else min_views)
    verts, faces, _colors = fusion.extract_triangle_mesh(vol)
    from . import remesh         # (here: remesh imports regions, which nothing else of this module needs)
    if int(taubin_iterations) > 0 and verts.shape[0]:
        verts = remesh.smooth_taubin(verts, faces, iterations=int(taubin_iterations))
    if int(target_faces) > 0 and faces.shape[0] > int(target_faces):
        small = remesh.simplify_mesh(verts, faces, int(target_faces))
        verts, faces = small.verts, small.faces
    return verts, faces


# ------------------------------------------------------------------------------------------------ files
def actorshq_mask_path(source_dir) -> Callable[[int, int], str]:
    """(camera index, frame) -> `masks/Cam{c+1:03d}/Cam{c+1:03d}_mask{f:06d}.png` under source_dir, ActorsHQ's layout."""
    root = os.fspath(source_dir)
    return lambda c, f: os.path.join(root, "masks", f"Cam{c + 1:03d}", f"Cam{c + 1:03d}_mask{f:06d}.png")


def write_hull_meshes(gstar_dir, mask_path: Union[str, os.PathLike, Callable[[int, int], str]], mesh_dir, frame_0: int = 0,
                      frame_end: int = 0, interval: int = 1, res: str = "100k", *, lo=None, hi=None, voxel_size: float = 0.008,
                      sdf_trunc: float = 0.02, min_views: Optional[int] = None, taubin_iterations: int = 10,
                      target_faces: int = 100_000, threshold: int = 128, views_in_flight: int = 2, device=None) -> list:
    """Per frame f in range(frame_0, frame_end, interval): the hull of the frame's masks, written to
    `mesh_{f:06d}_smooth_{res}.obj` under mesh_dir -- the names mesh_depth.render_mesh_depth_files(from_humanrf=True) and
    dataprep.prepare_first_frame read, which then complete the sequence's inputs unchanged.  gstar_dir must hold
    `rgb_cameras.npz` (intrinsics, extrinsics, shape); mask_path: a callable (camera index, frame) -> the 8-bit grey PNG of
    that camera's rectified alpha mask (formats.load_png_gray8), or the capture's directory (actorshq_mask_path).  The principal
    point is (W / 2, H / 2), as prepare_first_frame renders (wo_cxcy=True).  Returns the paths written."""
    rig = _rig.Rig.load(os.path.join(os.fspath(gstar_dir), "rgb_cameras.npz"), **_RIG_CHECKS)[0]
    path_of = mask_path if callable(mask_path) else actorshq_mask_path(mask_path)
    frames = list(range(int(frame_0), int(frame_end), int(interval)))
    if not frames:
        raise ValueError("no frame in range(frame_0, frame_end, interval)")
    os.makedirs(os.fspath(mesh_dir), exist_ok=True)
    out = []
    for f in frames:
        masks = [formats.load_png_gray8(path_of(c, f)) for c in range(rig.C)]
        verts, faces = hull_mesh(rig, masks, lo, hi, voxel_size, sdf_trunc, min_views, taubin_iterations, target_faces,
                                 threshold=threshold, views_in_flight=views_in_flight, device=device)
        if not int(faces.shape[0]):
            raise ValueError(f"frame {f}: the hull is empty")
        path = os.path.join(os.fspath(mesh_dir), f"mesh_{f:06d}_smooth_{res}.obj")
        formats.save_obj(path, verts.cpu().numpy(), faces.cpu().numpy())
        out.append(path)
    return out


def main(argv=None) -> int:
    """python -m gaustar_amd.hull GSTAR_DIR MASKS MESH_DIR --frame-0 A --frame-end B [--interval K] [--res 100k] ...: the hull
    meshes of a capture's frames (write_hull_meshes); MASKS is the capture's directory (masks/CamNNN/CamNNN_maskFFFFFF.png)."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gaustar_amd.hull", description=main.__doc__)
    ap.add_argument("gstar_dir")
    ap.add_argument("masks")
    ap.add_argument("mesh_dir")
    ap.add_argument("--frame-0", type=int, default=0)
    ap.add_argument("--frame-end", type=int, required=True)
    ap.add_argument("--interval", type=int, default=1)
    ap.add_argument("--res", default="100k")
    ap.add_argument("--voxel-size", type=float, default=0.008)
    ap.add_argument("--sdf-trunc", type=float, default=0.02)
    ap.add_argument("--min-views", type=int, default=None)
    ap.add_argument("--taubin", type=int, default=10, metavar="K", help="Taubin pairs (0 = off)")
    ap.add_argument("--faces", type=int, default=100_000, help="the face count to decimate to (0 = off)")
    ap.add_argument("--threshold", type=int, default=128)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    for p in write_hull_meshes(a.gstar_dir, a.masks, a.mesh_dir, a.frame_0, a.frame_end, a.interval, a.res, voxel_size=a.voxel_size,
                               sdf_trunc=a.sdf_trunc, min_views=a.min_views, taubin_iterations=a.taubin, target_faces=a.faces,
                               threshold=a.threshold, device=a.device):
        print(p)
    return 0


__all__ = ["mask_distance", "radius_for", "HullVolume", "carve_views", "finish", "default_min_views", "rig_box", "hull_bounds",
           "hull_mesh", "actorshq_mask_path", "write_hull_meshes", "CAMERA_DTYPE", "MAX_RADIUS"]

if __name__ == "__main__":
    raise SystemExit(main())
