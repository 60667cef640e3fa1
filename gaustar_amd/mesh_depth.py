"""A mesh's depth maps and masks over the rig on the GPU (data_process/render_depth_from_mesh.py:13-101,
`render_mesh_depth_w_aitviewer`).

Every stage of a tracked sequence reads, per frame and camera, the depth map and mask of the frame's INPUT mesh:
`{f:04d}/depth[_humanrf]/img_{c:04d}_depth.npz` (the depth and mask losses of refine.py:634-660, detect_topo_err,
warp_mesh_using_flow's visibility tests) and `{f:04d}/masks[_humanrf]/img_{c:04d}_alpha.png` (the camera loader,
gaustar_scene/cameras.py:97-106).  The reference renders them with aitviewer's OpenGL HeadlessRenderer and writes them with
cv2.  Here a depth-only triangle rasterizer (include/gsr.h, gsr_meshdepth.hip) draws them, behind three calls:

    view = mesh_depth_view(verts, faces, extr, intr, H, W)            # one camera: depth, mask, (face,) n_clipped
    render_mesh_depth(verts, faces, rig, sink)                        # the rig: sink(i, view) per camera of this rank's shard
    render_mesh_depth_files(camera_path, mesh_folder, gstar_folder)   # the reference's signature and files

The rules (stated once in gsr_meshdepth.hip's header, restated in numpy in tests/meshdepth_ref.py), and where they depart
from the reference's renderer:
  * the centre of pixel (row r, column c) is at image coordinates (x, y) = (c, r): the convention of this package's own
    consumers (gsr_rig.h: rig_project, then rig_query's int(pix + 0.5)), so a vertex finds its own depth at the pixel it
    queries.  OpenGL presumably samples at c + 0.5; neither aitviewer nor OpenGL is available to compare with, so parity with
    the reference's images is NOT pinned;
  * a face with any vertex at lz <= znear (default 0.01) is skipped whole and counted in n_clipped instead of being clipped
    against the near plane (the cameras of a capture rig stand outside the subject);
  * pixels nothing covers hold `background` (default 100.0; every consumer only needs it above max_depth = 10; aitviewer's own
    far value is not pinned);
  * the `_depth.jpg` colour-map preview (:97-101) is not written;
  * without a principal point (the reference's wo_cxcy=True) cx = W / 2, cy = H / 2 (_rig.py), which rig_project assumes.
Coverage has inclusive edges and no back-face culling; depth is perspective-correct in f64 and rounded to f32; the nearest
depth wins a pixel, ties go to the lower face index.  The result is an integer minimum per pixel: bitwise reproducible and
independent of small_max, of views_in_flight and of the sharding over ranks.
"""
from __future__ import annotations

import os
import threading
import warnings
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass
from typing import Callable, List, Optional

import numpy as np
import torch

from . import _host, _lib, _meshargs as _ma, _rig, formats, sweep
from ._lib import ptr as _p

ZNEAR = 0.01
BACKGROUND = 100.0
TEST_CAMERAS = [5, 15, 25, 35, 45]      # render_depth_from_mesh.py:40
MAX_WRITER_THREADS = 8


@dataclass
class MeshDepthView:
    """depth [H,W] f32: the depth of the nearest face at the pixel's centre, `background` where nothing covers; mask [H,W]
    uint8: 255 where covered, else 0; face [H,W] int32: the visible face, -1 where nothing covers (None unless asked for);
    n_clipped [1] int32 on the device: faces skipped for a vertex at lz <= znear."""
    depth: torch.Tensor
    mask: torch.Tensor
    face: Optional[torch.Tensor]
    n_clipped: torch.Tensor


def cam16(extr, intr, cx: float, cy: float):
    """The [host] camera block of gsr_mesh_depth_view: sweep.cam14's 14 doubles and the principal point (of a Rig: Rig.cam16)."""
    return _rig.camera_block(extr, intr, (cx, cy))


def _check_out(out: MeshDepthView, H: int, W: int, dev, return_faces: bool) -> None:
    want = [("depth", torch.float32), ("mask", torch.uint8)] + ([("face", torch.int32)] if return_faces else [])
    for name, dt in want:
        t = getattr(out, name)
        if t is None or tuple(t.shape) != (H, W) or t.dtype != dt or t.device != dev or not t.is_contiguous():
            raise ValueError(f"out.{name} must be a contiguous [{H},{W}] {dt} tensor on {dev}")
    n = out.n_clipped
    if n is None or n.numel() != 1 or n.dtype != torch.int32 or n.device != dev:
        raise ValueError(f"out.n_clipped must be one int32 on {dev}")


def _view(lib, v, f, block, H: int, W: int, znear: float, background: float, return_faces: bool, small_max: int,
          out: Optional[MeshDepthView]) -> MeshDepthView:
    dev = v.device
    if out is None:
        out = MeshDepthView(depth=torch.empty(H, W, dtype=torch.float32, device=dev), mask=torch.empty(H, W, dtype=torch.uint8, device=dev),
                            face=torch.empty(H, W, dtype=torch.int32, device=dev) if return_faces else None,
                            n_clipped=torch.empty(1, dtype=torch.int32, device=dev))
    else:
        _check_out(out, H, W, dev, return_faces)
    V, F = int(v.shape[0]), int(f.shape[0])
    ws = torch.empty(int(lib.gsr_mesh_depth_workspace_bytes(H, W, F)), dtype=torch.uint8, device=dev)
    face = out.face if return_faces else None
    _lib.check(lib.gsr_mesh_depth_view(H, W, V, F, _p(v), _p(f), block, float(znear), float(background), int(small_max), _p(ws),
                                       _p(out.depth), _p(out.mask), _p(face), _p(out.n_clipped), _host.stream_of(v)), "gsr_mesh_depth_view")
    return MeshDepthView(out.depth, out.mask, face, out.n_clipped)


@torch.no_grad()
def mesh_depth_view(verts, faces, extr, intr, H: int, W: int, *, principal_point=None, znear: float = ZNEAR,
                    background: float = BACKGROUND, return_faces: bool = False, small_max: int = 0,
                    out: Optional[MeshDepthView] = None, device=None) -> MeshDepthView:
    """The mesh (verts [V,3], faces [F,3]; numpy or torch) seen by one pinhole camera: extr [4,4] (or [3,4]) COLMAP
    world-to-camera, intr [3,3] (fx, fy; its principal point is NOT read), image (H, W).  principal_point: (cx, cy) in pixels,
    None = (W / 2, H / 2).  Runs on the current stream without a host read.  out: a MeshDepthView whose tensors are written in
    place.  small_max: tuning only (0 = the library's default); the result does not depend on it."""
    H, W = int(H), int(W)
    if H <= 0 or W <= 0:
        raise ValueError(f"image size must be positive, got {(H, W)}")
    v, f = _ma.mesh_on(verts, faces, _host.resolve_device(device, verts, what="mesh_depth"))
    block = cam16(extr, intr, *_rig.principal_point(H, W, principal_point))
    with _host.on_device(v.device):
        return _view(_lib.load(), v, f, block, H, W, znear, background, return_faces, small_max, out)


@torch.no_grad()
def render_mesh_depth(verts, faces, rig: dict, sink: Callable[[int, MeshDepthView], None], *, use_principal_point: bool = False,
                      views_in_flight: int = 2, rank: Optional[int] = None, world: Optional[int] = None, znear: float = ZNEAR,
                      background: float = BACKGROUND, return_faces: bool = False, small_max: int = 0, device=None) -> List[int]:
    """The mesh over the cameras of `rig` (the `cmr` dict, _rig.py).  The mesh is uploaded once; per camera i of this rank's shard
    (sweep.camera_shard) the view is rendered and handed to sink(i, view), so a rig of 160 cameras never holds 160 images.
    With views_in_flight > 1 the cameras run on that many streams (sweep.run_cameras) and sink is called from the worker's thread
    under the worker's stream: what it enqueues there is ordered after the render, and it must be safe to call from several
    threads.  (With an empty sink a second view in flight gains nothing: a view is some 45 us of device work at 1080p, DESIGN
    section 8 f13; more than one is for a sink that copies or writes.)  use_principal_point: read (cx, cy) from
    intrinsics[i][:2, 2] (the reference's wo_cxcy=False) instead of (W / 2, H / 2).  Returns the camera indices of the shard."""
    lib = _lib.load()
    rig = _rig.Rig.of(rig)
    dev = _host.resolve_device(device, verts, what="mesh_depth")
    v, f = _ma.mesh_on(verts, faces, dev)
    mine = sweep.camera_shard(rig.C, rank, world)

    def per_camera(_j, i):
        sink(i, _view(lib, v, f, rig.cam16(i, use_principal_point), *rig.hw(i), znear, background, return_faces, small_max, None))

    sweep.run_cameras(mine, per_camera, views_in_flight, dev)
    return mine


def _mesh_paths(mesh_folder, from_humanrf: bool, mesh_res: str, frame_0: int, frame_end: int, interval: int):
    """[(frame index, path)] as render_depth_from_mesh.py:61-88 pairs them."""
    folder = os.fspath(mesh_folder)
    if from_humanrf:
        return [(i, os.path.join(folder, f"mesh_{i:06d}_smooth_{mesh_res}.obj")) for i in range(frame_0, frame_end, interval)]
    names = sorted(n for n in os.listdir(folder) if not n.startswith(".") and os.path.isfile(os.path.join(folder, n)))
    other = [n for n in names if not n.lower().endswith(".obj")]
    if other:
        raise ValueError(f"{folder}: only OBJ meshes are supported, found {other[0]!r}")
    return [(k + frame_0, os.path.join(folder, names[k])) for k in range(0, len(names), interval)]


def render_mesh_depth_files(camera_path, mesh_folder, gstar_folder, test=False, wo_cxcy=False, from_humanrf=False, mesh_res="100k",
                            frame_0=0, frame_end=0, interval=1, views_in_flight: int = 2, znear: float = ZNEAR,
                            background: float = BACKGROUND) -> None:
    """render_depth_from_mesh.py:13-101 with the reference's signature and files.  Reads `ids`, `intrinsics`, `extrinsics`
    and `shape` from the camera npz (test=True: cameras [5, 15, 25, 35, 45], whose shape rows stay those of the first five, as in
    the reference); wo_cxcy=True puts the principal point at (W / 2, H / 2).  Meshes are read with formats.load_obj: with
    from_humanrf `mesh_{i:06d}_smooth_{mesh_res}.obj` for i in range(frame_0, frame_end, interval) at scale 1, otherwise
    every `interval`-th OBJ file of mesh_folder in sorted order at scale 0.001, the k-th being frame frame_0 + k; a mesh in any
    other format raises ValueError.  Writes per frame i and camera c `{i:04d}/depth{label}/img_{c:04d}_depth.npz` (key
    `depth`, f32 [H,W] of that camera, compressed) and `{i:04d}/masks{label}/img_{c:04d}_alpha.png` (8-bit grey, 255 =
    covered), label = '_humanrf' or ''.  The `_depth.jpg` preview is not written.  The compressed npz is host-bound: the files
    are written by a pool of at most 8 threads, at most twice that many images waiting, while the GPU renders on.  Warns once
    per frame whose mesh has faces at or behind `znear`."""
    rig, info = _rig.Rig.load(camera_path)
    sel = TEST_CAMERAS if test else slice(None)
    C = len(np.asarray(info["ids"])[sel])
    rig = _rig.Rig.of({"intrinsics": rig.intr[sel], "extrinsics": rig.extr[sel], "shape": rig.shape[:C]})
    label = "_humanrf" if from_humanrf else ""
    scale = 1.0 if from_humanrf else 0.001
    frames = _mesh_paths(mesh_folder, from_humanrf, mesh_res, int(frame_0), int(frame_end), int(interval))
    for _i, path in frames:
        if not path.lower().endswith(".obj") or not os.path.exists(path):
            raise ValueError(f"{path}: not an OBJ mesh")
    root = os.fspath(gstar_folder)
    threads = max(1, min(MAX_WRITER_THREADS, os.cpu_count() or 1))
    slots = threading.BoundedSemaphore(2 * threads)

    def write(i, c, depth, mask, done):
        try:
            done.synchronize()          # the copies into the pinned buffers
            np.savez_compressed(os.path.join(root, f"{i:04d}/depth{label}/img_{c:04d}_depth.npz"), depth=depth.numpy())
            formats.save_png_gray8(os.path.join(root, f"{i:04d}/masks{label}/img_{c:04d}_alpha.png"), mask.numpy())
        finally:
            slots.release()

    with ThreadPoolExecutor(max_workers=threads) as pool:
        for i, path in frames:
            os.makedirs(os.path.join(root, f"{i:04d}/masks{label}"), exist_ok=True)
            os.makedirs(os.path.join(root, f"{i:04d}/depth{label}"), exist_ok=True)
            verts, faces, _ = formats.load_obj(path)
            jobs, clipped = [], []

            def sink(c, view, i=i, jobs=jobs, clipped=clipped):
                slots.acquire()
                depth = torch.empty(view.depth.shape, dtype=torch.float32, pin_memory=True).copy_(view.depth, non_blocking=True)
                mask = torch.empty(view.mask.shape, dtype=torch.uint8, pin_memory=True).copy_(view.mask, non_blocking=True)
                clipped.append(torch.empty(1, dtype=torch.int32, pin_memory=True).copy_(view.n_clipped, non_blocking=True))
                done = torch.cuda.Event()
                done.record()
                jobs.append(pool.submit(write, i, c, depth, mask, done))

            render_mesh_depth(verts * scale, faces, rig, sink, use_principal_point=not wo_cxcy, views_in_flight=views_in_flight,
                              znear=znear, background=background)
            for j in jobs:
                j.result()
            n = max((int(x) for x in clipped), default=0)
            if n > 0:
                warnings.warn(f"{path}: up to {n} faces per camera have a vertex at or behind znear = {znear} and were not drawn")


__all__ = ["MeshDepthView", "mesh_depth_view", "render_mesh_depth", "render_mesh_depth_files", "cam16"]
