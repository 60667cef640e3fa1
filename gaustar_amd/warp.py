"""Scene-flow mesh warping to the next frame (gaustar_tools/warp_mesh.py:216-401, `warp_mesh_using_flow`) on the GPU.

Between two frames the reference moves the refined mesh along the optical flow of every camera (train_seq.py:242-245); the
warped `{f+interval:04d}/coarse_mesh/warp_smooth.obj` is the mesh the next frame starts from (train_seq.py:112).  The
reference needs trimesh, cv2, open3d and pytorch3d for it and runs numpy loops per vertex.  Here it runs as HIP kernels
(include/gsr.h, gsr_warp.hip) behind two calls:

    res = warp_mesh(verts, faces, rig, frames)            # native: move_raw / _propagated / _smoothed [V,3] f64, counts
    warp_mesh_using_flow(mesh_path, data_root, work_root, f_idx, interval=1)      # the reference's signature and files

Vertex normals are computed once per warp.  Per camera: three launches reduce the two edge maps and write the camera's row
[V,3] of a [C,V,3] table (the vertex's move, NaN where it is not visible); the RAFT flows are read raw, with the reference's
pad and nearest resize fused into the lookup.  Cameras are sharded over ranks (sweep.camera_shard) and run `views_in_flight`
at a time (pipelines.ViewPipelines); the rows come back with one all_gather (sweep.gather_rows).  Over the rig every rank runs
the same deterministic passes on the same table: outlier removal and mean per vertex, 20 propagation sweeps (gsr_topo.hip's,
one call per component), 5 smoothing sweeps.  Host synchronisations: ViewPipelines.run waits for the device before the
cameras start and each pipeline waits for its stream once its cameras are done (with views_in_flight = 1 the cameras run on the
calling stream without a wait), and warp_mesh waits for its stream once at the end.  The mesh's topology, neighbour lists and
vertex-face lists are built (with host reads) on first use and kept on the faces tensor, as meshes.MeshTopology.of does.

post_processing = 'mesh' (the reference's default) is the above.  With 'voxel' (warp_mesh.py:368-376) the propagation is not
run: the vertices with count >= min_observe are binned into voxels of cfg.voxel_size (Open3D's VoxelGrid rule, gsr_topo.hip's
keys), each voxel takes the mean move of its vertices, and every vertex takes the distance-weighted mean of its cfg.knn_K
nearest voxel centres (gaustar_amd.knn, gsr_knn.hip), which is then smoothed.  Departures: the voxels stand in ascending key
order (Open3D's order is its hash map's and unspecified; it decides only which of two equidistant centres comes first); the
vertices enter the keys and the search rounded to f32 (Open3D bins the f64 vertices); the weights are f64 (the reference's
are f32).  No observed vertex raises ValueError (the reference crashes in Open3D).  save_inter raises ValueError.  An
isolated vertex (no neighbours) keeps its move through propagation and becomes NaN in smoothing, as np.average of an empty
selection makes it; the reference raises IndexError there (its empty neighbour list is a float array).
"""
from __future__ import annotations

import ctypes
import json
import os
import threading
from concurrent.futures import ThreadPoolExecutor
from dataclasses import asdict, dataclass
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _host, _lib, _meshargs as _ma, _rig, formats, sweep
from ._lib import ptr as _p

PROP_SWEEPS = 20     # mesh_vert_propagate(max_ite=20) (warp_mesh.py:384, :133)
SMOOTH_SWEEPS = 5    # mesh_color_smoothing(ite_num=5) (:394)
FLOW_DIRS = {1: "flow_bi", 2: "flow_bi_2f", 4: "flow_bi_4f", 6: "flow_bi_6f"}    # :242-251
MAX_PREFETCH_THREADS = 8


@dataclass
class WarpConfig:
    """warp_config (warp_mesh.py:14-25): fields and defaults of the reference."""
    min_observe: int = 4
    depth_edge_ker_size: int = 7
    knn_K: int = 8
    cmr_view_max_cos: float = -0.5
    max_move_dist: float = 0.2
    voxel_size: float = 0.04
    bi_direct_pix_threshold: float = 4
    bi_direct_depth_threshold: float = 0.004
    edge_scalar: float = 10000
    edge_threshold: float = 0.1
    post_processing: str = "mesh"

    def save_cfg(self, dir: str) -> None:
        """The reference's config.json: every field, sorted keys, indent 4 (:27-45)."""
        text = json.dumps(asdict(self), sort_keys=True, indent=4, separators=(",", ": "))
        with open(os.path.join(dir, "config.json"), "w") as fh:
            fh.write(text)

    def params(self):
        """The [host] parameter block of gsr_warp_view."""
        return (ctypes.c_double * 6)(float(self.cmr_view_max_cos), float(self.edge_scalar), float(self.edge_threshold),
                                     float(self.bi_direct_depth_threshold), float(self.bi_direct_pix_threshold),
                                     float(self.max_move_dist))


@dataclass
class MeshWarp:
    """move_raw [V,3] f64: the rig mean after outlier removal, 0 where count < min_observe (warp_{f:04d}.obj);
    move_propagated (warp_mesh_prop.obj) and move_smoothed (warp_smooth.obj) [V,3] f64; verts_raw / verts_propagated /
    verts_smoothed = verts + the move; observed [V] int32: cameras that see the vertex; count [V] int32: after outlier
    removal (the one :384 uses).  With return_stages: table [C,V,3] f64 (NaN = not visible) and normals [V,3] f64.
    post_processing = 'voxel': move_voxel / verts_voxel [V,3] f64 (warp_voxel.obj) is what gets smoothed, and
    move_propagated / verts_propagated are None; in 'mesh' mode move_voxel / verts_voxel are None."""
    move_raw: torch.Tensor
    move_propagated: Optional[torch.Tensor]
    move_smoothed: torch.Tensor
    verts_raw: torch.Tensor
    verts_propagated: Optional[torch.Tensor]
    verts_smoothed: torch.Tensor
    observed: torch.Tensor
    count: torch.Tensor
    table: Optional[torch.Tensor] = None
    normals: Optional[torch.Tensor] = None
    move_voxel: Optional[torch.Tensor] = None
    verts_voxel: Optional[torch.Tensor] = None


def vertex_face_csr(topo):
    """meshes.MeshTopology.vertex_face_csr: (offsets [V+1], entries [3F]) int32, built once per MeshTopology."""
    return topo.vertex_face_csr


def _pad6(flow: torch.Tensor, pad):
    p = (0, 0, 0, 0) if pad is None else tuple(int(x) for x in np.int32(np.asarray(pad, np.float64)).reshape(-1))
    if len(p) != 4:
        raise ValueError(f"pad must be (top, bottom, left, right), got {pad!r}")
    return (ctypes.c_int * 6)(int(flow.shape[0]), int(flow.shape[1]), *p)


@torch.no_grad()
def warp_mesh(verts, faces, rig: dict, frames: Callable[[int], tuple], cfg: WarpConfig = WarpConfig(), pad=None,
              views_in_flight: int = 2, rank: Optional[int] = None, world: Optional[int] = None,
              return_stages: bool = False, device=None) -> MeshWarp:
    """warp_mesh_using_flow's computation (warp_mesh.py:259-397) for the mesh (verts [V,3], faces [F,3]; numpy or torch) seen
    by the cameras of `rig` (the `cmr` dict, _rig.py).  frames(i) -> (flow_f, flow_b, depth_cur, depth_next) for camera i, on
    any device: the raw RAFT flows [h,w,2] in (x, y) order and the depth maps [H,W] of frames f and f + interval; called once
    per camera of this rank's shard.  pad: (top, bottom, left, right) of the flows (pad.txt), or None."""
    if cfg.post_processing not in ("mesh", "voxel"):
        raise ValueError(f"warp_mesh: post_processing={cfg.post_processing!r} is not implemented (only 'mesh' and 'voxel')")
    lib = _lib.load()
    rig = _rig.Rig.of(rig)
    dev = _host.resolve_device(device, verts, what="warp_mesh")
    from . import meshes
    v = _ma.verts_on(verts, dev)
    V = int(v.shape[0])
    # (upload passes a long tensor on `dev` through: MeshTopology.of caches on a faces tensor that is passed again)
    topo = meshes.MeshTopology.of(_ma.upload(faces, dev, torch.long), V)
    f, F = topo.faces, topo.F
    C = rig.C
    fbuf = torch.empty(max(F, 1), 6, dtype=torch.float64, device=dev)
    normals = torch.empty(V, 3, dtype=torch.float64, device=dev)

    # ---- per camera: one row [V,3] of the table
    mine = sweep.camera_shard(C, rank, world)
    local = torch.empty(len(mine), 3 * V, dtype=torch.float64, device=dev)
    ws_bytes = int(lib.gsr_warp_view_workspace_bytes(1, 1))
    params = cfg.params()

    def to_dev(x, name, i):
        t = torch.as_tensor(x) if not isinstance(x, torch.Tensor) else x
        if name.startswith("depth") and t.dim() == 3:
            t = t[..., 0]
        return t.to(device=dev, dtype=torch.float32).contiguous()

    def per_camera(j, i):
        ff, fb, dc, dn = (to_dev(x, n, i) for x, n in zip(frames(i), ("flow_f", "flow_b", "depth_cur", "depth_next")))
        H, W = rig.hw(i)
        if tuple(dc.shape) != (H, W) or tuple(dn.shape) != (H, W):
            raise ValueError(f"camera {i}: depth {tuple(dc.shape)} / {tuple(dn.shape)} vs rig shape {(H, W)}")
        if ff.dim() != 3 or ff.shape[2] != 2 or ff.shape != fb.shape:
            raise ValueError(f"camera {i}: flows must be [h,w,2] of one shape, got {tuple(ff.shape)} / {tuple(fb.shape)}")
        ws = torch.empty(ws_bytes, dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_warp_view(H, W, V, _p(v), _p(normals), _p(ff), _p(fb), _pad6(ff, pad), _p(dc), _p(dn),
                                     rig.cam14(i), params, _p(ws), _p(local[j]),
                                     _host.stream_of(v)), "gsr_warp_view")

    with _host.on_device(v.device):
        # ---- once per warp: world-space vertex normals
        vf_off, vf_ent = topo.vertex_face_csr
        _lib.check(lib.gsr_vertex_normals(V, F, _p(v), _p(f), _p(vf_off), _p(vf_ent), _p(fbuf), _p(normals), _host.stream_of(v)),
                   "gsr_vertex_normals")
        sweep.run_cameras(mine, per_camera, views_in_flight, dev)
        table = sweep.gather_rows(local, C, rank, world)

        # ---- over the rig (every rank, same table, same bits)
        stream = _host.stream_of(v)
        move = torch.empty(V, 3, dtype=torch.float64, device=dev)
        observed = torch.empty(V, dtype=torch.int32, device=dev)
        count = torch.empty(V, dtype=torch.int32, device=dev)
        valid = torch.empty(V, dtype=torch.uint8, device=dev)
        _lib.check(lib.gsr_warp_aggregate(C, V, _p(table.contiguous()), int(cfg.min_observe), _p(move), _p(observed), _p(count),
                                          _p(valid), stream), "gsr_warp_aggregate")
        off, nbr = topo.vertex_neighbours
        prop = vox = None
        if cfg.post_processing == "voxel":
            vox = _voxel_interpolate(lib, v, move, valid, cfg, stream)
        else:
            # propagation: the valid set evolves independently of the values, so one scalar call per component is the vector result
            comp = move.t().contiguous()
            prop_c = torch.empty_like(comp)
            tmp = torch.empty(V, dtype=torch.float64, device=dev)
            va, vb = torch.empty_like(valid), torch.empty_like(valid)
            for k in range(3):
                _lib.check(lib.gsr_topo_propagate(V, _p(off), _p(nbr), PROP_SWEEPS, _p(comp[k]), _p(valid), _p(prop_c[k]), _p(tmp),
                                                  _p(va), _p(vb), stream), "gsr_topo_propagate")
            prop = prop_c.t().contiguous()
        pre = vox if prop is None else prop
        smooth = torch.empty_like(pre)
        stmp = torch.empty_like(pre)
        _lib.check(lib.gsr_warp_smooth(V, _p(off), _p(nbr), SMOOTH_SWEEPS, _p(pre), _p(smooth), _p(stmp), stream), "gsr_warp_smooth")
        res = MeshWarp(move_raw=move, move_propagated=prop, move_smoothed=smooth, verts_raw=v + move,
                       verts_propagated=None if prop is None else v + prop, verts_smoothed=v + smooth, observed=observed, count=count,
                       move_voxel=vox, verts_voxel=None if vox is None else v + vox)
        if return_stages:
            res.table, res.normals = table.view(C, V, 3), normals
        torch.cuda.current_stream().synchronize()
    return res


VOXEL_BITS = 21      # gsr_topo_voxel_keys: voxel index bits per axis of a key


def _voxel_interpolate(lib, v, move, valid, cfg: WarpConfig, stream) -> torch.Tensor:
    """warp_mesh.py:368-371: build_voxel_from_pc over the observed vertices and interpolate_in_voxel for every vertex ->
    [V,3] f64.  Reads the device twice (the observed vertices, the number of voxels)."""
    from . import knn
    vs = float(cfg.voxel_size)
    sel = torch.nonzero(valid).reshape(-1)
    n = int(sel.shape[0])
    if n == 0:
        raise ValueError("warp_mesh: post_processing='voxel' found no vertex seen by min_observe cameras: there is no voxel")
    v32 = v.float().contiguous()
    pts = v32[sel].contiguous()
    vmin, skeys, order, vid, head, flags = knn.voxel_groups(lib, pts, vs, stream)
    n_vox, overflow = (int(x) for x in torch.stack([vid[-1] + 1, flags[0].long()]).cpu())
    if overflow:
        raise ValueError(f"the observed vertices span more than 2^{VOXEL_BITS} voxels of {vs} along an axis")
    vox_move, _ = knn.segment_mean(vid, order, move[sel].contiguous(), n_vox)
    ukeys = skeys[head]
    mask = (1 << VOXEL_BITS) - 1
    index = torch.stack([ukeys >> (2 * VOXEL_BITS), (ukeys >> VOXEL_BITS) & mask, ukeys & mask], 1).double()
    centre = ((vmin.double() - vs * 0.5) + (index + 0.5) * vs).float().contiguous()
    idx, d2, _ = knn._search(v32, centre, int(cfg.knn_K), False, True, False)
    return knn.weighted_mean(idx, d2, vox_move, 1.0 / (vs * vs))


class _Prefetch:
    """Loads frames(i) for the cameras in `order` on a bounded thread pool, at most `depth` cameras ahead of the consumer, so
    that npz decompression overlaps the GPU."""

    def __init__(self, load: Callable[[int], tuple], order: Sequence[int], threads: int, depth: int):
        self.load, self.order, self.depth = load, list(order), depth
        self.pool = ThreadPoolExecutor(max_workers=threads)
        self.futures = {}
        self.next = 0
        self.lock = threading.Lock()

    def _fill(self, upto: int):
        while self.next < len(self.order) and self.next <= upto:
            i = self.order[self.next]
            self.futures[i] = self.pool.submit(self.load, i)
            self.next += 1

    def __call__(self, i: int):
        with self.lock:
            pos = self.order.index(i)
            self._fill(pos + self.depth)
            fut = self.futures.pop(i)
        return fut.result()

    def close(self):
        self.pool.shutdown(wait=True, cancel_futures=True)


def warp_mesh_using_flow(mesh_path, data_root, work_root, f_idx, interval=1, cmr=None, save_inter=False, from_humanrf=False,
                         views_in_flight: int = 2, prefetch_threads: int = MAX_PREFETCH_THREADS,
                         cfg: Optional[WarpConfig] = None) -> MeshWarp:
    """warp_mesh.py:216-401 with the reference's signature, files and errors.  Paths are joined by concatenation as in the
    reference (data_root and work_root end with '/').  Reads rgb_cameras.npz (unless cmr is given), the mesh (OBJ, vertex
    order kept), {f:04d}/{flow_dir}/pad.txt and {c:04d}_{f,b}.npz ('flow'), {f:04d}/depth[_humanrf]/img_{c:04d}_depth.npz and
    the same for f + interval ('depth').  Writes config.json, warp_{f:04d}.obj, warp_mesh_prop.obj and warp_smooth.obj
    under {f+interval:04d}/coarse_mesh/ (the last two with the input's vertex colours).  Every input is checked before the
    first launch.  save_inter=True raises ValueError.  cfg: the warp_config to use (the reference builds its default inside
    the function); with cfg.post_processing = 'voxel' warp_voxel.obj is written instead of warp_mesh_prop.obj (:373-376)."""
    if save_inter:
        raise ValueError("warp_mesh_using_flow: save_inter=True is not implemented")
    rig, _info = _rig.Rig.load(data_root + "rgb_cameras.npz" if cmr is None else cmr)
    C = rig.C
    cfg = WarpConfig() if cfg is None else cfg
    out_dir = work_root + f"{(f_idx + interval):04d}/coarse_mesh/"
    os.makedirs(out_dir, exist_ok=True)
    cfg.save_cfg(out_dir)
    verts, faces, colours = formats.load_obj(mesh_path)
    if interval not in FLOW_DIRS:
        raise RuntimeError("Interval Error!")
    flow_dir = data_root + f"{f_idx:04d}/{FLOW_DIRS[interval]}/"
    label = "_humanrf" if from_humanrf else ""
    pad_path = flow_dir + "pad.txt"
    pad = np.int32(np.loadtxt(pad_path)) if os.path.exists(pad_path) else None
    for c in range(C):
        if not os.path.exists(flow_dir + f"{c:04d}_f.npz"):
            raise RuntimeError("Flow not found!")
        if not os.path.exists(data_root + f"{f_idx:04d}/depth{label}/img_{c:04d}_depth.npz"):
            raise RuntimeError("Depth not found!")

    def load(c):
        ff = np.load(flow_dir + f"{c:04d}_f.npz")["flow"]
        fb = np.load(flow_dir + f"{c:04d}_b.npz")["flow"]
        dc = np.load(data_root + f"{f_idx:04d}/depth{label}/img_{c:04d}_depth.npz")["depth"]
        dn = np.load(data_root + f"{(f_idx + interval):04d}/depth{label}/img_{c:04d}_depth.npz")["depth"]
        return tuple(torch.from_numpy(np.ascontiguousarray(x, np.float32)).pin_memory() for x in (ff, fb, dc, dn))

    mine = sweep.camera_shard(C)
    threads = max(1, min(MAX_PREFETCH_THREADS, int(prefetch_threads), len(mine)))
    pre = _Prefetch(load, mine, threads, depth=threads + max(1, int(views_in_flight)))   # (each camera pins ~40 MB at 1080p)
    try:
        res = warp_mesh(verts, faces, rig, pre, cfg, pad=pad, views_in_flight=views_in_flight)
    finally:
        pre.close()
    formats.save_obj(out_dir + f"warp_{f_idx:04d}.obj", res.verts_raw.cpu().numpy(), faces)
    if res.verts_voxel is not None:
        formats.save_obj(out_dir + "warp_voxel.obj", res.verts_voxel.cpu().numpy(), faces, colours)
    else:
        formats.save_obj(out_dir + "warp_mesh_prop.obj", res.verts_propagated.cpu().numpy(), faces, colours)
    formats.save_obj(out_dir + "warp_smooth.obj", res.verts_smoothed.cpu().numpy(), faces, colours)
    return res


__all__ = ["WarpConfig", "MeshWarp", "warp_mesh", "warp_mesh_using_flow", "vertex_face_csr"]
