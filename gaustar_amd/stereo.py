"""Plane-sweep stereo behind a depth prior on the GPU: the photo-consistency refinement of the visual hull.

gaustar_amd.hull makes a sequence's meshes from the masks alone, and a hull closes over every concavity: depth rendered from it
is too near there, and the depth loss pulls the Gaussians outward by as much.  The rig also has a calibrated, rectified colour
image per camera, and the hull bounds the surface from outside: the true depth along a ray is at or behind the hull's.  So per
reference camera a short band of planes behind the prior is swept and scored against a few neighbouring cameras:

    lumas = [luma(img) for img in images]                       # [H,W] uint8: (77 R + 150 G + 29 B + 128) >> 8
    sources = select_sources(rig, 4)                            # [C,S] int32: neighbours by the angle at the subject, -1 = none
    view = sweep_view(rig, r, sources[r], lumas, prior, cfg)    # StereoView(depth, score, state, plane) of camera r
    views = sweep_rig(rig, images, priors, sources, cfg)        # every camera, the lumas resident, two views in flight
    views = check_consistency(rig, views, sources, cfg)         # state 3 -> 4 where enough sources agree
    merged = merge_volumes(hull_volume, stereo_volume)          # the hull's TSDF carved by the fused stereo depth
    verts, faces, info = refine_hull(rig, images, masks)        # all of it: hull, priors, sweep, consistency, fusion, merge, mesh
    write_stereo_meshes(gstar_dir, gstar_dir, capture, mesh_dir, 0, 10, 1)   # the names write_hull_meshes writes

The rules are stated in include/gsr.h and restated in tests/stereo_ref.py; the device agrees with the restatement bit for bit.
state per pixel: 0 not covered by the prior, 1 covered but no plane had enough valid sources, 2 the best cost stayed below
min_score, 3 accepted, 4 accepted and met by its sources' depths.  depth keeps the prior's bits below state 3.

What to know about the result:
  * textureless and specular regions keep the hull: a window whose variance is below min_var scores nothing, a cost below
    min_score is not accepted, and a depth its neighbours do not meet does not reach the volume;
  * where stereo data ends the surface steps back to the hull within a voxel or two: the merged TSDF is the hull's there;
  * a window that crosses the silhouette is rejected as soon as its taps leave a source image, and scores badly otherwise:
    the rim of the subject keeps the hull;
  * exposure differences between cameras are handled by the normalisation of the correlation only;
  * one rank only: the consistency pass needs the neighbours' maps, and a sharded form has not been built.
"""
from __future__ import annotations

import os
from dataclasses import dataclass, replace
from typing import Callable, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _host, _lib, _rig, formats, fusion, hull, mesh_depth, sweep
from ._lib import ptr as _p
from ._meshargs import tensor_of

ZNEAR = 0.01
MAX_SOURCES = 8
MAX_BAND = 4096
CAMERA_DTYPE = np.dtype([("R", "<f8", (9,)), ("t", "<f8", (3,)), ("fx", "<f8"), ("fy", "<f8"), ("cx", "<f8"), ("cy", "<f8"),
                         ("image", "<u8"), ("state", "<u8"), ("H", "<i4"), ("W", "<i4")])      # gsr_stereo.hip's StereoCamera
_RIG_CHECKS = dict(min_side=2, finite=True, positive_focal=True)


class StereoView(NamedTuple):
    """depth [H,W] f32, score [H,W] f32 (-2 = none), state [H,W] uint8, plane [H,W] int16 (-1 = none), on the device."""
    depth: torch.Tensor
    score: torch.Tensor
    state: torch.Tensor
    plane: torch.Tensor


@dataclass(frozen=True)
class StereoConfig:
    """The knobs of the sweep and of the consistency pass.  step: the distance between planes; the band of a pixel with prior
    depth d is [d - near, d + far]; a prior at or beyond `background` (or at or before znear = 0.01) is not covered; radius:
    the window is (2 radius + 1)^2; min_var: the least variance of a window, in grey levels squared; a plane needs min_sources
    valid sources and costs the mean of its `keep` best scores (None: max(1, S // 2)); min_score: the least cost that is
    accepted; tol (None: 2 step) and min_consistent: the consistency pass."""
    step: float = 0.004
    near: float = 0.008
    far: float = 0.12
    background: float = 50.0
    radius: int = 3
    min_var: float = 4.0
    min_sources: int = 2
    keep: Optional[int] = None
    min_score: float = 0.6
    tol: Optional[float] = None
    min_consistent: int = 2

    def resolved(self, S: int) -> "StereoConfig":
        """The config with keep and tol filled in for S sources, checked.  ValueError: a knob outside its range."""
        S = int(S)
        if not 1 <= S <= MAX_SOURCES:
            raise ValueError(f"between 1 and {MAX_SOURCES} sources, got {S}")
        vals = [self.step, self.near, self.far, self.background, self.min_var, self.min_score]
        if not all(np.isfinite(float(v)) for v in vals):
            raise ValueError("the stereo parameters must be finite")
        if not self.step > 0:
            raise ValueError("step must be positive")
        if self.near < 0 or self.far < 0:
            raise ValueError("near and far must not be negative")
        if not (self.near + self.far) / self.step <= MAX_BAND:
            raise ValueError(f"(near + far) / step must be at most {MAX_BAND}")
        if not self.background > ZNEAR:
            raise ValueError("background must be beyond znear")
        if not (self.background + self.far) / self.step < 32768.0:
            raise ValueError("the farthest plane index, floor((background + far) / step), must fit int16: raise step or lower background")
        if int(self.radius) not in (1, 2, 3):
            raise ValueError("radius must be 1, 2 or 3")
        if not self.min_var > 0:
            raise ValueError("min_var must be positive")
        if not 1 <= int(self.min_sources) <= S:
            raise ValueError(f"min_sources must be between 1 and the number of sources ({S})")
        keep = max(1, S // 2) if self.keep is None else int(self.keep)
        if not 1 <= keep <= S:
            raise ValueError(f"keep must be between 1 and the number of sources ({S})")
        tol = 2.0 * float(self.step) if self.tol is None else float(self.tol)
        if not (tol > 0 and np.isfinite(tol)):
            raise ValueError("tol must be positive")
        if not 1 <= int(self.min_consistent) <= S:
            raise ValueError(f"min_consistent must be between 1 and the number of sources ({S})")
        return replace(self, keep=keep, tol=tol)


def _rig_of(rig) -> _rig.Rig:
    rig = _rig.Rig.of(rig, **_RIG_CHECKS)
    if not rig.C:
        raise ValueError("the rig has no camera")
    return rig


# ------------------------------------------------------------------------------------------------ luma
@torch.no_grad()
def luma(image, device=None) -> torch.Tensor:
    """image [H,W,3] uint8 RGB (numpy, or a torch tensor, which must be on a GPU) -> [H,W] uint8 on the device,
    Y = (77 R + 150 G + 29 B + 128) >> 8; an [H,W] uint8 image is taken as luma already.  Runs on the current stream without a
    host read.  ValueError: another dtype or shape, a CPU tensor."""
    if isinstance(image, torch.Tensor):
        t = image
        if t.dtype != torch.uint8 or t.dim() not in (2, 3) or (t.dim() == 3 and t.shape[2] != 3) or 0 in t.shape:
            raise ValueError(f"image must be [H,W,3] or [H,W] uint8, got {t.dtype} {tuple(t.shape)}")
        if not t.is_cuda:
            raise ValueError("a torch image must be on a GPU (pass numpy for host data)")
        t = t.contiguous()
    else:
        a = np.asarray(image)
        if a.dtype != np.uint8 or a.ndim not in (2, 3) or (a.ndim == 3 and a.shape[2] != 3) or 0 in a.shape:
            raise ValueError(f"image must be [H,W,3] or [H,W] uint8, got {a.dtype} {a.shape}")
        t = torch.from_numpy(np.ascontiguousarray(a)).to(_host.resolve_device(device, what="gaustar_amd.stereo"))
    if t.dim() == 2:
        return t
    H, W = int(t.shape[0]), int(t.shape[1])
    with _host.on_device(t.device):
        out = torch.empty(H, W, dtype=torch.uint8, device=t.device)
        _lib.check(_lib.load().gsr_stereo_luma(H, W, _p(t), _p(out), _host.stream_of(t)), "gsr_stereo_luma")
    return out


# ------------------------------------------------------------------------------------------------ sources and poses
def camera_centres(rig) -> np.ndarray:
    """[C,3] f64: -R^T t per camera."""
    extr = _rig_of(rig).extr
    return -np.einsum("cji,cj->ci", extr[:, :3, :3], extr[:, :3, 3])


def select_sources(rig, n_sources: int = 4, min_angle_deg: float = 5.0, max_angle_deg: float = 40.0, focus=None) -> np.ndarray:
    """[C,S] int32: per camera r the S = n_sources other cameras s with the smallest angle at `focus` (default: the centre of
    hull.rig_box) between the two camera centres, among those whose angle lies in [min_angle_deg, max_angle_deg]; sorted by
    (angle, index), padded with -1.  Host only.  ValueError: n_sources outside [1, 8], an empty or reversed angle range."""
    rig = _rig_of(rig)
    S = int(n_sources)
    if not 1 <= S <= MAX_SOURCES:
        raise ValueError(f"n_sources must be between 1 and {MAX_SOURCES}, got {n_sources}")
    if not 0 <= float(min_angle_deg) <= float(max_angle_deg) <= 180:
        raise ValueError("need 0 <= min_angle_deg <= max_angle_deg <= 180")
    if focus is None:
        lo, hi = hull.rig_box(rig)
        focus = 0.5 * (lo + hi)
    rays = camera_centres(rig) - np.asarray(focus, np.float64).reshape(1, 3)
    with np.errstate(all="ignore"):
        rays = rays / np.linalg.norm(rays, axis=1, keepdims=True)
        angle = np.degrees(np.arccos(np.clip(rays @ rays.T, -1.0, 1.0)))        # NaN for a camera at the focus: never chosen
    out = np.full((rig.C, S), -1, np.int32)
    for r in range(rig.C):
        cand = [(float(angle[r, s]), s) for s in range(rig.C) if s != r and float(min_angle_deg) <= angle[r, s] <= float(max_angle_deg)]
        cand.sort()
        for j, (_a, s) in enumerate(cand[:S]):
            out[r, j] = s
    return out


def relative_pose(rig, r: int, s: int) -> Tuple[np.ndarray, np.ndarray]:
    """(R_sr [3,3], t_sr [3]) f64 with x_s = R_sr x_r + t_sr: R_sr = R_s R_r^T, t_sr = t_s - R_sr t_r, each element three
    products added as (a + b) + c in double -- no matmul call, so that the device and tests/stereo_ref.py read the same bits."""
    rig = _rig_of(rig)
    Rr, tr = rig.extr[r][:3, :3].tolist(), rig.extr[r][:3, 3].tolist()
    Rs, ts = rig.extr[s][:3, :3].tolist(), rig.extr[s][:3, 3].tolist()
    R = [[(Rs[i][0] * Rr[j][0] + Rs[i][1] * Rr[j][1]) + Rs[i][2] * Rr[j][2] for j in range(3)] for i in range(3)]
    t = [ts[i] - ((R[i][0] * tr[0] + R[i][1] * tr[1]) + R[i][2] * tr[2]) for i in range(3)]
    return np.array(R, np.float64), np.array(t, np.float64)


def _sources_of(row, C: int, r: int) -> List[int]:
    """A row of a sources table without its -1 padding, checked."""
    row = np.asarray(row)
    if row.ndim != 1 or not np.issubdtype(row.dtype, np.integer):
        raise ValueError("a sources row must be a 1-D integer array")
    srcs = [int(s) for s in row if int(s) != -1]
    if not 1 <= len(srcs) <= MAX_SOURCES:
        raise ValueError(f"camera {r} needs between 1 and {MAX_SOURCES} sources, got {len(srcs)}")
    for s in srcs:
        if not 0 <= s < C:
            raise ValueError(f"camera {r}: source index {s} outside the rig's {C} cameras")
        if s == r:
            raise ValueError(f"camera {r} is listed as its own source")
    return srcs


def _check_map(x, hw, dtype, dev, what: str) -> torch.Tensor:
    if not isinstance(x, torch.Tensor) or x.dtype != dtype or tuple(x.shape) != tuple(hw):
        got = f"{x.dtype} {tuple(x.shape)}" if isinstance(x, torch.Tensor) else type(x).__name__
        raise ValueError(f"{what} must be a {tuple(hw)} {dtype} tensor, got {got}")
    if not x.is_cuda or (dev is not None and x.device != dev):
        raise ValueError(f"{what} must be on {'a GPU' if dev is None else dev}, got {x.device}")
    return x.contiguous()


def _ref_cam(rig: _rig.Rig, r: int, use_principal_point: bool):
    cx, cy = rig.principal(r, use_principal_point)
    return (_lib.c_double * 4)(float(rig.intr[r][0, 0]), float(rig.intr[r][1, 1]), float(cx), float(cy))


def _table(rig: _rig.Rig, r: int, srcs: Sequence[int], images: Sequence[torch.Tensor], states, use_principal_point: bool) -> np.ndarray:
    table = np.zeros(len(srcs), CAMERA_DTYPE)
    for j, s in enumerate(srcs):
        R, t = relative_pose(rig, r, s)
        cx, cy = rig.principal(s, use_principal_point)
        H, W = rig.hw(s)
        table[j] = (R.reshape(-1), t, float(rig.intr[s][0, 0]), float(rig.intr[s][1, 1]), float(cx), float(cy), images[j].data_ptr(),
                    0 if states is None else states[j].data_ptr(), H, W)
    return table


# ------------------------------------------------------------------------------------------------ the sweep
@torch.no_grad()
def sweep_view(rig, r: int, sources_row, lumas, prior_depth, cfg: Optional[StereoConfig] = None,
               use_principal_point: bool = False) -> StereoView:
    """Camera r of the rig swept against the cameras of sources_row (indices into the rig; -1 entries are padding).  lumas:
    indexable by camera, [H_i,W_i] uint8 tensors on one GPU (luma()'s; only r's and the sources' are read); prior_depth
    [H_r,W_r] f32 on that GPU, e.g. mesh_depth's render of the hull (its background of 100 is not covered).  Runs on the
    current stream without a host read.  ValueError before any launch: a source out of range or equal to r, no source or more
    than 8, wrong dtypes, shapes or devices, a knob of cfg outside its range."""
    rig = _rig_of(rig)
    r = int(r)
    if not 0 <= r < rig.C:
        raise ValueError(f"camera {r} outside the rig's {rig.C} cameras")
    srcs = _sources_of(sources_row, rig.C, r)
    cfg = (StereoConfig() if cfg is None else cfg).resolved(len(srcs))
    ref = _check_map(lumas[r], rig.hw(r), torch.uint8, None, f"luma {r}")
    dev = ref.device
    imgs = [_check_map(lumas[s], rig.hw(s), torch.uint8, dev, f"luma {s}") for s in srcs]
    prior = _check_map(prior_depth, rig.hw(r), torch.float32, dev, "prior_depth")
    H, W = rig.hw(r)
    lib = _lib.load()
    table = _table(rig, r, srcs, imgs, None, use_principal_point)
    params = (_lib.c_double * 6)(cfg.step, cfg.near, cfg.far, cfg.background, cfg.min_var, cfg.min_score)
    with _host.on_device(dev):
        out = StereoView(torch.empty(H, W, dtype=torch.float32, device=dev), torch.empty(H, W, dtype=torch.float32, device=dev),
                         torch.empty(H, W, dtype=torch.uint8, device=dev), torch.empty(H, W, dtype=torch.int16, device=dev))
        cams = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
        _lib.check(lib.gsr_stereo_sweep(H, W, _p(ref), _p(prior), _ref_cam(rig, r, use_principal_point), len(srcs), table.ctypes.data,
                                        _p(cams), params, int(cfg.radius), int(cfg.min_sources), int(cfg.keep), _p(out.depth),
                                        _p(out.score), _p(out.state), _p(out.plane), _host.stream_of(ref)), "gsr_stereo_sweep")
    return out


def _image_of(src, i: int, hw, dev, what: str = "image") -> torch.Tensor:
    """Camera i's colour or grey image of `src` (list, stack or callable), checked, contiguous on dev."""
    t = tensor_of(src(i) if callable(src) else src[i])
    return _rig.fetch_image(lambda _i: t, i, hw, (3,) if t.dim() == 3 else (), (torch.uint8,), dev, what)


def _check_sources(sources, rig: _rig.Rig) -> np.ndarray:
    sources = np.asarray(sources)
    if sources.ndim != 2 or sources.shape[0] != rig.C or not np.issubdtype(sources.dtype, np.integer):
        raise ValueError(f"sources must be an integer array [C,S] with one row per camera of the rig ({rig.C})")
    return sources


@torch.no_grad()
def sweep_rig(rig, images, prior_depths, sources=None, cfg: Optional[StereoConfig] = None, views_in_flight: int = 2, *,
              use_principal_point: bool = False, device=None) -> List[StereoView]:
    """Every camera of the rig swept against its row of `sources` (default: select_sources(rig)).  images: one [H,W,3] or [H,W]
    uint8 image per camera, as a list (shapes may differ), a stack or a callable i -> image; prior_depths: one [H,W] f32 map
    per camera, likewise.  The lumas of the whole rig are made first and stay resident (160 cameras of 1080p: 330 MB); then
    the cameras run `views_in_flight` at a time on as many streams (sweep.run_cameras).  The result does not depend on
    views_in_flight.  One rank: every camera's view is needed by check_consistency.  Returns the views in camera order."""
    rig = _rig_of(rig)
    if not callable(images):
        first = images[0] if hasattr(images, "__len__") and len(images) else None
        tail = (3,) if first is not None and getattr(first, "ndim", 2) == 3 else ()
        _rig.check_images(images, rig, tail, (torch.uint8,), "image", on_gpu=True)
    _rig.check_images(prior_depths, rig, (), (torch.float32,), "prior depth", on_gpu=True)
    sources = _check_sources(select_sources(rig) if sources is None else sources, rig)
    rows = [_sources_of(sources[r], rig.C, r) for r in range(rig.C)]
    for row in rows:
        (StereoConfig() if cfg is None else cfg).resolved(len(row))
    dev = _host.resolve_device(device, what="gaustar_amd.stereo")
    everyone = list(range(rig.C))
    lumas: List[Optional[torch.Tensor]] = [None] * rig.C
    priors: List[Optional[torch.Tensor]] = [None] * rig.C
    views: List[Optional[StereoView]] = [None] * rig.C

    def make_luma(_j, i):
        lumas[i] = luma(_image_of(images, i, rig.hw(i), dev))
        priors[i] = _rig.fetch_image(prior_depths, i, rig.hw(i), (), (torch.float32,), dev, "prior depth")

    def per_camera(_j, i):
        views[i] = sweep_view(rig, i, rows[i], lumas, priors[i], cfg, use_principal_point)

    sweep.run_cameras(everyone, make_luma, views_in_flight, dev)
    sweep.run_cameras(everyone, per_camera, views_in_flight, dev)
    return views


# ------------------------------------------------------------------------------------------------ consistency
@torch.no_grad()
def check_consistency(rig, views: Sequence[StereoView], sources, cfg: Optional[StereoConfig] = None, *,
                      use_principal_point: bool = False) -> List[StereoView]:
    """The second pass, after all sweeps: a pixel of state 3 becomes state 4 iff at least cfg.min_consistent of its camera's
    sources agree -- the point at the refined depth lies beyond znear in the source, its nearest source pixel is on the image,
    has state >= 3 FROM THE SWEEP and a depth within cfg.tol (default 2 step) of the point's.  Reading the sweep's states
    keeps the result free of the order of the cameras.  Returns new views (depth, score and plane shared with the input)."""
    rig = _rig_of(rig)
    if not hasattr(views, "__len__") or len(views) != rig.C:
        raise ValueError(f"need one view per camera of the rig ({rig.C})")
    sources = _check_sources(sources, rig)
    rows = [_sources_of(sources[r], rig.C, r) for r in range(rig.C)]
    cfgs = [(StereoConfig() if cfg is None else cfg).resolved(len(row)) for row in rows]
    dev = None
    for i, v in enumerate(views):
        d = _check_map(v.depth, rig.hw(i), torch.float32, dev, f"depth {i}")
        dev = d.device
        _check_map(v.state, rig.hw(i), torch.uint8, dev, f"state {i}")
    lib = _lib.load()
    depths = [v.depth.contiguous() for v in views]
    states = [v.state.contiguous() for v in views]
    out = []
    with _host.on_device(dev):
        for r in range(rig.C):
            srcs, c = rows[r], cfgs[r]
            H, W = rig.hw(r)
            table = _table(rig, r, srcs, [depths[s] for s in srcs], [states[s] for s in srcs], use_principal_point)
            cams = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
            new = torch.empty(H, W, dtype=torch.uint8, device=dev)
            _lib.check(lib.gsr_stereo_consistency(H, W, _p(depths[r]), _p(states[r]), _ref_cam(rig, r, use_principal_point), len(srcs),
                                                  table.ctypes.data, _p(cams), float(c.tol), int(c.min_consistent), _p(new),
                                                  _host.stream_of(new)), "gsr_stereo_consistency")
            out.append(StereoView(views[r].depth, views[r].score, new, views[r].plane))
    return out


# ------------------------------------------------------------------------------------------------ merge
@torch.no_grad()
def merge_volumes(hull_volume: fusion.TSDFVolume, stereo_volume: fusion.TSDFVolume, min_weight: float = 3.0) -> fusion.TSDFVolume:
    """A finished hull volume carved by a fusion volume of the same grid (fusion.integrate_views of the consistent depths):
    tsdf = max(t_h, t_s) where w_s >= min_weight and w_h == 1, else t_h -- the hull bounds the surface from outside, so stereo
    can only carve; weight = w_h; color = the stereo volume's where w_s > 0, else 0; touched by hull.finish's rule.  Returns a
    new TSDFVolume that fusion.extract_triangle_mesh reads.  ValueError: volumes of different grids or devices."""
    a, b = hull_volume, stereo_volume
    if not isinstance(a, fusion.TSDFVolume) or not isinstance(b, fusion.TSDFVolume):
        raise ValueError("both volumes must be fusion.TSDFVolume (a hull.HullVolume is one)")
    if [int(v) for v in a.u0] != [int(v) for v in b.u0] or [int(v) for v in a.nu] != [int(v) for v in b.nu] or \
            a.voxel_size != b.voxel_size or a.sdf_trunc != b.sdf_trunc:
        raise ValueError("the volumes must share one grid, voxel size and truncation")
    if a.device != b.device:
        raise ValueError("the volumes must be on one device")
    if not (min_weight > 0 and np.isfinite(min_weight)):
        raise ValueError("min_weight must be positive")
    out = fusion.TSDFVolume.from_units(a.u0, a.nu, a.voxel_size, a.sdf_trunc, a.device)
    with _host.on_device(a.device):
        _lib.check(_lib.load().gsr_stereo_merge(a.grid, _p(a.tsdf), _p(a.weight), _p(b.tsdf), _p(b.weight), _p(b.color), float(min_weight),
                                                _p(out.tsdf), _p(out.weight), _p(out.color), _p(out.touched), _host.stream_of(out.tsdf)),
                   "gsr_stereo_merge")
    out.n_views = a.n_views
    return out


# ------------------------------------------------------------------------------------------------ the whole path
def _extr44(extr) -> np.ndarray:
    E = np.eye(4)
    E[:3] = np.asarray(extr, np.float64)[:3]
    return E


@torch.no_grad()
def refine_hull(rig, images, masks, lo=None, hi=None, voxel_size: float = 0.008, sdf_trunc: float = 0.02, min_views: Optional[int] = None,
                taubin_iterations: int = 10, target_faces: int = 100_000, *, sources=None, cfg: Optional[StereoConfig] = None,
                min_weight: float = 3.0, threshold: int = 128, views_in_flight: int = 2, use_principal_point: bool = False,
                coarse_voxel: float = 0.032, device=None):
    """The visual hull of the masks, refined by the colour images: (verts [V,3] f32, faces [F,3] int32, info).  In order:
    hull.hull_bounds (without lo / hi), HullVolume, carve_views, finish; the hull's mesh; mesh_depth.render_mesh_depth of it
    for the priors; sweep_rig; check_consistency; fusion.integrate_views of where(state == 4, depth, 0) and the colour image
    per camera into a second volume of the same grid; merge_volumes; fusion.extract_triangle_mesh; then hull_mesh's Taubin
    smoothing and decimation options.  info: `states` [C,5] int64, the per-camera counts of states 0 to 4 (one host read),
    `hull_faces` and `faces`, the face counts before and after the refinement (before smoothing and decimation).  One rank."""
    if int(taubin_iterations) < 0 or int(target_faces) < 0:
        raise ValueError("taubin_iterations and target_faces must not be negative")
    rig = _rig_of(rig)
    C = rig.C
    kw = dict(threshold=threshold, use_principal_point=use_principal_point)
    if lo is None or hi is None:
        lo, hi = hull.hull_bounds(rig, masks, lo, hi, coarse_voxel, min_views=min_views, views_in_flight=views_in_flight, device=device, **kw)
    vol = hull.HullVolume(lo, hi, voxel_size, sdf_trunc, device)
    dev = vol.device
    hull.carve_views(vol, rig, masks, views_in_flight, 0, 1, **kw)
    hull.finish(vol, hull.default_min_views(C) if min_views is None else min_views)
    hv, hf, _ = fusion.extract_triangle_mesh(vol)
    if not int(hf.shape[0]):
        raise ValueError("refine_hull: the hull is empty")
    priors: List[Optional[torch.Tensor]] = [None] * C

    def keep_depth(i, view):
        priors[i] = view.depth

    mesh_depth.render_mesh_depth(hv, hf, rig.as_dict(), keep_depth, use_principal_point=use_principal_point, views_in_flight=views_in_flight,
                                 rank=0, world=1, device=dev)
    if sources is None:
        sources = select_sources(rig)
    views = sweep_rig(rig, images, priors, sources, cfg, views_in_flight, use_principal_point=use_principal_point, device=dev)
    views = check_consistency(rig, views, sources, cfg, use_principal_point=use_principal_point)
    svol = fusion.TSDFVolume.from_units(vol.u0, vol.nu, voxel_size, sdf_trunc, dev)
    with _host.on_device(dev):
        for i, v in enumerate(views):
            img = _image_of(images, i, rig.hw(i), dev)
            rgb = img if img.dim() == 3 else img[:, :, None].expand(-1, -1, 3).contiguous()
            depth = torch.where(v.state == 4, v.depth, torch.zeros_like(v.depth))
            cx, cy = rig.principal(i, use_principal_point)
            fusion.integrate_views(svol, depth, rgb, (float(rig.intr[i][0, 0]), float(rig.intr[i][1, 1]), float(cx), float(cy)),
                                   _extr44(rig.extr[i]))
        merged = merge_volumes(vol, svol, min_weight)
        verts, faces, _colors = fusion.extract_triangle_mesh(merged)
        kinds = torch.arange(5, dtype=torch.uint8, device=dev)          # (torch.bincount would read the maximum back per camera)
        counts = torch.stack([(v.state.reshape(-1, 1) == kinds).sum(0) for v in views]).cpu().numpy()
    info = {"states": counts, "hull_faces": int(hf.shape[0]), "faces": int(faces.shape[0])}
    from . import remesh         # (here: remesh imports regions, which nothing else of this module needs)
    if int(taubin_iterations) > 0 and verts.shape[0]:
        verts = remesh.smooth_taubin(verts, faces, iterations=int(taubin_iterations))
    if int(target_faces) > 0 and faces.shape[0] > int(target_faces):
        small = remesh.simplify_mesh(verts, faces, int(target_faces))
        verts, faces = small.verts, small.faces
    return verts, faces, info


# ------------------------------------------------------------------------------------------------ files
def gstar_image_path(gstar_dir) -> Callable[[int, int], str]:
    """(camera index, frame) -> `{f:04d}/images/img_{c:04d}.png` under gstar_dir, where dataprep writes the rectified images."""
    root = os.fspath(gstar_dir)
    return lambda c, f: os.path.join(root, f"{f:04d}", "images", f"img_{c:04d}.png")


def write_stereo_meshes(gstar_dir, image_path: Union[str, os.PathLike, Callable[[int, int], str]],
                        mask_path: Union[str, os.PathLike, Callable[[int, int], str]], mesh_dir, frame_0: int = 0, frame_end: int = 0,
                        interval: int = 1, res: str = "100k", *, lo=None, hi=None, voxel_size: float = 0.008, sdf_trunc: float = 0.02,
                        min_views: Optional[int] = None, taubin_iterations: int = 10, target_faces: int = 100_000,
                        cfg: Optional[StereoConfig] = None, n_sources: int = 4, min_weight: float = 3.0, threshold: int = 128,
                        views_in_flight: int = 2, device=None) -> list:
    """Per frame f in range(frame_0, frame_end, interval): refine_hull of the frame's rectified images and masks, written to
    `mesh_{f:06d}_smooth_{res}.obj` under mesh_dir -- the names hull.write_hull_meshes writes, which
    mesh_depth.render_mesh_depth_files(from_humanrf=True) and dataprep.prepare_first_frame read unchanged.  gstar_dir must hold
    `rgb_cameras.npz`; image_path: a callable (camera index, frame) -> the rectified colour image (dataprep.load_image_rgb8), or
    the directory dataprep wrote them under (gstar_image_path); mask_path: as hull.write_hull_meshes takes it.  The principal
    point is (W / 2, H / 2).  Returns the paths written."""
    from . import dataprep
    rig = _rig.Rig.load(os.path.join(os.fspath(gstar_dir), "rgb_cameras.npz"), **_RIG_CHECKS)[0]
    image_of = image_path if callable(image_path) else gstar_image_path(image_path)
    mask_of = mask_path if callable(mask_path) else hull.actorshq_mask_path(mask_path)
    frames = list(range(int(frame_0), int(frame_end), int(interval)))
    if not frames:
        raise ValueError("no frame in range(frame_0, frame_end, interval)")
    sources = select_sources(rig, n_sources)
    os.makedirs(os.fspath(mesh_dir), exist_ok=True)
    out = []
    for f in frames:
        masks = [formats.load_png_gray8(mask_of(c, f)) for c in range(rig.C)]
        verts, faces, _info = refine_hull(rig, lambda c, f=f: dataprep.load_image_rgb8(image_of(c, f)), masks, lo, hi, voxel_size, sdf_trunc,
                                          min_views, taubin_iterations, target_faces, sources=sources, cfg=cfg, min_weight=min_weight,
                                          threshold=threshold, views_in_flight=views_in_flight, device=device)
        if not int(faces.shape[0]):
            raise ValueError(f"frame {f}: the refined hull is empty")
        path = os.path.join(os.fspath(mesh_dir), f"mesh_{f:06d}_smooth_{res}.obj")
        formats.save_obj(path, verts.cpu().numpy(), faces.cpu().numpy())
        out.append(path)
    return out


def main(argv=None) -> int:
    """python -m gaustar_amd.stereo GSTAR_DIR MASKS MESH_DIR --frame-0 A --frame-end B [--images DIR] [--interval K] ...: the
    hull meshes of a capture's frames, refined by plane-sweep stereo (write_stereo_meshes); MASKS is the capture's directory
    (masks/CamNNN/CamNNN_maskFFFFFF.png); the rectified images are read from GSTAR_DIR (FFFF/images/img_CCCC.png) or --images."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gaustar_amd.stereo", description=main.__doc__)
    ap.add_argument("gstar_dir")
    ap.add_argument("masks")
    ap.add_argument("mesh_dir")
    ap.add_argument("--images", default=None, help="where the rectified images are (default: GSTAR_DIR)")
    ap.add_argument("--frame-0", type=int, default=0)
    ap.add_argument("--frame-end", type=int, required=True)
    ap.add_argument("--interval", type=int, default=1)
    ap.add_argument("--res", default="100k")
    ap.add_argument("--voxel-size", type=float, default=0.008)
    ap.add_argument("--sdf-trunc", type=float, default=0.02)
    ap.add_argument("--min-views", type=int, default=None)
    ap.add_argument("--taubin", type=int, default=10, metavar="K", help="Taubin pairs (0 = off)")
    ap.add_argument("--faces", type=int, default=100_000, help="the face count to decimate to (0 = off)")
    ap.add_argument("--sources", type=int, default=4, help="source cameras per reference camera (1..8)")
    ap.add_argument("--step", type=float, default=0.004)
    ap.add_argument("--far", type=float, default=0.12)
    ap.add_argument("--radius", type=int, default=3)
    ap.add_argument("--min-score", type=float, default=0.6)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    cfg = StereoConfig(step=a.step, far=a.far, radius=a.radius, min_score=a.min_score)
    for p in write_stereo_meshes(a.gstar_dir, a.gstar_dir if a.images is None else a.images, a.masks, a.mesh_dir, a.frame_0, a.frame_end,
                                 a.interval, a.res, voxel_size=a.voxel_size, sdf_trunc=a.sdf_trunc, min_views=a.min_views,
                                 taubin_iterations=a.taubin, target_faces=a.faces, cfg=cfg, n_sources=a.sources, device=a.device):
        print(p)
    return 0


__all__ = ["luma", "select_sources", "relative_pose", "StereoConfig", "StereoView", "sweep_view", "sweep_rig", "check_consistency",
           "merge_volumes", "refine_hull", "write_stereo_meshes", "CAMERA_DTYPE"]

if __name__ == "__main__":
    raise SystemExit(main())
