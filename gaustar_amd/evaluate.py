"""How good a result is, measured on the device (include/gsr.h "Scoring a result", gsr_eval.hip): the exact distance from
points to a triangle mesh, Chamfer distance and F-score between two meshes, PSNR and SSIM of renders.

    hit = surface_distance(points, verts, faces)          # SurfaceHit(dist [K] f64, face [K] i32, bary [K,3] f64, closest [K,3] f64)
    smp = sample_surface(verts, faces, n, seed=0)         # SurfaceSamples(face_ids, bary, points): area-weighted, deterministic
    md  = mesh_distance((va, fa), (vb, fb), n_samples=100_000, thresholds=(0.005, 0.01), seed=0)
    im  = image_metrics(pred, gt, mask=None, clamp=True)  # ImageMetrics(psnr, ssim, mse, n)
    vm  = evaluate_views(model, cameras, gt_rgb, bg_color=(1., 1., 1.))
    md  = score_frame("result.obj", "ground_truth.obj")

This takes the place of the reference's scorer (gaussian_splatting/metrics.py, utils/image_utils.py), which needs torchvision
and lpips, reads PNG directories and has no geometric score.  LPIPS is not offered: its network weights are not part of this
project.

Definitions, as include/gsr.h states them and tests/eval_ref.py restates them in numpy (the same inputs give the same bits
for faces, barycentrics, points, distances, counts and maxima; sums are fixed-order and repeat from call to call).
  * The distance of a point to a mesh is the distance to the closest point of its closest triangle (the region test of
    Ericson 5.1.5 in float64); among triangles at the same squared distance the lowest index wins.
  * A sample is area-weighted by stratified integer weights and a hash of (seed, k): the same mesh, n and seed give the same
    samples everywhere.
  * mesh_distance(A, B), A the result and B the ground truth, takes n samples of each; with d_AB the distances of A's samples
    to B and d_BA those of B's samples to A, per direction mean = sum d / n, mean_sq = sum d^2 / n and max;
    chamfer = mean_AB + mean_BA, chamfer_sq = mean_sq_AB + mean_sq_BA; per threshold tau precision = #(d_AB < tau) / n,
    recall = #(d_BA < tau) / n, fscore = 2 P R / (P + R), 0 where P + R = 0.  The default thresholds are defaults, not
    measurements: choose them for the scale of the scene.
  * mse = SSE / n with the difference and its square in f32 and the sum in f64; psnr = 20 log10(1 / sqrt(mse)) in f64 on the
    host (+inf for mse = 0); ssim = losses.ssim of the (clamped) pair.  Departure from the reference, on purpose: it takes the
    mean and the logarithm in f32.  Masked SSIM is not offered: with a mask, ssim is None.
"""
from __future__ import annotations

import math
from typing import Callable, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _host, _lib, _meshargs as _ma
from ._lib import ptr as _p

_NAN = "a vertex or a query point is NaN or infinite, or too large for its distance to be formed: no face is closest"
_NO_AREA = "no face of the mesh has a positive, finite area (of at least 2^-991): it cannot be sampled"
# (no list can name a vertex twice here, and "no area" wins over the NaN it usually comes with)
_ERR = dict(index="a vertex index, or another index into the mesh or the points, lies outside its array", dup=None, nan=_NAN,
            degenerate=_NO_AREA, degenerate_first=True)


class SurfaceHit(NamedTuple):
    """Per query: its distance to the mesh, the closest face, the closest point's barycentrics (u, v, w) on that face's
    (first, second, third) vertex and the closest point itself."""
    dist: torch.Tensor
    face: torch.Tensor
    bary: torch.Tensor
    closest: torch.Tensor


class SurfaceSamples(NamedTuple):
    face_ids: torch.Tensor
    bary: torch.Tensor
    points: torch.Tensor


class DirectedDistance(NamedTuple):
    mean: float
    mean_sq: float
    max: float
    counts: Tuple[int, ...]


class MeshDistance(NamedTuple):
    """a_to_b: the result's samples against the ground truth; b_to_a: the other way.  precision, recall and fscore have one
    entry per threshold."""
    a_to_b: DirectedDistance
    b_to_a: DirectedDistance
    chamfer: float
    chamfer_sq: float
    thresholds: Tuple[float, ...]
    precision: Tuple[float, ...]
    recall: Tuple[float, ...]
    fscore: Tuple[float, ...]
    n_samples: int


class ImageMetrics(NamedTuple):
    psnr: float
    ssim: Optional[float]
    mse: float
    n: int


class ViewMetrics(NamedTuple):
    psnr: np.ndarray
    ssim: np.ndarray
    mean_psnr: float
    mean_ssim: float


def _mesh(verts, faces):
    verts, faces = _ma.mesh_f64(verts, faces)
    if int(faces.shape[0]) == 0:
        raise ValueError("the mesh has no faces")
    return verts, faces


# ------------------------------------------------------------------------------------------------ closest point
def _face_records(verts: torch.Tensor, faces: torch.Tensor, err: torch.Tensor) -> torch.Tensor:
    """tri [9,F] f64 on the current stream: what every search over this mesh stages."""
    F = int(faces.shape[0])
    tri = torch.empty(9, F, dtype=torch.float64, device=faces.device)
    _lib.check(_lib.load().gsr_eval_gather(F, int(verts.shape[0]), _p(faces), _p(verts), _p(tri), _p(err), _host.stream_of(faces)),
               "gsr_eval_gather")
    return tri


def _closest(pts: torch.Tensor, tri: torch.Tensor, err: torch.Tensor, subset=None, n_live=None) -> SurfaceHit:
    """The search alone, nothing read back.  Rows are slots: queries in order, or subset's entries."""
    dev, K = pts.device, int(pts.shape[0])
    S = K if subset is None else int(subset.shape[0])
    face = torch.full((S,), -1, dtype=torch.int32, device=dev)
    bary = torch.full((S, 3), float("nan"), dtype=torch.float64, device=dev)
    closest = torch.full((S, 3), float("nan"), dtype=torch.float64, device=dev)
    dist = torch.full((S,), float("inf"), dtype=torch.float64, device=dev)
    _lib.check(_lib.load().gsr_eval_closest(S, _p(subset), _p(n_live), K, int(tri.shape[1]), _p(pts), _p(tri), _p(face), _p(bary),
                                            _p(closest), _p(dist), _p(err), _host.stream_of(pts)), "gsr_eval_closest")
    return SurfaceHit(dist, face, bary, closest)


def _i32_on(x, dev, shape_dims: int, what: str) -> torch.Tensor:
    if not torch.is_tensor(x) or x.dtype != torch.int32 or x.device != dev or x.dim() != shape_dims:
        raise ValueError(f"{what} must be an int32 tensor on the mesh's GPU")
    return x.contiguous()


@torch.no_grad()
def surface_distance(points: torch.Tensor, verts: torch.Tensor, faces: torch.Tensor, subset: Optional[torch.Tensor] = None,
                     n_live: Optional[torch.Tensor] = None) -> SurfaceHit:
    """The closest point of the mesh for every point of points [K,3] f64.  verts [V,3] f64 (f32 is widened, which is exact),
    faces [F,3] int32 or int64, all on one GPU.  subset [S] int32: only those queries, one output row per entry, in its order;
    n_live [1] int32 on the device: only the first min(S, n_live) rows are searched (the others stay face -1, dist +inf, NaN).
    One host read: the err word.  ValueError: no faces, an index outside its array, a coordinate that is not finite."""
    verts, faces = _mesh(verts, faces)
    dev = faces.device
    pts = _ma.points_f64(points, dev, "points")
    if subset is not None:
        subset = _i32_on(subset, dev, 1, "subset")
    if n_live is not None:
        n_live = _i32_on(n_live.reshape(-1), dev, 1, "n_live")
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        hit = _closest(pts, _face_records(verts, faces, err), err, subset, n_live)
    _ma.raise_if(int(err.cpu()), **_ERR)
    return hit


# ------------------------------------------------------------------------------------------------ samples
def _sample(verts: torch.Tensor, faces: torch.Tensor, n: int, seed: int, err: torch.Tensor) -> SurfaceSamples:
    """Nothing read back: what makes the weights unusable lands in err bit 3."""
    lib, st, dev = _lib.load(), _host.stream_of(faces), faces.device
    F, V = int(faces.shape[0]), int(verts.shape[0])
    area = torch.empty(F, dtype=torch.float64, device=dev)
    _lib.check(lib.gsr_eval_areas(F, V, _p(faces), _p(verts), _p(area), _p(err), st), "gsr_eval_areas")
    m = area.max()                                                    # exact, whatever the order
    biased = (m.view(torch.int64) >> 52) & 0x7ff                      # m = mu 2^e, mu in [0.5, 1): e = biased - 1022
    ok = torch.isfinite(m) & (m > 0) & (biased >= 31)
    err |= (~ok).to(torch.int32) * 8
    scale = ((2077 - biased).clamp(1, 2046) << 52).view(torch.float64)   # 2^(32 - e), from its bits
    w = torch.floor(area * scale).to(torch.int64)
    w = torch.where(ok, w, torch.zeros_like(w))
    cum = torch.cumsum(w, 0)
    ids = torch.zeros(n, dtype=torch.int32, device=dev)
    bary = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
    points = torch.full((n, 3), float("nan"), dtype=torch.float64, device=dev)
    _lib.check(lib.gsr_eval_sample(n, F, V, _p(faces), _p(verts), _p(cum), int(seed) & (2 ** 64 - 1), _p(ids), _p(bary), _p(points),
                                   _p(err), st), "gsr_eval_sample")
    return SurfaceSamples(ids, bary, points)


def _n_samples(n) -> int:
    n = int(n)
    if not 1 <= n <= 2 ** 31 - 1:
        raise ValueError("the number of samples must lie in [1, 2^31)")
    return n


@torch.no_grad()
def sample_surface(verts: torch.Tensor, faces: torch.Tensor, n: int, seed: int = 0) -> SurfaceSamples:
    """n points on the mesh, area-weighted: face_ids [n] int32 (non-decreasing), bary [n,3] f64 (>= 0, of sum exactly 1) and
    points [n,3] f64.  Which face a sample takes is decided in integers -- weights floor(area 2^(32-e)) scaled so that the
    largest lies in [2^31, 2^32), their int64 scan, n equal strata -- so a face gets its share of n to within one sample and a
    face without area none; `seed` moves the points inside their faces, not the faces.  One host read: the err word."""
    verts, faces = _mesh(verts, faces)
    n = _n_samples(n)
    err = _ma.new_err(faces.device)
    with _host.on_device(faces.device):
        smp = _sample(verts, faces, n, seed, err)
    _ma.raise_if(int(err.cpu()), **_ERR)
    return smp


# ------------------------------------------------------------------------------------------------ mesh against mesh
def _stats_into(dist: torch.Tensor, thr: torch.Tensor, ws: torch.Tensor, out: torch.Tensor) -> None:
    _lib.check(_lib.load().gsr_eval_distance_stats(int(dist.shape[0]), _p(dist), int(thr.shape[0]), _p(thr), _p(ws), _p(out), _host.stream_of(dist)),
               "gsr_eval_distance_stats")


def _workspace(dev) -> torch.Tensor:
    return torch.empty(int(_lib.load().gsr_eval_workspace_bytes()) // 8 + 1, dtype=torch.float64, device=dev)


@torch.no_grad()
def mesh_distance(a, b, n_samples: int = 100_000, thresholds: Sequence[float] = (0.005, 0.01), seed: int = 0,
                  return_samples: bool = False):
    """The result mesh a = (verts, faces) against the ground truth b = (verts, faces): n_samples points of each (seeds `seed`
    and `seed + 1`) and their exact distances to the other mesh, d_ab and d_ba.  -> MeshDistance: per direction (a_to_b, b_to_a)
    mean = sum d / n, mean_sq = sum d^2 / n, max and the counts #(d < tau); chamfer = mean_ab + mean_ba; chamfer_sq = mean_sq_ab +
    mean_sq_ba; per threshold tau precision = #(d_ab < tau) / n, recall = #(d_ba < tau) / n, fscore = 2 P R / (P + R), 0 where
    P + R = 0.  The default thresholds are defaults, not measurements.  With return_samples also the two SurfaceHit (a's samples
    on b, b's samples on a; their `closest` lie on the other mesh).  One host read."""
    va, fa = _mesh(*a)
    vb, fb = _mesh(*b)
    dev = fa.device
    if fb.device != dev:
        raise ValueError("the two meshes must be on the same GPU")
    n = _n_samples(n_samples)
    taus = tuple(float(t) for t in thresholds)
    T = len(taus)
    if T > int(_lib.load().gsr_eval_max_thresholds()):
        raise ValueError(f"at most {_lib.load().gsr_eval_max_thresholds()} thresholds")
    thr = torch.tensor(taus, dtype=torch.float64, device=dev) if T else torch.zeros(0, dtype=torch.float64, device=dev)
    status = torch.zeros(2 * (3 + T) + 1, dtype=torch.int64, device=dev)
    err = _ma.new_err(dev)
    ws = _workspace(dev)
    hits = []
    with _host.on_device(dev):
        for d, (src, dst, s) in enumerate((((va, fa), (vb, fb), seed), ((vb, fb), (va, fa), seed + 1))):
            smp = _sample(*src, n, s, err)
            hit = _closest(smp.points, _face_records(*dst, err), err)
            _stats_into(hit.dist, thr, ws, status[d * (3 + T):])
            hits.append(hit)
    status[-1:] = err
    host = status.cpu().numpy()                                       # the one read
    _ma.raise_if(int(host[-1]), **_ERR)
    dirs = []
    for d in range(2):
        blk = host[d * (3 + T):(d + 1) * (3 + T)]
        f = blk[:3].view(np.float64)
        dirs.append(DirectedDistance(float(f[0]) / n, float(f[1]) / n, float(f[2]), tuple(int(c) for c in blk[3:])))
    ab, ba = dirs
    precision = tuple(c / n for c in ab.counts)
    recall = tuple(c / n for c in ba.counts)
    fscore = tuple(2 * p * r / (p + r) if p + r > 0 else 0.0 for p, r in zip(precision, recall))
    md = MeshDistance(ab, ba, ab.mean + ba.mean, ab.mean_sq + ba.mean_sq, taus, precision, recall, fscore, n)
    return (md, hits[0], hits[1]) if return_samples else md


def score_frame(result_obj: str, gt_obj: str, device="cuda", **kw):
    """mesh_distance of two OBJ files (formats.load_obj): the result against the ground truth."""
    from . import formats
    dev = torch.device(device)

    def mesh(path):
        v, f, _c = formats.load_obj(path)
        return torch.from_numpy(np.asarray(v, np.float64)).to(dev), torch.from_numpy(np.asarray(f)).to(dev)
    return mesh_distance(mesh(result_obj), mesh(gt_obj), **kw)


# ------------------------------------------------------------------------------------------------ images
def _chw(t: torch.Tensor, what: str) -> torch.Tensor:
    if not torch.is_tensor(t) or not t.is_cuda:
        raise ValueError(f"{what} must be a tensor on a GPU")
    if t.dim() != 3 or t.dtype != torch.float32 or min(t.shape) < 1:
        raise ValueError(f"{what} must be [C,H,W] float32, not empty")
    return t.detach()


def _sse_into(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor], clamp: bool, ws: torch.Tensor, out: torch.Tensor) -> None:
    """out [2] 64-bit words: f64 SSE, int64 count.  Views are used as they are."""
    C, H, W = (int(v) for v in pred.shape)
    _lib.check(_lib.load().gsr_eval_image_sse(C, H, W, _p(pred), pred.stride(0), pred.stride(1), pred.stride(2), _p(gt), gt.stride(0),
                                              gt.stride(1), gt.stride(2), _p(mask), int(bool(clamp)), _p(ws), _p(out), _host.stream_of(pred)),
               "gsr_eval_image_sse")


def _psnr(mse: float) -> float:
    if mse != mse:
        return float("nan")
    return float("inf") if mse == 0.0 else 20.0 * math.log10(1.0 / math.sqrt(mse))


@torch.no_grad()
def image_metrics(pred: torch.Tensor, gt: torch.Tensor, mask: Optional[torch.Tensor] = None, clamp: bool = True) -> ImageMetrics:
    """pred, gt [C,H,W] f32 on a GPU, any strides; mask [H,W] bool or uint8: only the pixels where it is set.  clamp: pred is
    first brought into [0, 1], as the reference's render code does before it writes an image.  -> ImageMetrics(psnr, ssim, mse,
    n), n the elements compared; ssim is None with a mask.  One host read."""
    pred, gt = _chw(pred, "pred"), _chw(gt, "gt")
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError("pred and gt must have the same shape and GPU")
    dev = pred.device
    if mask is not None:
        if not torch.is_tensor(mask) or tuple(mask.shape) != tuple(pred.shape[1:]) or mask.dtype not in (torch.bool, torch.uint8) \
                or mask.device != dev:
            raise ValueError("mask must be [H,W] bool or uint8 on the images' GPU")
        mask = mask.to(torch.uint8).contiguous()
    out = torch.zeros(3, dtype=torch.float64, device=dev)
    with _host.on_device(dev):
        _sse_into(pred, gt, mask, clamp, _workspace(dev), out)
    if mask is None:
        from . import losses
        out[2] = losses.ssim(pred.clamp(0.0, 1.0) if clamp else pred, gt).double()
    host = out.cpu().numpy()                                          # the one read
    n = int(host[1:2].view(np.int64)[0])
    if n == 0:
        raise ValueError("the mask keeps no pixel")
    mse = float(host[0]) / n
    return ImageMetrics(_psnr(mse), None if mask is not None else float(np.float32(host[2])), mse, n)


def evaluate_views(model, cameras: Sequence, gt_rgb: Union[torch.Tensor, Callable[[int], torch.Tensor]],
                   bg_color=(1.0, 1.0, 1.0), sh_deg: Optional[int] = None, mask: Optional[torch.Tensor] = None,
                   views_in_flight: int = 2) -> ViewMetrics:
    """Renders harness.SurfaceGaussians `model` from every camera without autograd (render_image_gaussian_rasterizer, the render
    clamped to [0, 1]) and scores it against gt_rgb, [C,3,H,W] f32 or a callable i -> [3,H,W] f32 on the model's GPU;
    views_in_flight views at a time on as many streams (pipelines.ViewPipelines).  mask [H,W]: the PSNR over its pixels; the
    SSIM is of the whole image either way.  -> ViewMetrics(psnr [C] f64, ssim [C] f32, mean_psnr, mean_ssim), numpy arrays.
    One host read, at the end."""
    from . import losses, pipelines
    dev = model.device
    n = len(cameras)
    if n == 0:
        raise ValueError("no cameras")
    if mask is not None:
        if not torch.is_tensor(mask) or mask.dim() != 2 or mask.dtype not in (torch.bool, torch.uint8) or mask.device != dev:
            raise ValueError("mask must be [H,W] bool or uint8 on the model's GPU")
        mask = mask.to(torch.uint8).contiguous()
    for cam in cameras:
        cam.on_device(dev)                                            # (the cameras' caches are not locked)
    lanes = max(1, min(int(views_in_flight), n))
    sse = torch.zeros(n, 2, dtype=torch.float64, device=dev)
    ssim = torch.zeros(n, dtype=torch.float32, device=dev)
    ws = [_workspace(dev) for _ in range(lanes)]

    def work(t, i):
        with torch.no_grad():                                         # (grad mode is per thread)
            img = model.render_image_gaussian_rasterizer(cameras[i], bg_color=bg_color, sh_deg=sh_deg)
            pred = img.permute(2, 0, 1)
            gt = _chw(gt_rgb(i) if callable(gt_rgb) else gt_rgb[i], "gt_rgb")
            if gt.shape != pred.shape or gt.device != dev:
                raise ValueError(f"view {i}: the render is {tuple(pred.shape)}, its ground truth {tuple(gt.shape)}")
            if mask is not None and tuple(mask.shape) != tuple(pred.shape[1:]):
                raise ValueError(f"view {i}: the mask is {tuple(mask.shape)}, the render {tuple(pred.shape[1:])}")
            _sse_into(pred, gt, mask, True, ws[t], sse[i])
            ssim[i] = losses.ssim(pred.clamp(0.0, 1.0), gt)

    pipelines.ViewPipelines(lanes, dev).run(work, list(range(n)))
    host = torch.cat([sse.reshape(-1), ssim.double()]).cpu().numpy()  # the one read
    counts = np.ascontiguousarray(host[1:2 * n:2]).view(np.int64)
    if (counts == 0).any():
        raise ValueError("the mask keeps no pixel")
    mse = host[0:2 * n:2] / counts
    psnr = np.array([_psnr(float(x)) for x in mse], np.float64)
    s = host[2 * n:].astype(np.float32)
    return ViewMetrics(psnr, s, float(psnr.mean()), float(s.mean()))


__all__ = ["SurfaceHit", "SurfaceSamples", "DirectedDistance", "MeshDistance", "ImageMetrics", "ViewMetrics", "surface_distance",
           "sample_surface", "mesh_distance", "score_frame", "image_metrics", "evaluate_views"]
