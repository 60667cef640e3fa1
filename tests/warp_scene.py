"""The analytic scene of the warp tests (tests/test_warp.py, tests/test_gpu_warp.py, tools/bench_warp.py): a sphere that
turns 4 degrees about the vertical axis through its centre and moves by (0.02, -0.01, 0.03) m between two frames.

Depth maps are ray-sphere z-depths at pixel centres (pixel (r, c) at pix = (r, c), the reference's projection without the
principal point), 10 off the subject.  The flows come from back-projecting each pixel onto the sphere, moving the point (or
moving it back) and re-projecting it, stored as RAFT stores them ([h, w, 2] in (x, y) order), 0 off the subject.  The turn
leaves both depth maps unchanged, so only a correct flow path recovers it.  Built with torch in f64 on any device."""
import math

import numpy as np
import torch

TURN_DEG = 4.0
SHIFT = (0.02, -0.01, 0.03)
BACKGROUND = 10.0


def motion():
    """(R [3,3], t [3]) f64 numpy: x' = R (x - c) + c + t for the sphere centre c."""
    a = math.radians(TURN_DEG)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    return R, np.asarray(SHIFT, np.float64)


def moved(verts, center):
    """The vertices of frame f+1: R (v - c) + c + t, f64."""
    R, t = motion()
    c = np.asarray(center, np.float64)
    return (np.asarray(verts, np.float64) - c) @ R.T + c + t


def _rays(H, W, fx, fy, device):
    r = torch.arange(H, dtype=torch.float64, device=device)[:, None].expand(H, W)
    c = torch.arange(W, dtype=torch.float64, device=device)[None, :].expand(H, W)
    return r, c, torch.stack([(c - W * 0.5) / fx, (r - H * 0.5) / fy, torch.ones_like(r)], -1)


def _hit(d_loc, Rw, tw, centre, radius):
    """z-depth of the first hit of the local rays d_loc (z = 1) with the sphere; NaN where none."""
    o = -(Rw.T @ tw)                                  # camera centre in the world
    d = d_loc @ Rw                                    # world directions (R^T d per pixel)
    oc = o - centre
    b = (d * oc).sum(-1)
    a = (d * d).sum(-1)
    disc = b * b - a * ((oc * oc).sum() - radius * radius)
    lam = (-b - torch.sqrt(disc)) / a
    lam = torch.where((disc > 0) & (lam > 0), lam, torch.full_like(lam, float("nan")))
    return lam, o, d


def _project(X, Rw, tw, fx, fy, H, W):
    loc = X @ Rw.T + tw
    return fy * (loc[..., 1] / loc[..., 2]) + H * 0.5, fx * (loc[..., 0] / loc[..., 2]) + W * 0.5


def frames(extr, intr, shape, center, radius, device="cpu", flow_shape=None, pad=None):
    """One camera -> (flow_f, flow_b [h,w,2] f32, depth_cur, depth_next [H,W] f32) on `device`.  flow_shape (h, w) and pad
    (top, bottom, left, right): store the flows as RAFT would for a padded, downscaled input -- the full-resolution flow at
    the pixel cv2's nearest resize reads for each padded position, divided by the f32 scale the reader multiplies by."""
    H, W = int(shape[0]), int(shape[1])
    fx, fy = float(intr[0, 0]), float(intr[1, 1])
    dev = torch.device(device)
    Rw = torch.as_tensor(np.asarray(extr, np.float64)[:3, :3], device=dev)
    tw = torch.as_tensor(np.asarray(extr, np.float64)[:3, 3], device=dev)
    c0 = torch.as_tensor(np.asarray(center, np.float64), device=dev)
    Rm, tm = (torch.as_tensor(x, device=dev) for x in motion())
    c1 = c0 + tm
    r, c, dl = _rays(H, W, fx, fy, dev)
    out = []
    flows = []
    for centre, other, fwd in ((c0, c1, True), (c1, c0, False)):
        lam, o, d = _hit(dl, Rw, tw, centre, radius)
        X = o + d * lam[..., None]
        Y = (X - centre) @ Rm + other if not fwd else (X - centre) @ Rm.T + other      # forward: R (x - c0) + c1
        pr, pc = _project(Y, Rw, tw, fx, fy, H, W)
        hit = ~torch.isnan(lam)
        fl = torch.stack([torch.where(hit, pc - c, 0.0), torch.where(hit, pr - r, 0.0)], -1)
        flows.append(fl)
        out.append(torch.where(hit, lam, torch.full_like(lam, BACKGROUND)).float())
    if flow_shape is not None:
        h, w = flow_shape
        top, bottom, left, right = pad if pad is not None else (0, 0, 0, 0)
        hp, wp = h + top + bottom, w + left + right
        scale = float(np.float32(H / hp))
        # the full-resolution pixel that resizeNN maps padded position (i, j) to is the smallest y with floor(y / (H / hp))
        # = i; take the flow there (any pixel of the block would do for the tests)
        ys = torch.clamp(torch.ceil((torch.arange(h, device=dev, dtype=torch.float64) + top) * (H / hp)), max=H - 1).long()
        xs = torch.clamp(torch.ceil((torch.arange(w, device=dev, dtype=torch.float64) + left) * (W / wp)), max=W - 1).long()
        flows = [fl[ys][:, xs] / scale for fl in flows]
    return flows[0].float().contiguous(), flows[1].float().contiguous(), out[0].contiguous(), out[1].contiguous()
