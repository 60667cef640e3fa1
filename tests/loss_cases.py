"""Cases, references and error measures shared by tests/test_loss_cases.py (CPU) and tests/test_gpu_losses_edges.py (GPU).
TEST INFRASTRUCTURE ONLY.

The reference is oracle/loss_oracle.py evaluated in float64 on the CPU (its window is the f32 window converted to f64, i.e.
GW[] of gsr_loss.hip), gradients from autograd; both sides get the same f32 input values.  The error of a gradient is
max|g - g64| / max(max|g64|, 1/N) with N = C H W of the cropped image: 1/N is the gradient's natural unit (the L1 term alone
is (1 - f)/N per pixel), which keeps the measure meaningful where the f64 gradient itself is ~1e-17 (pred == gt)."""
import collections
import os
import re

import torch

from conftest import ROOT
from oracle import loss_oracle

LOSS_TOL = 2e-6          # absolute on loss, l1 mean and ssim mean (tests/test_gpu_losses.py)
GRAD_TOL = 2e-4          # in the measure above
EDGE_FACTOR = 4.0        # value edges: the kernel may be this many times the f32 conv2d oracle's own error (another, equally
                         # f32, association of the same cancelling sums: separable, taps paired)
LOSS_HIP = os.path.join(ROOT, "gaustar_amd", "csrc", "gsr_loss.hip")


def tile_dims():
    """(LT, LTY) as gsr_loss.hip states them: output tile width and height of the two SSIM kernels."""
    with open(LOSS_HIP) as fh:
        src = fh.read()
    lt = re.search(r"constexpr int LT = (\d+);", src)
    lty = re.search(r"#define GSR_SSIM_TILE_H (\d+)", src)
    assert lt and lty and "constexpr int LTY = GSR_SSIM_TILE_H;" in src, "gsr_loss.hip no longer states LT / LTY this way"
    return int(lt.group(1)), int(lty.group(1))


def tile_grid(H, W):
    lt, lty = tile_dims()
    return (W + lt - 1) // lt, (H + lty - 1) // lty      # (tiles per row, tile rows) = the launch grid's (x, y)


def n_ids(C, H, W):
    """Number of (channel, tile) ids xcd_tile distributes = workgroups of a launch = partial pairs the finalize sums."""
    gx, gy = tile_grid(H, W)
    return C * gx * gy


# (C, H, W) -> what the shape is there for, as a predicate on N = n_ids (asserted by tests/test_loss_cases.py)
SSIM_SHAPES = collections.OrderedDict([
    ((1, 1, 1), ("smaller than a halo", lambda n: n == 1)),
    ((3, 5, 7), ("smaller than the window", lambda n: n == 3)),
    ((1, 11, 11), ("exactly the window", lambda n: n == 1)),
    ((3, 15, 31), ("one short of a tile", lambda n: n == 3)),
    ((3, 16, 32), ("exactly one tile", lambda n: n == 3)),
    ((3, 17, 33), ("one past a tile: 2 x 2 tiles", lambda n: n == 12)),
    ((2, 16, 32), ("N < 8", lambda n: n == 2)),
    ((1, 32, 128), ("N % 8 == 0", lambda n: n >= 8 and n % 8 == 0)),
    ((1, 48, 96), ("N % 8 == 1", lambda n: n >= 8 and n % 8 == 1)),
    ((2, 37, 70), ("N % 8 == 2", lambda n: n >= 8 and n % 8 == 2)),
    ((5, 33, 65), ("N % 8 == 5", lambda n: n >= 8 and n % 8 == 5)),
    ((1, 48, 160), ("N % 8 == 7", lambda n: n >= 8 and n % 8 == 7)),
    ((1, 16, 98304), ("finalize: the unrolled loop is not entered", lambda n: n == 3072)),
    ((1, 16, 98305), ("finalize: thread 0 alone takes one unrolled trip", lambda n: n == 3073)),
    ((1, 16, 131073), ("finalize: every thread takes one unrolled trip, thread 0 a tail", lambda n: n == 4097)),
])
REM7_SHAPE = (1, 48, 160)      # planted tiles and determinism
LAYOUT_SHAPE = (3, 37, 70)
MARGIN_SHAPE = (3, 50, 70)     # for the crops that (3, 37, 70) cannot hold (40 rows)
# name -> (shape, margin (left, right, top, bottom), cropped (H, W))
MARGINS = collections.OrderedDict([
    ("m0503", (LAYOUT_SHAPE, (0, 5, 0, 3), (34, 65))),
    ("m4020", (LAYOUT_SHAPE, (4, 0, 2, 0), (35, 66))),
    ("m0000", (LAYOUT_SHAPE, (0, 0, 0, 0), (37, 70))),
    ("crop7x40", (MARGIN_SHAPE, (10, 20, 20, 23), (7, 40))),
    ("crop40x6", (MARGIN_SHAPE, (30, 34, 4, 6), (40, 6))),
    ("crop1x1", (MARGIN_SHAPE, (34, 35, 24, 25), (1, 1))),
])
EMPTY_MARGIN = (LAYOUT_SHAPE, (35, 35, 0, 0))
PLANTED = collections.OrderedDict([("first", 0), ("middle", 7), ("last", 14)])    # tile ids of REM7_SHAPE (row-major)


def natural(c, h, w, seed):
    """A smooth image with a little noise in [0, 1] (what a render against a photograph looks like), f32, CPU."""
    g = torch.Generator().manual_seed(seed)
    base = torch.rand(1, c, h // 4 + 2, w // 4 + 2, generator=g)
    img = torch.nn.functional.interpolate(base, size=(h, w), mode="bilinear", align_corners=False)[0]
    return (img + 0.05 * torch.randn(c, h, w, generator=g)).clamp(0, 1).contiguous()


def _seed(shape, k=0):
    c, h, w = shape
    return (c * 1000003 + h * 1009 + w) * 7 + k


def pair(shape):
    return natural(*shape, _seed(shape)), natural(*shape, _seed(shape, 1))


def crop(t, margin):
    if margin is None:
        return t
    m = margin
    return t[..., m[2]:(-m[3] if m[3] else None), m[0]:(-m[1] if m[1] else None)]


def planted(which):
    """gt == pred except inside ONE tile of REM7_SHAPE.  The differences are +-[0.004, 0.012]: their sum over the tile's 512
    pixels is ~4, so that N * l1 (l1 is an f32: half an ulp of it times N is 1.2e-7 of the sum) and the f32 summation inside
    the tile stay well inside LOSS_TOL = 2e-6; |pred - gt| is exact in f32 (Sterbenz).  Returns (pred, gt, (y0, y1, x0, x1),
    planted sum in f64)."""
    c, h, w = REM7_SHAPE
    lt, lty = tile_dims()
    gx, _ = tile_grid(h, w)
    tid = PLANTED[which]
    ty, tx = divmod(tid, gx)
    y0, x0 = ty * lty, tx * lt
    y1, x1 = min(y0 + lty, h), min(x0 + lt, w)
    pred = (0.1 + 0.8 * natural(c, h, w, _seed(REM7_SHAPE, 10 + tid))).contiguous()
    g = torch.Generator().manual_seed(_seed(REM7_SHAPE, 20 + tid))
    d = (0.004 + 0.008 * torch.rand(c, y1 - y0, x1 - x0, generator=g)) * (torch.rand(c, y1 - y0, x1 - x0, generator=g) < 0.5).float().mul(2).sub(1)
    gt = pred.clone()
    gt[:, y0:y1, x0:x1] += d
    return pred, gt, (y0, y1, x0, x1), (pred.double() - gt.double()).abs().sum().item()


Case = collections.namedtuple("Case", "name pred gt f margin")


def _in_range_builders():
    b = collections.OrderedDict()
    for shape in SSIM_SHAPES:
        b["shape-%dx%dx%d" % shape] = lambda s=shape: (*pair(s), 0.2, None)
    b["c4"] = lambda: (*pair((4,) + LAYOUT_SHAPE[1:]), 0.2, None)
    b["layout"] = lambda: (*pair(LAYOUT_SHAPE), 0.2, None)
    b["noise"] = lambda: (torch.rand(LAYOUT_SHAPE, generator=torch.Generator().manual_seed(5)),
                          torch.rand(LAYOUT_SHAPE, generator=torch.Generator().manual_seed(6)), 0.2, None)
    for name, (shape, margin, _) in MARGINS.items():
        b["margin-" + name] = lambda s=shape, m=margin: (*pair(s), 0.2, m)
    for which in PLANTED:
        b["planted-" + which] = lambda k=which: (*planted(k)[:2], 0.2, None)
    b["zero-vs-one"] = lambda: (torch.zeros(LAYOUT_SHAPE), torch.ones(LAYOUT_SHAPE), 0.2, None)
    b["identical"] = lambda: (pair(LAYOUT_SHAPE)[0], pair(LAYOUT_SHAPE)[0].clone(), 0.2, None)
    b["equal-constants"] = lambda: (torch.full(LAYOUT_SHAPE, 0.5), torch.full(LAYOUT_SHAPE, 0.5), 0.2, None)
    return b


def _value_edge_builders():
    b = collections.OrderedDict()
    b["times-ten"] = lambda: (10.0 * pair(LAYOUT_SHAPE)[0], 10.0 * pair(LAYOUT_SHAPE)[1], 0.2, None)
    b["constant-ten"] = lambda: (torch.full(LAYOUT_SHAPE, 10.0), pair(LAYOUT_SHAPE)[1], 0.2, None)   # depth-as-colour background
    return b


IN_RANGE = _in_range_builders()
VALUE_EDGE = _value_edge_builders()
EXACT = ("identical", "equal-constants")          # loss, l1 and 1 - ssim are 0; with f = 0 the gradient is exactly 0


def case(name):
    pred, gt, f, margin = (IN_RANGE.get(name) or VALUE_EDGE[name])()
    return Case(name, pred, gt, f, margin)


Ref = collections.namedtuple("Ref", "loss l1 ssim grad n")     # grad: full (uncropped) image, f64, CPU
_REFS = {}


def oracle(pred, gt, f=0.2, margin=None, dtype=torch.float64, key=None):
    """loss_oracle.l1_dssim in `dtype` on the CPU, on the f32 VALUES of pred / gt; the gradient as f64.  key: cache the result
    (a reference is computed once and shared)."""
    if key is not None and (key, dtype) in _REFS:
        return _REFS[(key, dtype)]
    x = pred.detach().cpu().float().to(dtype).clone().requires_grad_(True)
    y = gt.detach().cpu().float().to(dtype)
    loss, l1, s = loss_oracle.l1_dssim(x, y, f, margin)
    loss.backward()
    r = Ref(loss.item(), l1.item(), s.item(), x.grad.double(), crop(x, margin).numel())
    if key is not None:
        _REFS[(key, dtype)] = r
    return r


def case_oracle(c, dtype=torch.float64):
    return oracle(c.pred, c.gt, c.f, c.margin, dtype, key=c.name)


def loss_err(got, ref):
    """got: (loss, l1 mean, ssim mean); the largest absolute difference of the three."""
    return max(abs(float(a) - b) for a, b in zip(got, (ref.loss, ref.l1, ref.ssim)))


def grad_err(g, ref):
    g = g.detach().cpu().double().reshape(ref.grad.shape)
    return (g - ref.grad).abs().max().item() / max(ref.grad.abs().max().item(), 1.0 / ref.n)


def outside(shape, margin):
    """bool [H, W]: pixels outside the crop (their gradient must be exactly 0)."""
    m = torch.ones(shape[-2:], dtype=torch.bool)
    crop(m, margin)[...] = False
    return m


# ---------------------------------------------------------------- masked depth / silhouette L1
MAX_DEPTH = 10.0
DEPTH_SHAPES = [(1, 1), (3, 1025), (2, 2049), (1030, 3), (1025, 1100)]   # W > 1024 / > 2048: the four-in-flight column loop
                                                                        # once more; H > 1024: the row walk wraps
DEPTH_EDGE_SHAPE = (60, 83)
# [C, H, W] render, margin, (RGB tiles, depth rows): the ride-along plane has fewer workgroups than rows in the first two
FUSED = collections.OrderedDict([
    ("4x70x33", ((4, 70, 33), (0, 0, 27, 27), 2)),
    ("6x1030x40", ((6, 1030, 40), (3, 3, 500, 500), 4)),
    ("4x5x7", ((4, 5, 7), None, 1)),
])
FUSED_FINALIZE_WIDTHS = {32768: 3072, 43712: 4098}     # [4,16,W] render -> partial pairs rgb_depth_finalize_kernel sums


def depth_pair(H, W, seed=0):
    """pred in [4, 5]; gt: ~65 % foreground in [4, 5], ~30 % background (20.0), ~5 % exactly max_depth (in neither set).  Both
    terms are O(1).  Every set is non-empty from 3 pixels on; (1, 1) is one foreground pixel."""
    g = torch.Generator().manual_seed(1000 + 31 * H + W + seed)
    pred = 4.0 + torch.rand(H, W, generator=g)
    gt = 4.0 + torch.rand(H, W, generator=g)
    u = torch.rand(H, W, generator=g)
    gt[u < 0.30] = 20.0
    gt[u > 0.95] = MAX_DEPTH
    flat = gt.view(-1)
    if flat.numel() >= 3:
        flat[0], flat[1], flat[2] = 4.5, 20.0, MAX_DEPTH
    else:
        flat[:] = 4.5
    return pred, gt


DepthRef = collections.namedtuple("DepthRef", "depth mask grad n_fg n_bg")


def depth_oracle(pred, gt, max_depth, depth_factor, mask_factor):
    """loss_oracle.depth_mask_l1 in f64 on the f32 values; a term whose factor is 0 is left out (as the trainer does)."""
    x = pred.detach().cpu().float().double().clone().requires_grad_(True)
    y = gt.detach().cpu().float().double()
    d, m = loss_oracle.depth_mask_l1(x, y, max_depth, depth_factor, mask_factor)
    d = d if depth_factor != 0.0 else torch.zeros((), dtype=torch.float64)
    m = m if mask_factor != 0.0 else torch.zeros((), dtype=torch.float64)
    tot = d + m
    if tot.requires_grad:
        tot.backward()
    grad = x.grad if x.grad is not None else torch.zeros_like(x)
    return DepthRef(d.item(), m.item(), grad, int((y < max_depth).sum()), int((y > max_depth).sum()))
