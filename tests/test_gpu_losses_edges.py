"""GPU: the fused image losses (gsr_loss.hip through gaustar_amd/losses.py) at tile, layout and value edges, against
oracle/loss_oracle.py in float64 on the same f32 values.  Cases, reference and error measure: tests/loss_cases.py (pinned on
the CPU by tests/test_loss_cases.py).  Every comparison is over ALL elements of the full, uncropped gradient; pixels outside a
crop must be exactly 0.  Each test prints its figures before it asserts."""
import math

import numpy as np
import pytest
import torch

import loss_cases as lc
from loss_cases import GRAD_TOL, LOSS_TOL

pytestmark = pytest.mark.gpu


def _run(pred, gt, f=0.2, margin=None):
    """value + gradient through the public API.  pred: a CPU tensor (uploaded, made a leaf) or a device LEAF used as it is."""
    from gaustar_amd import losses
    p = pred.cuda().requires_grad_(True) if not pred.is_cuda else pred
    loss, parts = losses.l1_dssim_loss(p, gt.cuda(), f, margin, return_parts=True)
    loss.backward()
    parts = parts.cpu()
    assert float(loss.detach()) == float(parts[0])
    return parts, p.grad.detach().cpu()


def _hold(name, parts, grad, ref, loss_tol=LOSS_TOL, grad_tol=GRAD_TOL):
    le, ge = lc.loss_err(parts.tolist(), ref), lc.grad_err(grad, ref)
    print(f"{name}: kernel vs f64: loss {le:.2e} (bound {loss_tol:.2e}), gradient {ge:.2e} (bound {grad_tol:.2e})")
    assert torch.isfinite(grad).all()
    assert le <= loss_tol, f"{name}: loss / l1 / ssim off by {le:.3e}"
    assert ge <= grad_tol, f"{name}: gradient error {ge:.3e} in units of max(max|g64|, 1/N)"
    return le, ge


# ---------------------------------------------------------------- SSIM + L1: shapes
@pytest.mark.parametrize("name", ["shape-%dx%dx%d" % s for s in lc.SSIM_SHAPES] + ["c4", "noise", "zero-vs-one"])
def test_l1_dssim_shapes_against_f64(name, hip_lib):
    c = lc.case(name)
    parts, grad = _run(c.pred, c.gt, c.f)
    _hold(name, parts, grad, lc.case_oracle(c))


@pytest.mark.parametrize("which", list(lc.PLANTED))
def test_planted_tile_is_counted_once_and_only_there(which, hip_lib):
    """gt == pred except inside one tile of the N % 8 == 7 shape (first, middle, last id): a tile that xcd_tile drops or hands out
    twice loses or moves the planted sum and the gradient's support."""
    pred, gt, (y0, y1, x0, x1), total = lc.planted(which)
    n = pred.numel()
    c = lc.case("planted-" + which)
    ref = lc.case_oracle(c)
    parts, grad = _run(pred, gt, 0.2)
    print(f"planted-{which}: N * l1 = {n * float(parts[1]):.9g}, planted sum = {total:.9g}")
    assert abs(n * float(parts[1]) - total) <= LOSS_TOL
    _hold("planted-" + which, parts, grad, ref)
    # support: window forward + adjoint = the tile grown by 10.  Outside it pred == gt over the whole window, the f64 gradient is
    # ~1e-17 and an f32 evaluation leaves rounding noise: "zero" is GRAD_TOL of the unit 1/N, and inside the gradient is O(1/N).
    grown = torch.zeros(pred.shape[1:], dtype=torch.bool)
    grown[max(y0 - 10, 0):y1 + 10, max(x0 - 10, 0):x1 + 10] = True
    unit = max(ref.grad.abs().max().item(), 1.0 / n)
    assert float(grad[:, ~grown].abs().max()) <= GRAD_TOL * unit and float(grad[:, y0:y1, x0:x1].abs().max()) > 0.5 / n
    # the L1 part alone (f = 0) is exact: +-(1/N as the kernel forms it) on the planted pixels, 0.0 everywhere else
    parts0, grad0 = _run(pred, gt, 0.0)
    want = torch.sign(pred - gt) * float(np.float32(1.0) / np.float32(n))
    assert torch.equal(grad0, want) and abs(n * float(parts0[0]) - total) <= LOSS_TOL


# ---------------------------------------------------------------- SSIM + L1: layouts
_CONTIG = {}


def _contiguous_run(C):
    if C not in _CONTIG:
        pred, gt = lc.pair((C,) + lc.LAYOUT_SHAPE[1:])
        _CONTIG[C] = (pred, gt) + _run(pred, gt, 0.2)
    return _CONTIG[C]


def _garbage(*shape):
    return torch.full(shape, 7.0)       # what a read outside the view would bring in


def _layout(layout, pred, gt):
    """-> (pred as the kernel gets it, the leaf that collects its gradient, view of the leaf's gradient -> [C,H,W], gt)."""
    C, H, W = pred.shape
    if layout in ("hwc", "c2-hwc", "c4-hwc"):
        leaf = pred.permute(1, 2, 0).contiguous().cuda().requires_grad_(True)            # [H,W,C] storage
        return leaf.permute(2, 0, 1), leaf, lambda g: g.permute(2, 0, 1), gt.permute(1, 2, 0).contiguous().cuda().permute(2, 0, 1)
    if layout == "row-padded":
        wp, wg = _garbage(C, H, W + 13), _garbage(C, H, W + 9)
        wp[..., 5:5 + W], wg[..., 3:3 + W] = pred, gt
        leaf = wp.cuda().requires_grad_(True)
        return leaf[..., 5:5 + W], leaf, lambda g: g[..., 5:5 + W], wg.cuda()[..., 3:3 + W]
    if layout == "every-second-column":
        wp, wg = _garbage(C, H, 2 * W), _garbage(C, H, 2 * W + 1)
        wp[..., ::2], wg[..., 1::2] = pred, gt
        leaf = wp.cuda().requires_grad_(True)
        return leaf[..., ::2], leaf, lambda g: g[..., ::2], wg.cuda()[..., 1::2]
    if layout == "gt-expanded":
        leaf = pred.cuda().requires_grad_(True)
        return leaf, leaf, lambda g: g, gt[:1].cuda().expand(C, H, W)
    if layout == "batch-of-one":
        leaf = pred[None].cuda().requires_grad_(True)
        return leaf, leaf, lambda g: g[0], gt.cuda()[None]
    raise KeyError(layout)


# Whether the gradient came out bit-identical to the contiguous run's on the MI355X (True: it is held to that; False: it is held
# to GRAD_TOL against f64 instead).  The loss is bit-identical in every layout: the arithmetic does not depend on addresses.
GRAD_BIT_IDENTICAL = {"hwc": True, "row-padded": True, "every-second-column": True, "gt-expanded": True, "batch-of-one": True,
                      "c2-hwc": True, "c4-hwc": True, "generic": True}


def _hold_layout(name, parts, grad, parts_c, grad_c, ref):
    same = torch.equal(grad, grad_c)
    print(f"{name}: loss bit-identical to the contiguous run: {torch.equal(parts, parts_c)}, gradient bit-identical: {same}")
    assert torch.equal(parts, parts_c), f"{name}: {parts.tolist()} != contiguous {parts_c.tolist()}"
    _hold(name, parts, grad, ref)
    if GRAD_BIT_IDENTICAL[name]:
        assert same, f"{name}: gradient differs from the contiguous run by {float((grad - grad_c).abs().max()):.3e}"


@pytest.mark.parametrize("layout", ["hwc", "row-padded", "every-second-column", "gt-expanded", "batch-of-one", "c2-hwc", "c4-hwc"])
def test_layouts_compute_what_the_contiguous_image_does(layout, hip_lib):
    from gaustar_amd import losses
    C = {"c2-hwc": 2, "c4-hwc": 4}.get(layout, 3)
    pred, gt, parts_c, grad_c = _contiguous_run(C)
    if layout == "gt-expanded":                                   # other values: its own contiguous run
        gt = gt[:1].expand_as(pred).contiguous()
        parts_c, grad_c = _run(pred, gt, 0.2)
    p, leaf, view, g = _layout(layout, pred, gt)
    assert layout in ("gt-expanded", "batch-of-one") or not p.is_contiguous()
    assert layout != "gt-expanded" or g.stride(0) == 0
    loss, parts = losses.l1_dssim_loss(p, g, 0.2, return_parts=True)
    loss.backward()
    assert leaf.grad.shape == leaf.shape
    grad = view(leaf.grad).cpu()
    ref = lc.oracle(pred, gt, 0.2, key=("layout", layout))
    _hold_layout(layout, parts.cpu(), grad, parts_c, grad_c, ref)
    rest = leaf.grad.clone()
    view(rest).zero_()
    assert not rest.any()                                          # nothing of the storage outside the view is touched


def test_generic_instantiation_through_a_view_that_does_not_fit_32_bits(hip_lib):
    """ssim_stats_kernel<false> / ssim_grad_kernel<false> through the public API: 20 rows of a 2 GiB buffer whose row stride puts
    the last element at 2^29 elements or beyond, which view_fits_32 refuses.  (19 row strides of ceil(2^29 / 19) reach 2^29 + 4,
    so the buffer holds 19 strides + W elements; it stays untouched except for the rows used.)"""
    from gaustar_amd import losses
    W, H = 45, 20
    sy = -(-2 ** 29 // (H - 1))
    assert (H - 1) * sy + W - 1 >= 2 ** 29
    pred, gt = lc.pair((1, H, W))
    parts_c, grad_c = _run(pred, gt, 0.2)
    buf = torch.empty((H - 1) * sy + W, device="cuda")
    p = buf.as_strided((1, H, W), (0, sy, 1))
    p.copy_(pred.cuda())
    p = p.detach().requires_grad_(True)
    assert p.stride() == (0, sy, 1) and p.data_ptr() == buf.data_ptr()
    loss, parts = losses.l1_dssim_loss(p, gt.cuda(), 0.2, return_parts=True)
    loss.backward()
    parts, grad = parts.cpu(), p.grad.cpu()
    del p, loss, buf
    torch.cuda.empty_cache()
    _hold_layout("generic", parts, grad, parts_c, grad_c, lc.oracle(pred, gt, 0.2, key="generic"))


# ---------------------------------------------------------------- SSIM + L1: margins, dtypes
@pytest.mark.parametrize("name", list(lc.MARGINS))
def test_margins_against_the_oracles_own_crop(name, hip_lib):
    shape, margin, hw = lc.MARGINS[name]
    c = lc.case("margin-" + name)
    parts, grad = _run(c.pred, c.gt, c.f, margin)
    ref = lc.case_oracle(c)
    assert ref.n == shape[0] * hw[0] * hw[1]
    _hold("margin-" + name, parts, grad, ref)
    assert (grad[:, lc.outside(shape, margin)] == 0).all()


def test_a_margin_that_leaves_nothing_raises(hip_lib):
    from gaustar_amd import losses
    shape, margin = lc.EMPTY_MARGIN
    pred, gt = lc.pair(shape)
    with pytest.raises(RuntimeError, match="empty image"):
        losses.l1_dssim_loss(pred.cuda(), gt.cuda(), 0.2, margin)


@pytest.mark.parametrize("dtype", [torch.float64, torch.float16])
def test_pred_of_another_dtype_gets_its_gradient_in_that_dtype(dtype, hip_lib):
    from gaustar_amd import losses
    pred, gt = lc.pair(lc.LAYOUT_SHAPE)
    margin = (4, 0, 2, 0)
    p = pred.to(dtype).cuda().requires_grad_(True)
    loss, parts = losses.l1_dssim_loss(p, gt.cuda(), 0.2, margin, return_parts=True)
    loss.backward()
    parts32, grad32 = _run(p.detach().float().cpu(), gt, 0.2, margin)        # the f32 run of the converted input
    assert torch.equal(parts.cpu(), parts32)
    assert p.grad.dtype == dtype and p.grad.shape == p.shape
    assert torch.equal(p.grad.cpu(), grad32.to(dtype))


# ---------------------------------------------------------------- SSIM + L1: values
@pytest.mark.parametrize("name", list(lc.VALUE_EDGE))
def test_value_edges_within_four_times_the_f32_oracles_own_error(name, hip_lib):
    """Outside [0, 1] (the render is not clamped; depth-as-colour and its background reach 10) E[x^2] - mu^2 cancels against
    C2 = 9e-4 and ANY f32 evaluation loses digits: the bound is max(project constant, 4 x the error of the f32 conv2d oracle,
    which is what the trainer would otherwise run), not a fixed number."""
    c = lc.case(name)
    r64, r32 = lc.case_oracle(c), lc.case_oracle(c, torch.float32)
    le32, ge32 = lc.loss_err((r32.loss, r32.l1, r32.ssim), r64), lc.grad_err(r32.grad, r64)
    parts, grad = _run(c.pred, c.gt, c.f)
    le, ge = lc.loss_err(parts.tolist(), r64), lc.grad_err(grad, r64)
    print(f"{name}: f32 oracle vs f64: loss {le32:.3e}, gradient {ge32:.3e}; kernel / f32 oracle: loss {le / max(le32, 1e-300):.3f}, "
          f"gradient {ge / max(ge32, 1e-300):.3f}")
    _hold(name, parts, grad, r64, max(LOSS_TOL, lc.EDGE_FACTOR * le32), max(GRAD_TOL, lc.EDGE_FACTOR * ge32))


@pytest.mark.parametrize("name", lc.EXACT)
def test_equal_images_lose_nothing_and_have_no_l1_gradient(name, hip_lib):
    c = lc.case(name)
    assert torch.equal(c.pred, c.gt)
    parts, grad = _run(c.pred, c.gt, 0.2)
    print(f"{name}: loss {float(parts[0]):.3e}, l1 {float(parts[1]):.3e}, 1 - ssim {1.0 - float(parts[2]):.3e}")
    assert abs(float(parts[0])) <= LOSS_TOL and abs(float(parts[1])) <= LOSS_TOL and abs(1.0 - float(parts[2])) <= LOSS_TOL
    _hold(name, parts, grad, lc.case_oracle(c))                    # (the f64 gradient is ~1e-17: this is the 1/N floor of the measure)
    parts0, grad0 = _run(c.pred, c.gt, 0.0)                        # d|x - y|/dx at 0 is 0, as in torch
    assert float(parts0[0]) == 0.0 and float(parts0[1]) == 0.0 and not grad0.any()


# ---------------------------------------------------------------- masked depth / silhouette L1
def _run_depth(pred, gt, depth_factor, mask_factor, max_depth=lc.MAX_DEPTH, leaf=None):
    """pred: a CPU tensor (uploaded, made a leaf) or a device view of `leaf`; -> (loss, parts, gradient of the leaf)."""
    from gaustar_amd import losses
    p = pred.cuda().requires_grad_(True) if not pred.is_cuda else pred
    loss, parts = losses.depth_mask_l1_loss(p, gt if gt.is_cuda else gt.cuda(), max_depth, depth_factor, mask_factor, return_parts=True)
    loss.backward()
    return float(loss), parts.cpu(), (p if leaf is None else leaf).grad.detach().cpu()


def _hold_depth(name, parts, grad, ref):
    print(f"{name}: depth term off by {abs(float(parts[0]) - ref.depth):.2e}, mask term by {abs(float(parts[1]) - ref.mask):.2e}, "
          f"fg {int(parts[2])} / {ref.n_fg}, bg {int(parts[3])} / {ref.n_bg}")
    assert abs(float(parts[0]) - ref.depth) <= 1e-6 and abs(float(parts[1]) - ref.mask) <= 1e-6
    assert float(parts[2]) == ref.n_fg and float(parts[3]) == ref.n_bg
    np.testing.assert_allclose(grad.numpy(), ref.grad.numpy(), rtol=1e-5, atol=0)


@pytest.mark.parametrize("shape", lc.DEPTH_SHAPES, ids=lambda s: "%dx%d" % s)
def test_depth_shapes_against_f64(shape, hip_lib):
    pred, gt = lc.depth_pair(*shape)
    mf = 0.3 if shape != (1, 1) else 0.0                          # one foreground pixel: the mask term is off
    loss, parts, grad = _run_depth(pred, gt, 0.7, mf)
    ref = lc.depth_oracle(pred, gt, lc.MAX_DEPTH, 0.7, mf)
    _hold_depth("depth %dx%d" % shape, parts, grad, ref)
    assert abs(loss - (ref.depth + ref.mask)) <= 2e-6


def test_depth_layouts_a_channel_of_hwc_storage_and_a_transposed_gt(hip_lib):
    H, W = lc.DEPTH_EDGE_SHAPE
    pred, gt = lc.depth_pair(H, W)
    ref = lc.depth_oracle(pred, gt, lc.MAX_DEPTH, 0.7, 0.3)
    store = _garbage(H, W, 3)
    store[..., 1] = pred
    leaf = store.cuda().requires_grad_(True)
    gt_t = gt.t().contiguous().cuda().t()                          # [W,H] storage seen as [H,W]
    assert gt_t.stride() == (1, H)
    _, parts, grad = _run_depth(leaf[..., 1], gt_t, 0.7, 0.3, leaf=leaf)
    _hold_depth("depth hwc channel / transposed gt", parts, grad[..., 1], ref)
    assert not grad[..., 0].any() and not grad[..., 2].any()


def test_depth_value_edges(hip_lib):
    H, W = lc.DEPTH_EDGE_SHAPE
    pred, gt = lc.depth_pair(H, W)
    gt[5:25, 10:40] = 4.0 + torch.rand(20, 30, generator=torch.Generator().manual_seed(2))
    pred[5:25, 10:40] = gt[5:25, 10:40]                            # pred == gt on foreground: no gradient
    gt[30:50, 20:70] = lc.MAX_DEPTH                                # in neither set
    gt[0:5, 50:83] = float("inf")                                  # background
    ref = lc.depth_oracle(pred, gt, lc.MAX_DEPTH, 0.7, 0.3)
    _, parts, grad = _run_depth(pred, gt, 0.7, 0.3)
    _hold_depth("depth value edges", parts, grad, ref)
    assert not grad[5:25, 10:40].any() and not grad[30:50, 20:70].any() and (grad[0:5, 50:83] < 0).all()


@pytest.mark.parametrize("empty", ["foreground", "background"])
def test_depth_empty_sets(empty, hip_lib):
    """A term whose factor is 0 is absent (exactly 0, no NaN in the gradient) even where its set is empty; an ENABLED term over an
    empty set is NaN, like torch.mean of an empty selection."""
    H, W = lc.DEPTH_EDGE_SHAPE
    pred, _ = lc.depth_pair(H, W)
    gt = torch.full((H, W), 20.0) if empty == "foreground" else 4.0 + torch.rand(H, W, generator=torch.Generator().manual_seed(4))
    k = 0 if empty == "foreground" else 1
    off = (0.0, 0.3) if empty == "foreground" else (0.7, 0.0)
    loss, parts, grad = _run_depth(pred, gt, *off)
    ref = lc.depth_oracle(pred, gt, lc.MAX_DEPTH, *off)
    assert float(parts[k]) == 0.0 and float(parts[2 + k]) == 0.0 and math.isfinite(loss) and torch.isfinite(grad).all()
    _hold_depth(f"depth, no {empty}, its factor 0", parts, grad, ref)
    on = (1.0, 0.3) if empty == "foreground" else (0.7, 1.0)
    loss, parts, _ = _run_depth(pred, gt, *on)
    assert math.isnan(float(parts[k])) and math.isnan(loss)


# ---------------------------------------------------------------- the fused pair
def _fused_pair(shape, margin, seed=8):
    from gaustar_amd import losses
    C, H, W = shape
    g = torch.Generator().manual_seed(seed)
    img = torch.rand(C, H, W, generator=g)
    img[3:] = img[3:] * 12.0
    gt_rgb = torch.rand(1, 3, H, W, generator=g).cuda()
    gt_d = (torch.rand(H, W, generator=g) * 14.0).cuda()
    a = img.cuda().requires_grad_(True)
    b = img.cuda().requires_grad_(True)
    la, parts = losses.rgb_depth_loss(a, gt_rgb, gt_d, 10.0, 0.2, 0.7, 0.3, margin=margin, return_parts=True)
    lb = losses.l1_dssim_loss(b[:3], gt_rgb, 0.2, margin=margin) + losses.depth_mask_l1_loss(b[3], gt_d, 10.0, 0.7, 0.3)
    (2.0 * la).backward()
    (2.0 * lb).backward()
    print(f"fused {shape} {margin}: loss {float(la):.9g} vs {float(lb):.9g}, gradient off by {float((a.grad - b.grad).abs().max()):.2e}")
    assert abs(float(la) - float(lb)) < 1e-6 and parts.numel() == 7
    assert torch.allclose(a.grad, b.grad, rtol=0, atol=1e-9) and float(a.grad[:4].abs().max()) > 0
    return a.grad.cpu()


@pytest.mark.parametrize("name", list(lc.FUSED))
def test_rgb_depth_loss_equals_the_two_separate_losses_at_edges(name, hip_lib):
    """As test_gpu_losses.py::test_rgb_depth_loss_equals_the_two_separate_losses, where the ride-along depth plane has fewer
    workgroups than the depth image has rows, and on an image smaller than the window."""
    shape, margin, _ = lc.FUSED[name]
    grad = _fused_pair(shape, margin)
    assert not grad[4:].any()
    assert not grad[:3][:, lc.outside(shape, margin)].any()        # the RGB gradient stays inside the crop ..
    assert (grad[3] != 0).all() and grad[:3].any()                  # .. the depth gradient covers the WHOLE image


@pytest.mark.parametrize("width", list(lc.FUSED_FINALIZE_WIDTHS))
def test_rgb_depth_finalize_where_its_unrolled_loop_starts(width, hip_lib):
    """rgb_depth_finalize_kernel sums 3 x tiles partial pairs: 3072 (the 4 x 1024 prologue is not entered) and 4098 (every thread
    takes one trip, two threads a tail)."""
    assert lc.n_ids(3, 16, width) == lc.FUSED_FINALIZE_WIDTHS[width]
    grad = _fused_pair((4, 16, width), None, seed=9)
    assert (grad[3] != 0).all()


# ---------------------------------------------------------------- determinism
@pytest.mark.parametrize("what", ["ssim", "depth", "fused"])
def test_two_calls_give_the_same_bits(what, hip_lib):
    """The file header of gsr_loss.hip promises a deterministic value (fixed-order reductions); the gradient has no reduction."""
    from gaustar_amd import losses
    if what == "ssim":
        pred, gt = lc.pair(lc.REM7_SHAPE)
        fn = lambda: _run(pred, gt, 0.2)
    elif what == "depth":
        pred, gt = lc.depth_pair(1030, 3)
        fn = lambda: _run_depth(pred, gt, 0.7, 0.3)[1:]
    else:
        shape, margin, _ = lc.FUSED["6x1030x40"]
        g = torch.Generator().manual_seed(8)
        img = torch.rand(shape, generator=g)
        img[3:] = img[3:] * 12.0
        gt_rgb, gt_d = torch.rand(3, *shape[1:], generator=g).cuda(), (torch.rand(shape[1:], generator=g) * 14.0).cuda()

        def fn():
            a = img.cuda().requires_grad_(True)
            loss, parts = losses.rgb_depth_loss(a, gt_rgb, gt_d, 10.0, 0.2, 0.7, 0.3, margin=margin, return_parts=True)
            loss.backward()
            return torch.cat([parts.cpu(), loss.detach().cpu()[None]]), a.grad.cpu()
    (p1, g1), (p2, g2) = fn(), fn()
    assert torch.equal(p1, p2) and torch.equal(g1, g2) and torch.isfinite(p1).all()
