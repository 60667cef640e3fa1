"""CPU: the shared loss cases (tests/loss_cases.py) reach the tile counts and remainders they are there for -- so that a change
of LT / LTY in gsr_loss.hip fails HERE instead of silently losing coverage -- and the conditions the GPU tests put on the kernels
hold for the reference alone: the f32 conv2d oracle stays within LOSS_TOL / GRAD_TOL of the f64 one on every in-range case."""
import math

import pytest
import torch

import loss_cases as lc


def test_shapes_reach_their_tile_counts_and_remainders():
    lt, lty = lc.tile_dims()
    assert (lt, lty) == (32, 16), "the shapes of tests/loss_cases.py were chosen for 32 x 16 tiles: choose them again"
    for shape, (what, holds) in lc.SSIM_SHAPES.items():
        assert holds(lc.n_ids(*shape)), f"{shape} no longer is '{what}': N = {lc.n_ids(*shape)}"
    ns = [lc.n_ids(*s) for s in lc.SSIM_SHAPES]
    assert sum(n < 8 for n in ns) >= 6 and {n % 8 for n in ns if n >= 8} >= {0, 1, 2, 5, 7}
    assert {3072, 3073, 4097} <= set(ns)                          # where the finalize kernels' 4 x 1024 prologue starts
    assert lc.n_ids(*lc.REM7_SHAPE) == 15 and lc.tile_grid(*lc.REM7_SHAPE[1:]) == (5, 3)
    assert max(lc.PLANTED.values()) == lc.n_ids(*lc.REM7_SHAPE) - 1 and min(lc.PLANTED.values()) == 0
    for name, (shape, margin, hw) in lc.MARGINS.items():
        assert tuple(lc.crop(torch.empty(shape), margin).shape[1:]) == hw, name
    assert 0 in lc.crop(torch.empty(lc.EMPTY_MARGIN[0]), lc.EMPTY_MARGIN[1]).shape
    for name, (shape, margin, tiles) in lc.FUSED.items():
        h, w = lc.crop(torch.empty(shape), margin).shape[1:]
        assert lc.n_ids(1, h, w) == tiles, name
        assert margin is None or tiles < shape[1], name                   # fewer RGB tiles than depth rows
    for width, n in lc.FUSED_FINALIZE_WIDTHS.items():
        assert lc.n_ids(3, 16, width) == n and n in (3072, 4098)
    assert any(w > 1024 for _, w in lc.DEPTH_SHAPES) and any(w > 2048 for _, w in lc.DEPTH_SHAPES)
    assert any(h > 1024 for h, _ in lc.DEPTH_SHAPES)


def test_planted_tiles_differ_inside_one_tile_only():
    for which in lc.PLANTED:
        pred, gt, (y0, y1, x0, x1), total = lc.planted(which)
        diff = pred != gt
        assert diff[:, y0:y1, x0:x1].all() and int(diff.sum()) == (y1 - y0) * (x1 - x0) == 512
        assert 2.0 < total < 6.2 and 0.0 <= float(gt.min()) and float(gt.max()) <= 1.0
        # |pred - gt| is exact in f32: the kernel's summands are the planted ones
        assert torch.equal((pred - gt).abs().double(), (pred.double() - gt.double()).abs())


@pytest.mark.parametrize("name", list(lc.IN_RANGE))
def test_f32_oracle_within_the_project_tolerances_of_f64(name):
    c = lc.case(name)
    assert 0.0 <= float(c.pred.min()) and float(c.pred.max()) <= 1.0 and 0.0 <= float(c.gt.min()) and float(c.gt.max()) <= 1.0
    r64, r32 = lc.case_oracle(c), lc.case_oracle(c, torch.float32)
    le, ge = lc.loss_err((r32.loss, r32.l1, r32.ssim), r64), lc.grad_err(r32.grad, r64)
    print(f"{name}: f32 oracle vs f64: loss {le:.2e}, gradient {ge:.2e}")
    assert le <= lc.LOSS_TOL and ge <= lc.GRAD_TOL
    assert (r64.grad[:, lc.outside(c.pred.shape, c.margin)] == 0).all()
    if name in lc.EXACT:
        assert abs(r64.loss) <= lc.LOSS_TOL and abs(r64.l1) <= lc.LOSS_TOL and abs(1.0 - r64.ssim) <= lc.LOSS_TOL


@pytest.mark.parametrize("name", list(lc.VALUE_EDGE))
def test_value_edges_are_where_f32_itself_loses_digits(name):
    """No bound here: the GPU test holds the kernel to max(project constant, 4 x this error).  What must hold is that the cases
    are finite and leave [0, 1]."""
    c = lc.case(name)
    r64, r32 = lc.case_oracle(c), lc.case_oracle(c, torch.float32)
    le, ge = lc.loss_err((r32.loss, r32.l1, r32.ssim), r64), lc.grad_err(r32.grad, r64)
    print(f"{name}: f32 oracle vs f64: loss {le:.2e}, gradient {ge:.2e}")
    assert float(c.pred.max()) > 5.0
    assert math.isfinite(le) and math.isfinite(ge) and torch.isfinite(r32.grad).all()


def test_depth_cases_have_all_three_kinds_of_pixel():
    for H, W in lc.DEPTH_SHAPES:
        pred, gt = lc.depth_pair(H, W)
        r = lc.depth_oracle(pred, gt, lc.MAX_DEPTH, 0.7, 0.3 if H * W > 1 else 0.0)
        assert r.n_fg >= 1 and math.isfinite(r.depth) and math.isfinite(r.mask)
        if H * W > 1:
            assert r.n_bg >= 1 and r.n_fg + r.n_bg < H * W and 0.05 < r.depth < 1.0 and 0.5 < r.mask < 3.0   # terms of O(1)
        nz = int((r.grad != 0).sum())
        assert nz == r.n_fg + r.n_bg or H * W == 1
