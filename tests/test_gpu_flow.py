"""RAFT optical flow on the GPU (gaustar_amd.flow, csrc/gsr_flow.hip): every kernel against f64 torch on the host with a
bound derived from the f32 format (u = 2^-24 is the unit roundoff), the whole model against tests/flow_ref.py in f64 with
the fixture's sensitivities, the bit-for-bit identities, the files and the refusals."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_ref
from conftest import GOLDEN_DIR

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
U = 2.0 ** -24
STAGES = (1, 4, 20)


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _randn(seed, *shape):
    return torch.randn(*shape, generator=_gen(seed), dtype=torch.float32)


def _slice(t, off=0, ch=None):
    from gaustar_amd import flow
    return flow._slice(t, off, ch)


def _bits_equal(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------ convolution
def _run_conv(lib, parts, weight, bias, stride=1, act=0, bn=None, residual=None, residual_relu=False, out_width=None, in_place_residual=False):
    """parts: [(buffer [N,H,W,Cbuf] f32 host, offset, channels)].  Returns (out buffer on the host [N,Ho,Wo,out_width], x NCHW f64)."""
    from gaustar_amd import flow
    from gaustar_amd._lib import FlowConvDesc
    c = flow._Conv(lib, weight, bias, DEV, bn)
    N, H, W, _ = parts[0][0].shape
    bufs = [p[0].to(DEV) for p in parts]
    kh, kw = weight.shape[2:]
    Ho, Wo = (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1
    width = c.Cout if out_width is None else out_width
    out = torch.full((N, Ho, Wo, width), 7.0, dtype=torch.float32, device=DEV)
    d = FlowConvDesc()
    d.N, d.H, d.W, d.KH, d.KW, d.stride, d.n_in, d.Cout, d.act, d.residual_relu = N, H, W, kh, kw, stride, len(parts), c.Cout, act, int(residual_relu)
    for i, (b, (_, off, ch)) in enumerate(zip(bufs, parts)):
        d.inputs[i] = _slice(b, off, ch)
    d.out = _slice(out, 0, c.Cout)
    res_dev = None
    if in_place_residual:
        out.copy_(residual.to(DEV))
        d.residual = d.out
    elif residual is not None:
        res_dev = residual.to(DEV)
        d.residual = _slice(res_dev)
    d.weights, d.bias = c.w.data_ptr(), c.b.data_ptr()
    if bn is not None:
        d.scale, d.shift = c.scale.data_ptr(), c.shift.data_ptr()
    rc = lib.gsr_flow_conv(ctypes.addressof(d), None)
    assert rc == 0, lib.gsr_last_error()
    torch.cuda.synchronize()
    x = torch.cat([p[0][..., p[1]:p[1] + p[2]] for p in parts], -1).double().permute(0, 3, 1, 2)
    return out.cpu(), x, c


def _conv_bound(x, weight, bias, stride, act, bn_c, residual):
    """(reference, bound), both [N,Ho,Wo,Cout] f64.  The device's result is a k-ordered f32 fma chain of K products from 0
    plus the bias: |err| <= (K + 2) u (sum|a b| + |bias|).  Then, each step adding its own roundings to the error so far e:
      scale and shift  y = v sc + sh: e |sc| + 2 u (|v sc| + |sh|)       (one product, one sum)
      relu, none       1-Lipschitz and exact: e
      sigmoid, tanh    1-Lipschitz; expf / tanhf within 2 ulp = 4 u, one sum and one quotient for the sigmoid: e + 8 u |f|
      residual         one sum: e + u |f + r|, the relu after it exact."""
    w, b = weight.double(), bias.double()
    pad = (weight.shape[2] // 2, weight.shape[3] // 2)
    K = weight.shape[1] * weight.shape[2] * weight.shape[3]
    v = F.conv2d(x, w, b, stride=stride, padding=pad)
    e = (K + 2) * U * (F.conv2d(x.abs(), w.abs(), None, stride=stride, padding=pad) + b.abs()[None, :, None, None])
    if bn_c is not None:
        sc, sh = bn_c.scale.cpu().double()[None, :, None, None], bn_c.shift.cpu().double()[None, :, None, None]
        e = e * sc.abs() + 2 * U * ((v * sc).abs() + sh.abs())
        v = v * sc + sh
    if act == 1:
        v = torch.relu(v)
    elif act in (2, 3):
        v = torch.sigmoid(v) if act == 2 else torch.tanh(v)
        e = e + 8 * U * v.abs()
    v, e = v.permute(0, 2, 3, 1), e.permute(0, 2, 3, 1)
    if residual is not None:
        r = residual.double()
        v = v + r
        e = e + U * v.abs()
    return v, e


def _bn(seed, c):
    g = _gen(seed)
    return (0.8 + 0.4 * torch.rand(c, generator=g), 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g),
            0.5 + torch.rand(c, generator=g))


# name: (N, H, W, [(buffer width, offset, channels)], Cout, kh, kw, stride, act, bn, residual kind, residual relu, out width)
CONV_CASES = {
    "7x7 stride 2, Cin 3, odd H and W, batch norm + relu": (1, 19, 23, [(3, 0, 3)], 64, 7, 7, 2, 1, True, None, False, None),
    "7x7, Cin 2 at the end of a 128-wide buffer": (1, 9, 11, [(128, 126, 2)], 128, 7, 7, 1, 1, False, None, False, None),
    "3x3, Cout 2, added in place (the flow's update)": (1, 10, 9, [(256, 0, 256)], 2, 3, 3, 1, 0, False, "in place", False, None),
    "3x3, 256 -> 126 into a 128-wide buffer": (1, 8, 9, [(256, 0, 256)], 126, 3, 3, 1, 1, False, None, False, 128),
    "1x1, 324 -> 256, H W = 272": (1, 16, 17, [(324, 0, 324)], 256, 1, 1, 1, 1, False, None, False, None),
    "1x1, 256 -> 576": (1, 6, 7, [(256, 0, 256)], 576, 1, 1, 1, 0, False, None, False, None),
    "1x5 on W = 4, three aligned slices, sigmoid": (1, 6, 4, [(128, 0, 128), (256, 64, 128), (384, 256, 128)], 128, 1, 5, 1, 2, False, None, False, None),
    "5x1 on H = 3, three slices, one unaligned, tanh": (1, 3, 7, [(128, 0, 128), (256, 128, 128), (130, 2, 128)], 128, 5, 1, 1, 3, False, None, False, None),
    "1x1 stride 2 on 17 x 15, batch norm": (1, 17, 15, [(64, 0, 64)], 96, 1, 1, 2, 0, True, None, False, None),
    "3x3 on a 1 x 1 image, residual + relu": (1, 1, 1, [(128, 0, 128)], 64, 3, 3, 1, 1, False, "given", True, None),
    "3x3 stride 2, batch of 2, batch norm, relu, residual + relu": (2, 9, 11, [(64, 0, 64)], 96, 3, 3, 2, 1, True, "given", True, None),
}


@pytest.mark.parametrize("name", list(CONV_CASES))
def test_convolution_against_f64(hip_lib, name):
    N, H, W, parts, Cout, kh, kw, stride, act, bn, res_kind, res_relu, out_width = CONV_CASES[name]
    seed = sorted(CONV_CASES).index(name) * 10
    bufs = [(_randn(seed + 1 + i, N, H, W, width), off, ch) for i, (width, off, ch) in enumerate(parts)]
    Cin = sum(p[2] for p in parts)
    weight = _randn(seed + 5, Cout, Cin, kh, kw) / np.sqrt(Cin * kh * kw) * 2.0
    bias = 0.3 * _randn(seed + 6, Cout)
    Ho, Wo = (H + 2 * (kh // 2) - kh) // stride + 1, (W + 2 * (kw // 2) - kw) // stride + 1
    residual = _randn(seed + 7, N, Ho, Wo, Cout) if res_kind else None
    out, x, c = _run_conv(hip_lib, bufs, weight, bias, stride, act, _bn(seed + 8, Cout) if bn else None, residual, res_relu, out_width,
                          in_place_residual=res_kind == "in place")
    want, bound = _conv_bound(x, weight, bias, stride, act, c if bn else None, residual)
    if res_relu:
        want = torch.relu(want)
    assert tuple(out.shape[:3]) == (N, Ho, Wo)
    err = (out[..., :Cout].double() - want).abs()
    print(f"{name}: max err / bound = {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert bool((err <= bound).all()), float((err - bound).max())
    if out_width is not None:
        assert bool((out[..., Cout:] == 7.0).all())          # the neighbouring channels of the buffer survive


def test_conv_refuses_what_it_does_not_cover(hip_lib):
    from gaustar_amd._lib import FlowConvDesc
    x = torch.zeros(1, 4, 4, 8, device=DEV)
    d = FlowConvDesc()
    d.N, d.H, d.W, d.KH, d.KW, d.stride, d.n_in, d.Cout = 1, 4, 4, 5, 5, 1, 1, 8
    d.inputs[0] = _slice(x)
    d.out = _slice(x)
    assert hip_lib.gsr_flow_conv(ctypes.addressof(d), None) != 0 and b"1x1, 3x3, 7x7, 1x5 or 5x1" in hip_lib.gsr_last_error()
    d.KH = d.KW = 3
    assert hip_lib.gsr_flow_conv(ctypes.addressof(d), None) != 0 and b"null" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_flow_conv(None, None) != 0


# ------------------------------------------------------------------------------------------------ volume, pyramid, lookup
@pytest.fixture(scope="module")
def pyramid(hip_lib):
    """Feature maps of a 16 x 17 grid, both volumes and the forward pyramid 16 x 17 -> 8 x 8 -> 4 x 4 -> 2 x 2 on the device."""
    h8, w8, C = 16, 17, 256
    P = h8 * w8
    f1, f2 = _randn(101, P, C), _randn(102, P, C)
    d1, d2 = f1.to(DEV), f2.to(DEV)
    packed = torch.empty(C * ((P + 63) // 64 * 64), device=DEV)
    vols = []
    for a, b in ((d1, d2), (d2, d1)):
        vol = torch.empty(P, P, device=DEV)
        assert hip_lib.gsr_flow_pack_features(P, C, b.data_ptr(), packed.data_ptr(), None) == 0
        assert hip_lib.gsr_flow_corr_volume(P, P, C, a.data_ptr(), packed.data_ptr(), vol.data_ptr(), None) == 0, hip_lib.gsr_last_error()
        vols.append(vol)
    levels, (h, w) = [vols[0]], (h8, w8)
    for _ in range(3):
        nxt = torch.empty(P, (h // 2) * (w // 2), device=DEV)
        assert hip_lib.gsr_flow_corr_pool(P, h, w, levels[-1].data_ptr(), nxt.data_ptr(), None) == 0
        levels.append(nxt)
        h, w = h // 2, w // 2
    torch.cuda.synchronize()
    return dict(h8=h8, w8=w8, P=P, f1=f1, f2=f2, vols=vols, levels=levels)


def test_volume_against_f64_and_its_transpose(pyramid):
    """The convolution's bound with K = 256 and no bias, scaled by the exact 1/16; the backward volume, built directly with
    the operands swapped, holds the transpose's bits: the same products in the same order."""
    f1, f2 = pyramid["f1"].double(), pyramid["f2"].double()
    want = f1 @ f2.t() / 16.0
    bound = (256 + 2) * U * (f1.abs() @ f2.abs().t()) / 16.0
    err = (pyramid["vols"][0].cpu().double() - want).abs()
    assert bool((err <= bound).all()), float((err / bound).max())
    assert _bits_equal(pyramid["vols"][1], pyramid["vols"][0].t().contiguous())


def test_pyramid_pools_odd_sizes_floored(pyramid):
    """(((a + b) + c) + d) / 4: three sums, the quarter exact: |err| <= 3 u (|a| + |b| + |c| + |d|) / 4, from the device's own
    finer level."""
    P, dims = pyramid["P"], [(16, 17), (8, 8), (4, 4), (2, 2)]
    for l in range(3):
        (h, w), (h2, w2) = dims[l], dims[l + 1]
        fine = pyramid["levels"][l].cpu().double().reshape(P, h, w)[:, :2 * h2, :2 * w2].reshape(P, h2, 2, w2, 2)
        want, mag = fine.mean((2, 4)), fine.abs().mean((2, 4))
        got = pyramid["levels"][l + 1].cpu().double().reshape(P, h2, w2)
        assert bool(((got - want).abs() <= 3 * U * mag).all())


def _lookup(lib, pyramid, flow):
    h8, w8, P = pyramid["h8"], pyramid["w8"], pyramid["P"]
    buf = torch.zeros(P, 8, device=DEV)
    buf[:, 6:8] = flow.to(DEV)
    out = torch.empty(P, 324, device=DEV)
    fl = _slice(buf, 6, 2)
    rc = lib.gsr_flow_corr_lookup(h8, w8, h8, w8, ctypes.addressof(fl), *(t.data_ptr() for t in pyramid["levels"]), out.data_ptr(), None)
    assert rc == 0, lib.gsr_last_error()
    torch.cuda.synchronize()
    return out.cpu()


def test_lookup_against_f64(hip_lib, pyramid):
    """Flows are multiples of 1/8 below 64 in size, so (grid + flow) / 2^l + d is exact in f32 at every level and so are the
    fractions; what rounds is, per tap, the weight's product and its product with the value, then three sums:
    |err| <= gamma_5 sum|w v| < 6 u sum|w v|.  Coordinates: on integers (flow 0), at -0.5, and beyond every edge of every level
    on each side; the rest random."""
    h8, w8, P = pyramid["h8"], pyramid["w8"], pyramid["P"]
    flow = torch.randint(-64, 65, (P, 2), generator=_gen(7)).float() / 8.0
    ys, xs = torch.meshgrid(torch.arange(h8), torch.arange(w8), indexing="ij")
    grid = torch.stack([xs, ys], -1).reshape(P, 2).float()
    flow[:40] = 0.0                                                            # on integers
    flow[40] = torch.tensor([-0.5, -0.5]) - grid[40]                           # at -0.5
    flow[41] = torch.tensor([-0.5, 3.0]) - grid[41]
    flow[42] = torch.tensor([5.0, -0.5]) - grid[42]
    for k, c in enumerate(((-40.0, 5.0), (60.0, 5.0), (5.0, -40.0), (5.0, 60.0), (-4.5, 7.25), (w8 + 3.5, 2.0), (3.0, h8 + 3.25), (-160.0, 200.0))):
        flow[43 + k] = torch.tensor(c) - grid[43 + k]
    got = _lookup(hip_lib, pyramid, flow).double()
    levels = [t.cpu().double().reshape(P, h, w) for t, (h, w) in zip(pyramid["levels"], [(16, 17), (8, 8), (4, 4), (2, 2)])]
    coords = (grid + flow).double()
    want = flow_ref.lookup(levels, coords)
    mag = flow_ref.lookup([t.abs() for t in levels], coords)
    assert bool(((got - want).abs() <= 6 * U * mag).all())
    assert bool((got[43:47] == 0).all()) and bool((got[50] == 0).all())         # wholly outside every level: zeros
    assert float(got[:40].abs().max()) > 0


def test_lookup_window_order(hip_lib, pyramid):
    """Channel 9 i + j samples at (x + d_i, y + d_j): on level-0 maps that hold their x coordinate, the first index moves the value."""
    h8, w8, P = pyramid["h8"], pyramid["w8"], pyramid["P"]
    ramp = torch.arange(w8, dtype=torch.float32)[None, None, :].expand(P, h8, w8).reshape(P, -1).contiguous().to(DEV)
    fake = dict(pyramid, levels=[ramp, *pyramid["levels"][1:]])
    out = _lookup(hip_lib, fake, torch.zeros(P, 2))
    p = 8 * w8 + 8                                                               # pixel (x 8, y 8): the window 4..12 lies inside
    win = out[p, :81].reshape(9, 9)
    assert torch.equal(win[:, 0], torch.arange(4, 13, dtype=torch.float32)) and torch.equal(win[:, 5], win[:, 0])


# ------------------------------------------------------------------------------------------------ the small kernels
@pytest.mark.parametrize("C,relu,with_residual", [(64, True, False), (96, True, True), (128, False, False)])
def test_instance_norm_against_f64(hip_lib, C, relu, with_residual):
    """Two images of 300 pixels (two chunks, the second short) with different means and spreads: they must not mix.  The sums
    are f64 (their error is far below u); mean and rstd are rounded to f32 once each, then y = (x - mean) rstd rounds twice:
    |err| <= u (rstd |mean| + 3 |y|) < 4 u (|y| + rstd |mean|); relu is exact; the residual's sum adds u |res + y|."""
    N, HW = 2, 300
    x = _randn(200 + C, N, HW, C) * torch.tensor([1.0, 5.0])[:, None, None] + torch.tensor([3.0, -20.0])[:, None, None]
    res = _randn(300 + C, N, HW, C) if with_residual else None
    dx, out = x.to(DEV), torch.empty(N, HW, C, device=DEV)
    ws = torch.empty(hip_lib.gsr_flow_instance_norm_workspace_bytes(N, HW, C), dtype=torch.uint8, device=DEV)
    dres = res.to(DEV) if with_residual else None
    rc = hip_lib.gsr_flow_instance_norm(N, HW, C, dx.data_ptr(), int(relu), None if dres is None else dres.data_ptr(), out.data_ptr(),
                                        ws.data_ptr(), None)
    assert rc == 0, hip_lib.gsr_last_error()
    torch.cuda.synchronize()
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    rstd = 1.0 / torch.sqrt(((xd - mean) ** 2).mean(1, keepdim=True) + 1e-5)
    y = (xd - mean) * rstd
    bound = 4 * U * (y.abs() + rstd * mean.abs())
    if relu:
        y = torch.relu(y)
    if with_residual:
        y = torch.relu(res.double() + y)
        bound = bound + U * y.abs()
    assert bool(((out.cpu().double() - y).abs() <= bound).all())


def test_gru_combine_against_f64(hip_lib):
    """r h rounds once: u |r h|.  (1 - z) h + z q: the difference, two products, one sum: 3 u (|(1 - z) h| + |z q|).  Slices
    of wider buffers; h is updated in place."""
    P, C = 301, 128
    zr, hx, q = torch.rand(P, 256, generator=_gen(1)), _randn(2, P, 384), _randn(3, P, 128).tanh()
    dzr, dhx, dq, drh = zr.to(DEV), hx.to(DEV), q.to(DEV), torch.empty(P, C, device=DEV)
    zs, rs, hs, qs, rhs = _slice(dzr, 0, C), _slice(dzr, C, C), _slice(dhx, 0, C), _slice(dq), _slice(drh)
    a = ctypes.addressof
    assert hip_lib.gsr_flow_gru_combine(P, 0, a(rs), a(hs), None, a(rhs), None) == 0, hip_lib.gsr_last_error()
    assert hip_lib.gsr_flow_gru_combine(P, 1, a(zs), a(hs), a(qs), a(hs), None) == 0, hip_lib.gsr_last_error()
    torch.cuda.synchronize()
    z, r, h, qd = zr[:, :C].double(), zr[:, C:].double(), hx[:, :C].double(), q.double()
    assert bool(((drh.cpu().double() - r * h).abs() <= U * (r * h).abs()).all())
    want = (1 - z) * h + z * qd
    assert bool(((dhx.cpu()[:, :C].double() - want).abs() <= 3 * U * (((1 - z) * h).abs() + (z * qd).abs())).all())
    assert torch.equal(dhx.cpu()[:, C:], hx[:, C:])                              # the rest of the buffer is untouched


def test_upsample_against_f64(hip_lib):
    """Per output: logits l_k = mask / 4 (exact), d_k = l_k - max (one rounding: the exponential's argument is off by u |d_k|),
    e_k = expf(d_k) within 2 ulp = 4 u, their sum over 9 (8 roundings), w_k = e_k / sum (1), w_k (8 flow) (1), summed over 9
    (8): relative to sum_k |w_k 8 flow_k| at most (2 (4 + D) + 8 + 1 + 1 + 8) u = (26 + 2 D) u, D = max_k |d_k|."""
    h8, w8, h, w, pt, pl = 16, 17, 125, 134, 1, 1
    P = h8 * w8
    mask = 6.0 * _randn(5, P, 576)
    buf = torch.zeros(P, 128)
    buf[:, 126:] = 3.0 * _randn(6, P, 2)
    dm, db, out = mask.to(DEV), buf.to(DEV), torch.empty(h, w, 2, device=DEV)
    fl = _slice(db, 126, 2)
    rc = hip_lib.gsr_flow_upsample(h8, w8, ctypes.addressof(fl), dm.data_ptr(), pt, pl, h, w, out.data_ptr(), None)
    assert rc == 0, hip_lib.gsr_last_error()
    torch.cuda.synchronize()
    logits = 0.25 * mask.double().t().reshape(9, 8, 8, h8, w8)
    wgt = torch.softmax(logits, 0)
    D = (logits.max(0).values - logits.min(0).values)                          # [i, j, y, x]
    f8 = F.pad(8 * buf[:, 126:].double().t().reshape(2, h8, w8), (1, 1, 1, 1))
    nb = torch.stack([f8[:, ky:ky + h8, kx:kx + w8] for ky in range(3) for kx in range(3)], 1)
    up = (wgt[None] * nb[:, :, None, None]).sum(1).permute(3, 1, 4, 2, 0).reshape(8 * h8, 8 * w8, 2)
    mag = (wgt[None] * nb[:, :, None, None].abs()).sum(1).permute(3, 1, 4, 2, 0).reshape(8 * h8, 8 * w8, 2)
    Dp = D.permute(2, 0, 3, 1).reshape(8 * h8, 8 * w8, 1)
    crop = lambda t: t[pt:pt + h, pl:pl + w]
    err = (out.cpu().double() - crop(up)).abs()
    assert bool((err <= (26 + 2 * crop(Dp)) * U * crop(mag)).all())


@pytest.mark.parametrize("factor,h,w", [(1, 125, 134), (2, 250, 268), (4, 252, 272), (2, 256, 14)])
def test_image_preparation(hip_lib, factor, h, w):
    """The integers (box mean half to even, replicate padding split pad//2 before) are exact: they are recovered from the
    result.  The value 2 (s / 255) - 1: the quotient within 2.5 ulp = 5 u, doubled exactly, one more rounding for the sum."""
    img = torch.randint(0, 256, (h, w, 3), generator=_gen(h + factor), dtype=torch.uint8)
    if factor > 1:
        img[:factor, :factor] = torch.tensor([[2, 0], [0, 0]] if factor == 2 else [[8] + [0] * 3] + [[0] * 4] * 3, dtype=torch.uint8)[..., None]   # .5 -> 0
    want = flow_ref.prep_image(img.numpy(), factor, torch.float64)
    out = torch.empty(*want.shape, device=DEV)
    assert hip_lib.gsr_flow_prep_image(h, w, img.to(DEV).data_ptr(), factor, out.data_ptr(), None) == 0, hip_lib.gsr_last_error()
    torch.cuda.synchronize()
    got = out.cpu().double()
    assert torch.equal(torch.round((got + 1.0) * 127.5), torch.round((want + 1.0) * 127.5))
    assert bool(((got - want).abs() <= 5 * U * (want + 1.0).abs() + U * want.abs()).all())


# ------------------------------------------------------------------------------------------------ the whole model
@pytest.fixture(scope="module")
def kat():
    return dict(np.load(os.path.join(GOLDEN_DIR, "flow", "flow_kat.npz")))


@pytest.fixture(scope="module")
def weights(hip_lib):
    from gaustar_amd import flow
    return {g: flow.RaftWeights.from_state_dict(flow_ref.seeded_state_dict(g), DEV) for g in (0.6, 1.0)}


@pytest.mark.parametrize("case", ["A", "B"])
def test_whole_model_against_f64(kat, weights, case):
    """Per stage k: max|gpu - ref64| <= 4 max(D_k, s_k), D_k = max|fixture - ref64| the reference's own f32 distance from the
    f64 model and s_k its sensitivity to 2^-23 in every weight.  The device runs the reference's precision in other summation
    orders: a k-ordered chain of up to 2 304 products where the host sums blocked partials, whose error constant is up to
    about 3 times a blocked sum's; hence the 4.
    Measured on an MI355X (px): see NOTEBOOK.md."""
    from gaustar_amd import flow
    gain = float(kat[f"{case}_gain"])
    im1, im2 = kat[f"{case}_image1"], kat[f"{case}_image2"]
    ref = flow_ref.raft(flow_ref.seeded_state_dict(gain), im1, im2, iters=20, stages=STAGES, dtype=torch.float64)
    model = flow.RaftFlow(weights[gain], iters=20)
    outs = model(im1, im2, factor=1, stages=STAGES)
    assert len(outs) == 3
    failures = []
    for k, got in zip(STAGES, outs):
        assert tuple(got.shape) == (125, 134, 2) and got.dtype == torch.float32 and got.device == DEV
        r = ref[k].numpy()
        D = float(np.abs(kat[f"{case}_flow_{k}"].astype(np.float64) - r).max())
        s = float(kat[f"{case}_s_{k}"])
        G = float(np.abs(got.cpu().numpy().astype(np.float64) - r).max())
        print(f"case {case} k={k}: device {G:.3e}  D_k {D:.3e}  s_k {s:.3e}  bound {4 * max(D, s):.3e}")
        if not G <= 4.0 * max(D, s):
            failures.append((k, G, D, s))
    assert not failures, failures


@pytest.fixture(scope="module")
def short_model(weights):
    from gaustar_amd import flow
    return flow.RaftFlow(weights[0.6], iters=3)


def test_pair_and_repeats_are_bit_equal(kat, short_model):
    im1, im2 = kat["A_image1"], kat["A_image2"]
    f, b = short_model.pair(im1, im2, factor=1)
    one, back = short_model(im1, im2, factor=1), short_model(im2, im1, factor=1)
    assert _bits_equal(f, one) and _bits_equal(b, back)
    assert _bits_equal(one, short_model(torch.from_numpy(im1).to(DEV), torch.from_numpy(im2).to(DEV), factor=1))
    assert not _bits_equal(f, b) and bool(torch.isfinite(f).all())
    side = torch.cuda.Stream(DEV)
    with torch.cuda.stream(side):
        other = short_model(im1, im2, factor=1)
    side.synchronize()
    assert _bits_equal(one, other)
    n = len(short_model._work)                                                  # one workspace per (shape, stream), reused
    assert n >= 2 and _bits_equal(one, short_model(im1, im2, factor=1)) and len(short_model._work) == n


def _smooth_u8(seed, h, w):
    base = torch.rand(1, 3, h // 8 + 2, w // 8 + 2, generator=_gen(seed))
    return (F.interpolate(base, size=(h, w), mode="bicubic", align_corners=True).clamp(0, 1)[0] * 255).round().to(torch.uint8).permute(1, 2, 0).contiguous()


def test_flow_frames_feeds_the_warp_with_the_same_bits(short_model):
    """warp.warp_mesh over flows made on the device, views in flight 2, against the same flows passed as host arrays."""
    import test_gpu_warp as tw
    from gaustar_amd import flow, warp
    rig = tw._small_rig(n_azim=2)
    C = len(rig["shape"])
    H, W = (int(x) for x in rig["shape"][0])
    fr = tw._frames(rig)
    cur = [_smooth_u8(10 + i, H, W).numpy() for i in range(C)]
    nxt = [np.roll(c, (2, -3), (0, 1)) for c in cur]
    dc, dn = [f[2] for f in fr], [f[3] for f in fr]
    v, f = tw._mesh(2)
    live = warp.warp_mesh(v, tw._faces_t(f), rig, flow.flow_frames(cur, nxt, dc, dn, short_model), views_in_flight=2, return_stages=True)
    host = [tuple(t.cpu().numpy() for t in short_model.pair(cur[i], nxt[i])) for i in range(C)]
    assert host[0][0].shape == (H // 2, W // 2, 2)
    again = warp.warp_mesh(v, tw._faces_t(f), rig, lambda i: (host[i][0], host[i][1], dc[i], dn[i]), views_in_flight=1, return_stages=True)
    for name in ("table", "move_raw", "verts_smoothed", "count"):
        assert _bits_equal(getattr(live, name), getattr(again, name)), name


def test_write_flows_files(tmp_path, kat, weights):
    from gaustar_amd import flow, formats, warp
    root = str(tmp_path)
    eye = np.eye(4)[None].repeat(2, 0)
    np.savez(os.path.join(root, "rgb_cameras.npz"), intrinsics=np.array([[[300.0, 0, 67], [0, 300.0, 62.5], [0, 0, 1]]] * 2), extrinsics=eye,
             shape=np.array([[128, 136]] * 2))
    images = {}
    for f in (0, 1):
        os.makedirs(os.path.join(root, f"{f:04d}", "images"))
        for c in (0, 1):
            images[f, c] = _smooth_u8(100 + 2 * c, 144, 152).numpy()[3 * f:3 * f + 128, 2 * f:2 * f + 136].copy()
            formats.save_png_rgb8(os.path.join(root, f"{f:04d}", "images", f"img_{c:04d}.png"), images[f, c])
    paths = flow.write_flows(root, 0, 2, 1, weights[0.6], factor=1, views_in_flight=2, rank=0, world=1, iters=2)
    out_dir = os.path.join(root, "0000", warp.FLOW_DIRS[1])
    assert sorted(os.listdir(out_dir)) == ["0000_b.npz", "0000_f.npz", "0001_b.npz", "0001_f.npz"]      # no pad.txt, no preview
    assert sorted(paths) == sorted(os.path.join(out_dir, n) for n in os.listdir(out_dir))
    assert not os.path.exists(os.path.join(root, "0001", warp.FLOW_DIRS[1]))
    first = {n: np.load(os.path.join(out_dir, n)) for n in os.listdir(out_dir)}
    model = flow.RaftFlow(weights[0.6], iters=2)
    for c in (0, 1):
        ff, fb = model.pair(images[0, c], images[1, c], factor=1)
        for tag, t in (("f", ff), ("b", fb)):
            z = first[f"{c:04d}_{tag}.npz"]
            assert z.files == ["flow"] and z["flow"].shape == (128, 136, 2) and z["flow"].dtype == np.float32
            assert z["flow"].tobytes() == t.cpu().numpy().tobytes()
    flow.write_flows(root, 0, 2, 1, weights[0.6], factor=1, views_in_flight=1, rank=0, world=1, iters=2)
    for n, z in first.items():
        assert np.load(os.path.join(out_dir, n))["flow"].tobytes() == z["flow"].tobytes()          # views in flight 1 against 2


def test_refusals_come_before_any_launch(weights):
    from gaustar_amd import flow
    model = flow.RaftFlow(weights[0.6], iters=2)
    ok = np.zeros((128, 136, 3), np.uint8)
    bad = [((ok.astype(np.float32), ok), 1, "uint8"),
           ((np.zeros((128, 136, 4), np.uint8), ok), 1, r"\[H,W,3\]"),
           ((np.zeros((128, 136), np.uint8), ok), 1, r"\[H,W,3\]"),
           ((torch.from_numpy(ok), ok), 1, "is on cpu"),
           (([[0]], ok), 1, "numpy array or a torch tensor"),
           ((ok, np.zeros((136, 136, 3), np.uint8)), 1, "one shape"),
           ((np.zeros((258, 272, 3), np.uint8),) * 2, 4, "not divisible"),
           ((ok, ok), 3, "factor must be 1, 2 or 4"),
           ((np.zeros((120, 400, 3), np.uint8),) * 2, 1, "under 128"),
           ((np.zeros((256, 240, 3), np.uint8),) * 2, 2, "under 128")]
    for images, factor, match in bad:
        with pytest.raises(ValueError, match=match):
            model(*images, factor=factor)
        with pytest.raises(ValueError, match=match):
            model.pair(*images, factor=factor)
    tight = flow.RaftFlow(weights[0.6], iters=2, max_volume_bytes=model.volume_bytes(128, 136, 1) - 1)
    with pytest.raises(ValueError, match="max_volume_bytes"):
        tight(ok, ok, factor=1)
    assert not model._work and not tight._work                                 # no workspace was made: nothing was launched
    assert model.volume_bytes(128, 136, 1) == 4 * 272 * (272 + 64 + 16 + 4)
    with pytest.raises(ValueError):
        flow.RaftFlow(weights[0.6], iters=0)
    with pytest.raises(ValueError):
        flow.RaftWeights.from_state_dict(flow_ref.seeded_state_dict(1.0), "cpu")
