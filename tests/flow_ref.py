"""A plain-torch restatement of RAFT's basic model at inference (gaustar_amd.flow, csrc/gsr_flow.hip), in this project's own
words: functions over the state dict, no modules.  The dtype is a parameter: f64 on the host is the yardstick of the tests,
f32 on the device (torch's own convolutions) the timing baseline of tools/bench_flow.py.  Also the seeded weights the
parity tests run with: no weight file is committed."""
from __future__ import annotations

import zlib

import numpy as np
import torch
import torch.nn.functional as F

from gaustar_amd.flow import BN_EPS, CONTEXT, HIDDEN, expected_shapes, pad_split

RADIUS, LEVELS = 4, 4


# ------------------------------------------------------------------------------------------------ weights
def seeded_state_dict(gain: float) -> dict:
    """The basic model's state dict (no `module.` prefix, no num_batches_tracked), every tensor from a generator seeded by the
    CRC32 of its key: convolution weights normal x gain / sqrt(fan_in); convolution biases, batch-norm biases and running
    means normal x 0.05; batch-norm weights uniform in [0.8, 1.2]; running variances uniform in [0.5, 1.5].  A strided
    block's `downsample.1` is its `norm3` (one module under two names in the reference)."""
    sd = {}
    for key, shape in expected_shapes().items():
        g = torch.Generator().manual_seed(zlib.crc32(key.replace("downsample.1", "norm3").encode()))
        if len(shape) == 4:
            t = torch.randn(shape, generator=g, dtype=torch.float64) * (float(gain) / np.sqrt(shape[1] * shape[2] * shape[3]))
        elif key.endswith("running_var"):
            t = 0.5 + torch.rand(shape, generator=g, dtype=torch.float64)
        elif key.endswith(".weight"):
            t = 0.8 + 0.4 * torch.rand(shape, generator=g, dtype=torch.float64)
        else:
            t = 0.05 * torch.randn(shape, generator=g, dtype=torch.float64)
        sd[key] = t.to(torch.float32)
    return sd


# ------------------------------------------------------------------------------------------------ image preparation
def box_mean(img: np.ndarray, factor: int) -> np.ndarray:
    """u8 [h,w,3] -> u8 [h/factor, w/factor, 3]: the mean over factor x factor boxes, rounded half to even in integers."""
    h, w, _ = img.shape
    n = factor * factor
    s = img.astype(np.int64).reshape(h // factor, factor, w // factor, factor, 3).sum((1, 3))
    q, r = np.divmod(s, n)
    up = (2 * r > n) | ((2 * r == n) & (q % 2 == 1))
    return (q + up).astype(np.uint8)


def prep_image(img: np.ndarray, factor: int, dtype=torch.float64) -> torch.Tensor:
    """u8 [h,w,3] -> [Hp,Wp,3]: box mean, replicate padding to a multiple of 8 split pad//2 before, 2 (x / 255) - 1."""
    small = box_mean(np.asarray(img), factor)
    padded = np.pad(small, (pad_split(small.shape[0]), pad_split(small.shape[1]), (0, 0)), mode="edge")
    return 2.0 * (torch.from_numpy(padded).to(dtype) / 255.0) - 1.0


# ------------------------------------------------------------------------------------------------ layers (NCHW)
def conv(sd, name, x, stride=1):
    w, b = sd[name + ".weight"], sd[name + ".bias"]
    return F.conv2d(x, w, b, stride=stride, padding=(w.shape[2] // 2, w.shape[3] // 2))


def batch_norm(sd, name, x):
    scale = sd[name + ".weight"] / torch.sqrt(sd[name + ".running_var"] + BN_EPS)
    return (x - sd[name + ".running_mean"][None, :, None, None]) * scale[None, :, None, None] + sd[name + ".bias"][None, :, None, None]


def instance_norm(x):
    mean = x.mean((2, 3), keepdim=True)
    var = ((x - mean) ** 2).mean((2, 3), keepdim=True)
    return (x - mean) / torch.sqrt(var + 1e-5)


def encoder(sd, p, x, batch: bool):
    """The residual encoder: 7x7 stride 2, three pairs of blocks (64, 96 and 128 channels; the last two pairs halve), 1x1."""
    norm = (lambda name, t: batch_norm(sd, name, t)) if batch else (lambda name, t: instance_norm(t))
    x = torch.relu(norm(f"{p}.norm1", conv(sd, f"{p}.conv1", x, 2)))
    for li in (1, 2, 3):
        for bi in (0, 1):
            b = f"{p}.layer{li}.{bi}"
            s = 2 if (bi == 0 and li > 1) else 1
            y = torch.relu(norm(f"{b}.norm1", conv(sd, f"{b}.conv1", x, s)))
            y = torch.relu(norm(f"{b}.norm2", conv(sd, f"{b}.conv2", y)))
            if s == 2:
                x = norm(f"{b}.downsample.1", conv(sd, f"{b}.downsample.0", x, 2))
            x = torch.relu(x + y)
    return conv(sd, f"{p}.conv2", x)


def correlation_pyramid(f1, f2):
    """f1, f2 [1,C,h,w] -> levels [P,hl,wl]: all-pairs dot products over sqrt(C), then three 2 x 2 means (odd sizes floored)."""
    _, C, h, w = f1.shape
    vol = (f1.reshape(C, h * w).t() @ f2.reshape(C, h * w)) / np.sqrt(C)
    levels = [vol.reshape(h * w, h, w)]
    for _ in range(LEVELS - 1):
        levels.append(F.avg_pool2d(levels[-1][:, None], 2, stride=2)[:, 0])
    return levels


def sample_zero(level, sx, sy):
    """level [P,hl,wl], sx, sy [P,...] -> bilinear samples, taps outside the map counting 0."""
    P, hl, wl = level.shape
    x0, y0 = torch.floor(sx), torch.floor(sy)
    ax, ay = sx - x0, sy - y0
    flat = level.reshape(P, hl * wl)
    out = torch.zeros_like(sx)
    for dy, wy in ((0, 1 - ay), (1, ay)):
        for dx, wx in ((0, 1 - ax), (1, ax)):
            xi, yi = (x0 + dx).long(), (y0 + dy).long()
            ok = (xi >= 0) & (xi < wl) & (yi >= 0) & (yi < hl)
            idx = (yi.clamp(0, hl - 1) * wl + xi.clamp(0, wl - 1)).reshape(P, -1)
            v = torch.gather(flat, 1, idx).reshape(sx.shape)
            out = out + torch.where(ok, v, torch.zeros_like(v)) * (wx * wy)
    return out


def lookup(levels, coords):
    """coords [P,2] (x, y) -> [P,324]: per level l the 9 x 9 window around coords / 2^l; channel 81 l + 9 i + j samples at
    (x + d_i, y + d_j), d = -4..4: the FIRST window index moves x (the reference stacks (dy, dx) onto (x, y))."""
    d = torch.arange(-RADIUS, RADIUS + 1, dtype=coords.dtype, device=coords.device)
    out = []
    for l, level in enumerate(levels):
        cx, cy = coords[:, 0] / 2 ** l, coords[:, 1] / 2 ** l
        sx = (cx[:, None, None] + d[None, :, None]).expand(-1, 9, 9)
        sy = (cy[:, None, None] + d[None, None, :]).expand(-1, 9, 9)
        out.append(sample_zero(level, sx, sy).reshape(-1, 81))
    return torch.cat(out, 1)


def update(sd, net, inp, corr, flow):
    """One step of the update block: motion encoder, the separable GRU, the flow head.  -> (net, delta_flow)"""
    u = "update_block"
    cor = torch.relu(conv(sd, f"{u}.encoder.convc1", corr))
    cor = torch.relu(conv(sd, f"{u}.encoder.convc2", cor))
    flo = torch.relu(conv(sd, f"{u}.encoder.convf1", flow))
    flo = torch.relu(conv(sd, f"{u}.encoder.convf2", flo))
    out = torch.relu(conv(sd, f"{u}.encoder.conv", torch.cat([cor, flo], 1)))
    x = torch.cat([inp, out, flow], 1)
    for half in ("1", "2"):
        hx = torch.cat([net, x], 1)
        z = torch.sigmoid(conv(sd, f"{u}.gru.convz{half}", hx))
        r = torch.sigmoid(conv(sd, f"{u}.gru.convr{half}", hx))
        q = torch.tanh(conv(sd, f"{u}.gru.convq{half}", torch.cat([r * net, x], 1)))
        net = (1 - z) * net + z * q
    delta = conv(sd, f"{u}.flow_head.conv2", torch.relu(conv(sd, f"{u}.flow_head.conv1", net)))
    return net, delta


def upsample(sd, net, flow):
    """The mask head and the convex combination: flow [1,2,h8,w8] -> [8 h8, 8 w8, 2]."""
    u = "update_block"
    mask = 0.25 * conv(sd, f"{u}.mask.2", torch.relu(conv(sd, f"{u}.mask.0", net)))
    _, _, h, w = flow.shape
    wgt = torch.softmax(mask.reshape(9, 8, 8, h, w), 0)                       # [k, i, j, y, x]
    f8 = F.pad(8 * flow[0], (1, 1, 1, 1))                                     # [2, h + 2, w + 2]
    nb = torch.stack([f8[:, ky:ky + h, kx:kx + w] for ky in range(3) for kx in range(3)], 1)   # [2, k, y, x]
    up = (wgt[None] * nb[:, :, None, None]).sum(1)                            # [2, i, j, y, x]
    return up.permute(3, 1, 4, 2, 0).reshape(8 * h, 8 * w, 2)


@torch.no_grad()
def raft(sd, image1, image2, iters=20, factor=1, dtype=torch.float64, stages=(), device="cpu") -> dict:
    """u8 images [h,w,3] -> {k: flow_up [h/factor, w/factor, 2] after k iterations} for k in stages and k = iters."""
    sd = {k: v.to(device=device, dtype=dtype) for k, v in sd.items()}
    im = [prep_image(i, factor, dtype).to(device).permute(2, 0, 1)[None] for i in (image1, image2)]
    hs, ws = image1.shape[0] // factor, image1.shape[1] // factor
    pt, pl = pad_split(hs)[0], pad_split(ws)[0]
    f1, f2 = encoder(sd, "fnet", torch.cat(im, 0), False).split(1, 0)
    levels = correlation_pyramid(f1, f2)
    c = encoder(sd, "cnet", im[0], True)
    net, inp = torch.tanh(c[:, :HIDDEN]), torch.relu(c[:, HIDDEN:HIDDEN + CONTEXT])
    _, _, h8, w8 = f1.shape
    gy, gx = torch.meshgrid(torch.arange(h8, dtype=dtype, device=device), torch.arange(w8, dtype=dtype, device=device), indexing="ij")
    grid = torch.stack([gx, gy], 0)[None]
    flow = torch.zeros_like(grid)
    out = {}
    for k in range(1, iters + 1):
        coords = (grid + flow)[0].reshape(2, -1).t()
        corr = lookup(levels, coords).t().reshape(1, -1, h8, w8)
        net, delta = update(sd, net, inp, corr, flow)
        flow = flow + delta
        if k == iters or k in stages:
            out[k] = upsample(sd, net, flow)[pt:pt + hs, pl:pl + ws].contiguous()
    return out
