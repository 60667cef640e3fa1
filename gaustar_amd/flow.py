"""RAFT optical flow on the GPU: the flows `warp.warp_mesh_using_flow` reads, from this package alone.

The reference makes `{f:04d}/flow_bi[_2f]/{c:04d}_{f,b}.npz` with data_process/RAFT/demo_GauSTAR.py (its own torch-1.6
environment, cv2, a CUDA extension): the basic model, 20 iterations, images at half resolution.  Here the same inference is
a string of hand-written HIP kernels (csrc/gsr_flow.hip, rules in include/gsr.h, restated in tests/flow_ref.py):

    weights = RaftWeights.load("raft-things.pth", "cuda")        # the checkpoint the reference's README names; not shipped
    model = RaftFlow(weights, iters=20)
    flow = model(image1, image2, factor=2)                        # u8 [H,W,3] x 2 -> f32 [H/2,W/2,2] in (x, y) order
    flow_f, flow_b = model.pair(image1, image2, factor=2)         # both directions, the feature encoder run once
    frames = flow_frames(images_cur, images_next, depth_cur, depth_next, model)   # what warp.warp_mesh takes; nothing leaves the GPU
    write_flows(data_root, 0, 10, 1, weights)                     # the reference's files
    python -m gaustar_amd.flow DATA_ROOT --model raft-things.pth --frame_0 0 --frame_end 10

What to know:
  * `factor` is an exact box mean (1, 2 or 4), rounded half to even in integers as cv2's INTER_AREA does; parity with cv2
    itself is not pinned (it is not a dependency);
  * the flow is kept as a flow, not as the difference of two coordinate grids: grid + flow is rounded once per lookup, which
    is closer to the f64 model than the reference's f32 run;
  * the backward volume is built directly with the operands swapped: the same products in the same order, so it holds the
    transpose's bits;
  * write_flows writes no pad.txt (nothing is cropped) and no preview JPEG;
  * results are bit-reproducible across calls, streams and views in flight: no atomics, fixed orders.
"""
from __future__ import annotations

import ctypes
import os
import threading
from typing import Callable, Dict, List, Optional, Tuple

import numpy as np
import torch

from . import _host, _lib
from ._lib import FlowConvDesc, FlowSlice

HIDDEN = 128            # raft.py:36-37: hidden and context dimensions of the basic model
CONTEXT = 128
FEATURES = 256          # raft.py:54
LEVELS, RADIUS = 4, 4   # raft.py:38-39
CORR_CH = LEVELS * (2 * RADIUS + 1) ** 2
MASK_CH = 64 * 9
MIN_SIDE = 128          # a padded side below this leaves the coarsest level one wide, where the reference divides by zero
BN_EPS = 1e-5
ACT_NONE, ACT_RELU, ACT_SIGMOID, ACT_TANH = range(4)


# ------------------------------------------------------------------------------------------------ the checkpoint
def _encoder_shapes(prefix: str, out_dim: int, batch_norm: bool) -> Dict[str, tuple]:
    s: Dict[str, tuple] = {}

    def conv(name, co, ci, kh, kw):
        s[f"{prefix}.{name}.weight"] = (co, ci, kh, kw)
        s[f"{prefix}.{name}.bias"] = (co,)

    def bn(name, c):
        if batch_norm:
            for k in ("weight", "bias", "running_mean", "running_var"):
                s[f"{prefix}.{name}.{k}"] = (c,)

    conv("conv1", 64, 3, 7, 7)
    bn("norm1", 64)
    cin = 64
    for li, dim in enumerate((64, 96, 128), start=1):
        for bi in range(2):
            b = f"layer{li}.{bi}"
            strided = bi == 0 and li > 1
            conv(f"{b}.conv1", dim, cin, 3, 3)
            conv(f"{b}.conv2", dim, dim, 3, 3)
            bn(f"{b}.norm1", dim)
            bn(f"{b}.norm2", dim)
            if strided:
                conv(f"{b}.downsample.0", dim, cin, 1, 1)
                bn(f"{b}.norm3", dim)
                bn(f"{b}.downsample.1", dim)
            cin = dim
    conv("conv2", out_dim, 128, 1, 1)
    return s


def expected_shapes() -> Dict[str, tuple]:
    """Key -> shape of the basic model's state dict (without the `module.` prefix and without BatchNorm's
    `num_batches_tracked` counters, which are accepted and ignored)."""
    s = _encoder_shapes("fnet", FEATURES, False)
    s.update(_encoder_shapes("cnet", HIDDEN + CONTEXT, True))
    u = "update_block"
    for name, (co, ci, kh, kw) in {
            "encoder.convc1": (256, CORR_CH, 1, 1), "encoder.convc2": (192, 256, 3, 3), "encoder.convf1": (128, 2, 7, 7),
            "encoder.convf2": (64, 128, 3, 3), "encoder.conv": (HIDDEN - 2, 256, 3, 3),
            "gru.convz1": (HIDDEN, 384, 1, 5), "gru.convr1": (HIDDEN, 384, 1, 5), "gru.convq1": (HIDDEN, 384, 1, 5),
            "gru.convz2": (HIDDEN, 384, 5, 1), "gru.convr2": (HIDDEN, 384, 5, 1), "gru.convq2": (HIDDEN, 384, 5, 1),
            "flow_head.conv1": (256, HIDDEN, 3, 3), "flow_head.conv2": (2, 256, 3, 3),
            "mask.0": (256, HIDDEN, 3, 3), "mask.2": (MASK_CH, 256, 1, 1)}.items():
        s[f"{u}.{name}.weight"] = (co, ci, kh, kw)
        s[f"{u}.{name}.bias"] = (co,)
    return s


def check_state_dict(sd) -> Dict[str, torch.Tensor]:
    """The reference's basic-model state dict with the `module.` prefix of DataParallel removed, every key and shape checked.
    ValueError names the first mismatch; a --small checkpoint is refused as such."""
    if not hasattr(sd, "items"):
        raise ValueError("a state dict (key -> tensor) is needed")
    sd = {(k[7:] if k.startswith("module.") else k): v for k, v in sd.items()}
    w = sd.get("fnet.conv1.weight")
    if "update_block.gru.convz.weight" in sd or (w is not None and tuple(w.shape)[:1] == (32,)):
        raise ValueError("this is a --small RAFT checkpoint; only the basic model (raft-things.pth and its kin) is implemented")
    want = expected_shapes()
    for k, shape in want.items():
        if k not in sd:
            raise ValueError(f"state dict: key {k!r} is missing")
        if not isinstance(sd[k], torch.Tensor) or tuple(sd[k].shape) != shape:
            got = tuple(sd[k].shape) if hasattr(sd[k], "shape") else type(sd[k]).__name__
            raise ValueError(f"state dict: {k!r} must have shape {shape}, got {got}")
        if not sd[k].dtype.is_floating_point:
            raise ValueError(f"state dict: {k!r} must be floating point, got {sd[k].dtype}")
    for k in sd:
        if k not in want and not k.endswith(".num_batches_tracked"):
            raise ValueError(f"state dict: unexpected key {k!r}")
    return {k: sd[k] for k in want}


def pad_split(n: int) -> Tuple[int, int]:
    """(before, after) of the padding that brings n up to a multiple of 8: InputPadder's 'sintel' split (utils/utils.py:11-14)."""
    pad = (8 - int(n) % 8) % 8
    return pad // 2, pad - pad // 2


class _Conv:
    """One convolution's packed operands on the device: weights [Kpad][Npad] with row (ky KW + kx) Cin + ci, bias, and the
    eval-mode batch norm that follows it as scale / shift."""

    def __init__(self, lib, weight: torch.Tensor, bias: torch.Tensor, device, bn=None):
        co, ci, kh, kw = (int(x) for x in weight.shape)
        self.Cout, self.Cin, self.KH, self.KW = co, ci, kh, kw
        K = kh * kw * ci
        Kp, Np = int(lib.gsr_flow_packed_k(K)), int(lib.gsr_flow_packed_n(co))
        packed = torch.zeros(Kp, Np, dtype=torch.float32)
        packed[:K, :co] = weight.detach().to(torch.float32).cpu().permute(2, 3, 1, 0).reshape(K, co)
        self.w = packed.to(device)
        self.b = bias.detach().to(torch.float32).cpu().contiguous().to(device)
        self.scale = self.shift = None
        if bn is not None:
            g, b, mean, var = (t.detach().cpu().to(torch.float64) for t in bn)
            scale = g / torch.sqrt(var + BN_EPS)
            self.scale = scale.to(torch.float32).to(device)
            self.shift = (b - mean * scale).to(torch.float32).to(device)


class RaftWeights:
    """The basic model's weights, repacked once for the kernels.  z and r of each GRU half share their input and are one
    convolution of 256 outputs; the context encoder's last convolution is split into its tanh and its relu half."""

    def __init__(self, sd: Dict[str, torch.Tensor], device):
        self.device = _host.resolve_device(device, what="gaustar_amd.flow", exc=ValueError)
        lib = _lib.load()
        dev = self.device

        def conv(name, rows=None, bn=None):
            w, b = sd[f"{name}.weight"], sd[f"{name}.bias"]
            if rows is not None:
                w, b = w[rows], b[rows]
            bnp = None if bn is None else tuple(sd[f"{bn}.{k}"] for k in ("weight", "bias", "running_mean", "running_var"))
            return _Conv(lib, w, b, dev, bnp)

        def encoder(p, batch_norm):
            e = {"conv1": conv(f"{p}.conv1", bn=f"{p}.norm1" if batch_norm else None), "blocks": []}
            for li in (1, 2, 3):
                for bi in (0, 1):
                    b = f"{p}.layer{li}.{bi}"
                    strided = bi == 0 and li > 1
                    e["blocks"].append({
                        "stride": 2 if strided else 1,
                        "conv1": conv(f"{b}.conv1", bn=f"{b}.norm1" if batch_norm else None),
                        "conv2": conv(f"{b}.conv2", bn=f"{b}.norm2" if batch_norm else None),
                        "down": conv(f"{b}.downsample.0", bn=f"{b}.downsample.1" if batch_norm else None) if strided else None})
            return e

        with _host.on_device(dev):
            self.fnet = encoder("fnet", False)
            self.fnet["conv2"] = conv("fnet.conv2")
            self.cnet = encoder("cnet", True)
            self.cnet["net"] = conv("cnet.conv2", slice(0, HIDDEN))
            self.cnet["inp"] = conv("cnet.conv2", slice(HIDDEN, HIDDEN + CONTEXT))
            u = "update_block"
            self.convc1, self.convc2 = conv(f"{u}.encoder.convc1"), conv(f"{u}.encoder.convc2")
            self.convf1, self.convf2 = conv(f"{u}.encoder.convf1"), conv(f"{u}.encoder.convf2")
            self.conv = conv(f"{u}.encoder.conv")
            self.gru = []
            for half in ("1", "2"):
                zr = _Conv(lib, torch.cat([sd[f"{u}.gru.convz{half}.weight"], sd[f"{u}.gru.convr{half}.weight"]]),
                           torch.cat([sd[f"{u}.gru.convz{half}.bias"], sd[f"{u}.gru.convr{half}.bias"]]), dev)
                self.gru.append((zr, conv(f"{u}.gru.convq{half}")))
            self.fh1, self.fh2 = conv(f"{u}.flow_head.conv1"), conv(f"{u}.flow_head.conv2")
            self.mask0, self.mask2 = conv(f"{u}.mask.0"), conv(f"{u}.mask.2")

    @classmethod
    def from_state_dict(cls, sd, device=None) -> "RaftWeights":
        return cls(check_state_dict(sd), device)

    @classmethod
    def load(cls, path, device=None) -> "RaftWeights":
        sd = torch.load(os.fspath(path), map_location="cpu")
        if isinstance(sd, dict) and "state_dict" in sd and "fnet.conv1.weight" not in sd and "module.fnet.conv1.weight" not in sd:
            sd = sd["state_dict"]
        return cls.from_state_dict(sd, device)


# ------------------------------------------------------------------------------------------------ one shape's launches
def _slice(t: torch.Tensor, offset: int = 0, channels: Optional[int] = None) -> FlowSlice:
    """Channels [offset, offset + channels) of the NHWC buffer t (its last axis is the pixel's stride)."""
    stride = int(t.shape[-1])
    return FlowSlice(t.data_ptr(), stride, int(offset), stride - int(offset) if channels is None else int(channels))


class _Work:
    """The buffers of one (image size, factor, stream) and the launches over them, made once and replayed: every argument
    but the result's pointer is fixed."""

    def __init__(self, model: "RaftFlow", h: int, w: int, factor: int, stream: int):
        self.lib = _lib.load()
        self.dev = model.weights.device
        self.stream = ctypes.c_void_p(stream)
        self.keep: list = []                 # descriptors and buffers the launch lists point into
        wt = model.weights
        self.h, self.w, self.factor = h, w, factor
        self.hs, self.ws = h // factor, w // factor
        (self.pt, pb), (self.pl, pr) = pad_split(self.hs), pad_split(self.ws)
        Hp, Wp = self.hs + self.pt + pb, self.ws + self.pl + pr
        self.Hp, self.Wp = Hp, Wp
        self.h8, self.w8 = Hp // 8, Wp // 8
        P = self.P = self.h8 * self.w8
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.raw = torch.empty(2, h, w, 3, dtype=torch.uint8, device=self.dev)
        self.img = torch.empty(2, Hp, Wp, 3, **f32)
        self.fmap = torch.empty(2, P, FEATURES, **f32)
        self.packed = torch.empty(FEATURES * ((P + 63) // 64 * 64), **f32)
        self.level_hw = [(self.h8 >> l, self.w8 >> l) for l in range(LEVELS)]
        self.levels = [torch.empty(P, hl * wl, **f32) for hl, wl in self.level_hw]
        self.hx = torch.zeros(P, HIDDEN + CONTEXT + HIDDEN, **f32)       # [h | inp | out (126), flow (2)]
        self.rh = torch.empty(P, HIDDEN, **f32)
        self.zr = torch.empty(P, 2 * HIDDEN, **f32)
        self.q = torch.empty(P, HIDDEN, **f32)
        self.corr = torch.empty(P, CORR_CH, **f32)
        self.cor1 = torch.empty(P, 256, **f32)
        self.corflo = torch.empty(P, 256, **f32)                         # [cor (192) | flo (64)]
        self.flo1 = torch.empty(P, 128, **f32)
        self.fh = torch.empty(P, 256, **f32)
        self.mask = torch.empty(P, MASK_CH, **f32)
        self._pool: Dict[tuple, torch.Tensor] = {}
        self.flow_slice = _slice(self.hx, 2 * HIDDEN + CONTEXT - 2 + 0, 2)
        self.keep.append(self.flow_slice)

        # ---- the launch lists
        self.prep = []
        for i in range(2):
            self._add(self.prep, "gsr_flow_prep_image", h, w, self.raw[i].data_ptr(), factor, self.img[i].data_ptr())
        self.features = []
        x = self._encoder(self.features, wt.fnet, self.img, 2, False)
        self._conv(self.features, wt.fnet["conv2"], [_slice(x)], 2, x.shape[1], x.shape[2], _slice(self.fmap))
        self.direction = [self._direction(wt, d) for d in (0, 1)]
        self.iteration = self._iteration(wt)
        self.tail = []
        hs = _slice(self.hx, 0, HIDDEN)
        self._conv(self.tail, wt.mask0, [hs], 1, self.h8, self.w8, _slice(self.fh), act=ACT_RELU)
        self._conv(self.tail, wt.mask2, [_slice(self.fh)], 1, self.h8, self.w8, _slice(self.mask))

    # -- list building
    def _add(self, prog: list, name: str, *args) -> None:
        prog.append((getattr(self.lib, name), name, (*args, self.stream)))

    def _buf(self, role: str, *shape) -> torch.Tensor:
        key = (role, *shape)
        if key not in self._pool:
            self._pool[key] = torch.empty(*shape, dtype=torch.float32, device=self.dev)
        return self._pool[key]

    def _conv(self, prog, c: _Conv, inputs: List[FlowSlice], N, H, W, out: FlowSlice, stride=1, act=ACT_NONE, residual=None,
              residual_relu=False) -> None:
        if sum(s.channels for s in inputs) != c.Cin or out.channels != c.Cout:
            raise AssertionError("a convolution's slices do not match its weights")
        d = FlowConvDesc()
        d.N, d.H, d.W, d.KH, d.KW, d.stride, d.n_in, d.Cout, d.act = N, H, W, c.KH, c.KW, stride, len(inputs), c.Cout, act
        d.residual_relu = int(residual_relu)
        for i, s in enumerate(inputs):
            d.inputs[i] = s
        d.out = out
        if residual is not None:
            d.residual = residual
        d.weights, d.bias = c.w.data_ptr(), c.b.data_ptr()
        if c.scale is not None:
            d.scale, d.shift = c.scale.data_ptr(), c.shift.data_ptr()
        self.keep.append(d)
        self._add(prog, "gsr_flow_conv", ctypes.addressof(d))

    def _inorm(self, prog, x: torch.Tensor, relu: bool, residual: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None):
        N, H, W, C = x.shape
        ws = self._buf("inorm", int(self.lib.gsr_flow_instance_norm_workspace_bytes(N, H * W, C)) // 4 + 1)
        self._add(prog, "gsr_flow_instance_norm", N, H * W, C, x.data_ptr(), int(relu), None if residual is None else residual.data_ptr(),
                  (x if out is None else out).data_ptr(), ws.data_ptr())

    def _encoder(self, prog, e, img: torch.Tensor, N: int, batch_norm: bool) -> torch.Tensor:
        """extractor.py:168-184 up to layer3; returns its output buffer [N,H/8,W/8,128]."""
        H, W = self.Hp // 2, self.Wp // 2
        x = self._buf("x0", N, H, W, 64)
        self._conv(prog, e["conv1"], [_slice(img)], N, self.Hp, self.Wp, _slice(x), stride=2, act=ACT_RELU if batch_norm else ACT_NONE)
        if not batch_norm:
            self._inorm(prog, x, True)
        for k, b in enumerate(e["blocks"]):
            s, dim = b["stride"], b["conv1"].Cout
            Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
            y1, y2 = self._buf("y1", N, Ho, Wo, dim), self._buf("y2", N, Ho, Wo, dim)
            out = self._buf(f"x{1 + k % 2}", N, Ho, Wo, dim)
            xd = x
            if batch_norm:
                self._conv(prog, b["conv1"], [_slice(x)], N, H, W, _slice(y1), stride=s, act=ACT_RELU)
                if b["down"] is not None:
                    xd = self._buf("xd", N, Ho, Wo, dim)
                    self._conv(prog, b["down"], [_slice(x)], N, H, W, _slice(xd), stride=s)
                self._conv(prog, b["conv2"], [_slice(y1)], N, Ho, Wo, _slice(out), act=ACT_RELU, residual=_slice(xd), residual_relu=True)
            else:
                self._conv(prog, b["conv1"], [_slice(x)], N, H, W, _slice(y1), stride=s)
                self._inorm(prog, y1, True)
                self._conv(prog, b["conv2"], [_slice(y1)], N, Ho, Wo, _slice(y2))
                if b["down"] is not None:
                    xd = self._buf("xd", N, Ho, Wo, dim)
                    self._conv(prog, b["down"], [_slice(x)], N, H, W, _slice(xd), stride=s)
                    self._inorm(prog, xd, False)
                self._inorm(prog, y2, True, residual=xd, out=out)
            x, H, W = out, Ho, Wo
        return x

    def _direction(self, wt: RaftWeights, d: int) -> list:
        """Direction d (0: image 1 -> 2): the volume and its pyramid, then the context encoder into h and inp."""
        prog: list = []
        P = self.P
        self._add(prog, "gsr_flow_pack_features", P, FEATURES, self.fmap[1 - d].data_ptr(), self.packed.data_ptr())
        self._add(prog, "gsr_flow_corr_volume", P, P, FEATURES, self.fmap[d].data_ptr(), self.packed.data_ptr(), self.levels[0].data_ptr())
        for l in range(1, LEVELS):
            hl, wl = self.level_hw[l - 1]
            self._add(prog, "gsr_flow_corr_pool", P, hl, wl, self.levels[l - 1].data_ptr(), self.levels[l].data_ptr())
        x = self._encoder(prog, wt.cnet, self.img[d:d + 1], 1, True)
        self._conv(prog, wt.cnet["net"], [_slice(x)], 1, self.h8, self.w8, _slice(self.hx, 0, HIDDEN), act=ACT_TANH)
        self._conv(prog, wt.cnet["inp"], [_slice(x)], 1, self.h8, self.w8, _slice(self.hx, HIDDEN, CONTEXT), act=ACT_RELU)
        return prog

    def _iteration(self, wt: RaftWeights) -> list:
        """raft.py:122-131 with update.py:127-136, less the mask head."""
        prog: list = []
        h8, w8, P = self.h8, self.w8, self.P
        fl = self.flow_slice
        hs, xs = _slice(self.hx, 0, HIDDEN), _slice(self.hx, HIDDEN, CONTEXT + HIDDEN)
        self.keep += [hs, xs]
        self._add(prog, "gsr_flow_corr_lookup", h8, w8, h8, w8, ctypes.addressof(fl), *(t.data_ptr() for t in self.levels), self.corr.data_ptr())
        self._conv(prog, wt.convc1, [_slice(self.corr)], 1, h8, w8, _slice(self.cor1), act=ACT_RELU)
        self._conv(prog, wt.convc2, [_slice(self.cor1)], 1, h8, w8, _slice(self.corflo, 0, 192), act=ACT_RELU)
        self._conv(prog, wt.convf1, [fl], 1, h8, w8, _slice(self.flo1), act=ACT_RELU)
        self._conv(prog, wt.convf2, [_slice(self.flo1)], 1, h8, w8, _slice(self.corflo, 192, 64), act=ACT_RELU)
        self._conv(prog, wt.conv, [_slice(self.corflo)], 1, h8, w8, _slice(self.hx, HIDDEN + CONTEXT, HIDDEN - 2), act=ACT_RELU)
        zs, rs, rhs, qs = _slice(self.zr, 0, HIDDEN), _slice(self.zr, HIDDEN, HIDDEN), _slice(self.rh), _slice(self.q)
        self.keep += [zs, rs, rhs, qs]
        for zr, cq in wt.gru:
            self._conv(prog, zr, [_slice(self.hx)], 1, h8, w8, _slice(self.zr), act=ACT_SIGMOID)
            self._add(prog, "gsr_flow_gru_combine", P, 0, ctypes.addressof(rs), ctypes.addressof(hs), None, ctypes.addressof(rhs))
            self._conv(prog, cq, [rhs, xs], 1, h8, w8, qs, act=ACT_TANH)
            self._add(prog, "gsr_flow_gru_combine", P, 1, ctypes.addressof(zs), ctypes.addressof(hs), ctypes.addressof(qs), ctypes.addressof(hs))
        self._conv(prog, wt.fh1, [hs], 1, h8, w8, _slice(self.fh), act=ACT_RELU)
        self._conv(prog, wt.fh2, [_slice(self.fh)], 1, h8, w8, fl, residual=fl)
        return prog

    # -- replay
    def run(self, prog: list) -> None:
        for fn, name, args in prog:
            if fn(*args) != 0:
                _lib.check(1, name)

    def upsample(self) -> torch.Tensor:
        out = torch.empty(self.hs, self.ws, 2, dtype=torch.float32, device=self.dev)
        _lib.check(self.lib.gsr_flow_upsample(self.h8, self.w8, ctypes.addressof(self.flow_slice), self.mask.data_ptr(), self.pt, self.pl,
                                              self.hs, self.ws, out.data_ptr(), self.stream), "gsr_flow_upsample")
        return out


# ------------------------------------------------------------------------------------------------ the model
class RaftFlow:
    """The basic model's inference (raft.py:86-142 with test_mode=True) over RaftWeights.  Images are uint8 [H,W,3] (numpy, or
    torch tensors on the weights' device); the result is the unpadded flow_up as the reference saves it: f32 [H/factor,
    W/factor, 2] in (x, y) order, on the device.  Runs on the current stream without a host read; the buffers of an (image
    size, factor, stream) are allocated on first use and reused.  stages: also return the flow after these iteration counts
    (for tests).  ValueError before any launch: a wrong dtype, shape or device, a size `factor` does not divide, a padded side
    under 128, a correlation volume above max_volume_bytes."""

    def __init__(self, weights: RaftWeights, iters: int = 20, max_volume_bytes: int = 16 << 30):
        if not isinstance(weights, RaftWeights):
            raise ValueError("weights must be RaftWeights")
        if int(iters) < 1:
            raise ValueError("iters must be at least 1")
        self.weights, self.iters, self.max_volume_bytes = weights, int(iters), int(max_volume_bytes)
        self._work: Dict[tuple, _Work] = {}
        self._lock = threading.Lock()

    def volume_bytes(self, h: int, w: int, factor: int = 2) -> int:
        """Bytes of one direction's correlation pyramid for images of h x w."""
        h8, w8 = ((n // factor + sum(pad_split(n // factor))) // 8 for n in (h, w))
        return 4 * h8 * w8 * sum((h8 >> l) * (w8 >> l) for l in range(LEVELS))

    def _check(self, images, factor) -> Tuple[int, int, int]:
        if factor not in (1, 2, 4):
            raise ValueError(f"factor must be 1, 2 or 4, got {factor!r}")
        shape = None
        for k, im in enumerate(images, start=1):
            if isinstance(im, torch.Tensor):
                if im.device != self.weights.device:
                    raise ValueError(f"image{k} is on {im.device}, the weights are on {self.weights.device} (pass numpy for host data)")
            elif not isinstance(im, np.ndarray):
                raise ValueError(f"image{k} must be a numpy array or a torch tensor, got {type(im).__name__}")
            if str(im.dtype).replace("torch.", "") != "uint8":
                raise ValueError(f"image{k} must be uint8, got {im.dtype}")
            if im.ndim != 3 or im.shape[2] != 3:
                raise ValueError(f"image{k} must be [H,W,3], got {tuple(im.shape)}")
            if shape is not None and tuple(im.shape) != shape:
                raise ValueError(f"the images must have one shape, got {shape} and {tuple(im.shape)}")
            shape = tuple(im.shape)
        h, w = int(shape[0]), int(shape[1])
        if h % factor or w % factor or h < factor or w < factor:
            raise ValueError(f"the image size {h} x {w} is not divisible by factor {factor}")
        Hp, Wp = (n // factor + sum(pad_split(n // factor)) for n in (h, w))
        if Hp < MIN_SIDE or Wp < MIN_SIDE:
            raise ValueError(f"the padded size {Hp} x {Wp} is under {MIN_SIDE} on a side: the coarsest pyramid level would be one wide")
        need = self.volume_bytes(h, w, factor)
        if need > self.max_volume_bytes:
            raise ValueError(f"the correlation volume of {h} x {w} at factor {factor} takes {need} bytes, above max_volume_bytes = "
                             f"{self.max_volume_bytes}")
        return h, w, int(factor)

    def _get_work(self, h, w, factor) -> _Work:
        stream = _host.raw_stream(self.weights.device.index)
        key = (h, w, factor, stream)
        with self._lock:
            wk = self._work.get(key)
        if wk is None:
            wk = _Work(self, h, w, factor, stream)
            with self._lock:
                self._work[key] = wk
        return wk

    def _load(self, wk: _Work, images) -> None:
        for i, im in enumerate(images):
            wk.raw[i].copy_(im if isinstance(im, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(im)), non_blocking=False)
        wk.run(wk.prep)
        wk.run(wk.features)

    def _run_direction(self, wk: _Work, d: int, stages):
        wk.hx[:, -2:].zero_()
        wk.run(wk.direction[d])
        out = []
        for it in range(1, self.iters + 1):
            wk.run(wk.iteration)
            if it == self.iters or it in stages:
                wk.run(wk.tail)
                out.append(wk.upsample())
        return out if stages else out[-1]

    @torch.no_grad()
    def __call__(self, image1, image2, factor: int = 2, stages=()):
        h, w, factor = self._check((image1, image2), factor)
        with _host.on_device(self.weights.device):
            wk = self._get_work(h, w, factor)
            self._load(wk, (image1, image2))
            return self._run_direction(wk, 0, tuple(stages))

    @torch.no_grad()
    def pair(self, image1, image2, factor: int = 2):
        """(flow 1 -> 2, flow 2 -> 1): the feature encoder runs once on both images, the context encoder per direction; each
        result has the bits of the single-direction call."""
        h, w, factor = self._check((image1, image2), factor)
        with _host.on_device(self.weights.device):
            wk = self._get_work(h, w, factor)
            self._load(wk, (image1, image2))
            return self._run_direction(wk, 0, ()), self._run_direction(wk, 1, ())


# ------------------------------------------------------------------------------------------------ the warp's input
def flow_frames(images_cur, images_next, depth_cur, depth_next, model: RaftFlow, factor: int = 2) -> Callable[[int], tuple]:
    """The `frames(i)` callable of warp.warp_mesh and SurfaceGaussians.warp_mesh: camera i's (flow_f, flow_b, depth_cur,
    depth_next), the flows made here from the camera's two images and never leaving the device.  Each argument is indexable
    by camera or a callable i -> array."""
    if not isinstance(model, RaftFlow):
        raise ValueError("model must be a RaftFlow")

    def get(src, i):
        return src(i) if callable(src) else src[i]

    def frames(i: int):
        ff, fb = model.pair(get(images_cur, i), get(images_next, i), factor)
        return ff, fb, get(depth_cur, i), get(depth_next, i)

    return frames


def _load_image(path_base: str) -> np.ndarray:
    from . import formats
    if os.path.exists(path_base + ".png"):
        return np.ascontiguousarray(formats.load_png_rgb8(path_base + ".png")[..., :3])
    if os.path.exists(path_base + ".jpg"):
        from PIL import Image
        return np.ascontiguousarray(np.array(Image.open(path_base + ".jpg").convert("RGB"), np.uint8))
    raise FileNotFoundError(f"{path_base}.png (or .jpg) not found")


@torch.no_grad()
def write_flows(data_root, frame_0: int, frame_end: int, interval: int, weights: RaftWeights, factor: int = 2, views_in_flight: int = 2,
                rank: Optional[int] = None, world: Optional[int] = None, iters: int = 20) -> list:
    """demo_GauSTAR.py:58-107: for f in range(frame_0, frame_end - interval, interval) and every camera c of
    `rgb_cameras.npz` in this rank's shard (sweep.camera_shard), the flows between `{f:04d}/images/img_{c:04d}.png` (`.jpg`
    through PIL where only that exists) and frame f + interval's, written with np.savez_compressed under key `flow` to
    `{f:04d}/{warp.FLOW_DIRS[interval]}/{c:04d}_f.npz` and `_b.npz`.  No pad.txt is written (nothing is cropped, and
    warp_mesh_using_flow reads its absence as no padding) and no preview JPEG.  Returns the paths written."""
    from . import _rig, sweep, warp
    if interval not in warp.FLOW_DIRS:
        raise RuntimeError("Interval Error!")
    root = os.fspath(data_root)
    rig = _rig.Rig.load(os.path.join(root, "rgb_cameras.npz"))[0]
    model = RaftFlow(weights, iters)
    mine = sweep.camera_shard(rig.C, rank, world)
    written: list = []
    for f in range(int(frame_0), int(frame_end) - int(interval), int(interval)):
        out_dir = os.path.join(root, f"{f:04d}", warp.FLOW_DIRS[interval])
        os.makedirs(out_dir, exist_ok=True)
        results: List[Optional[tuple]] = [None] * len(mine)

        def per_camera(j, c, f=f, results=results):
            im1 = _load_image(os.path.join(root, f"{f:04d}", "images", f"img_{c:04d}"))
            im2 = _load_image(os.path.join(root, f"{f + interval:04d}", "images", f"img_{c:04d}"))
            ff, fb = model.pair(im1, im2, factor)
            results[j] = (ff.cpu().numpy(), fb.cpu().numpy())

        sweep.run_cameras(mine, per_camera, views_in_flight, weights.device)
        for j, c in enumerate(mine):
            for arr, tag in zip(results[j], ("f", "b")):
                path = os.path.join(out_dir, f"{c:04d}_{tag}.npz")
                np.savez_compressed(path, flow=arr)
                written.append(path)
    return written


def main(argv=None) -> int:
    """python -m gaustar_amd.flow DATA_ROOT --model raft-things.pth --frame_0 A --frame_end B [--interval N]: the flows of a
    sequence's frames (write_flows), with the reference's option names."""
    import argparse
    ap = argparse.ArgumentParser(prog="python -m gaustar_amd.flow", description=main.__doc__)
    ap.add_argument("data_root")
    ap.add_argument("--model", required=True, help="the basic model's checkpoint (raft-things.pth)")
    ap.add_argument("--frame_0", type=int, default=0)
    ap.add_argument("--frame_end", type=int, default=0)
    ap.add_argument("--interval", type=int, default=1)
    ap.add_argument("--factor", type=int, default=2)
    ap.add_argument("--device", default=None)
    a = ap.parse_args(argv)
    for p in write_flows(a.data_root, a.frame_0, a.frame_end, a.interval, RaftWeights.load(a.model, a.device), a.factor):
        print(p)
    return 0


__all__ = ["RaftWeights", "RaftFlow", "flow_frames", "write_flows", "expected_shapes", "check_state_dict", "pad_split"]

if __name__ == "__main__":
    raise SystemExit(main())
