"""Generates tests/golden/flow/flow_kat.npz by IMPORTING the reference's own RAFT (data_process/RAFT/core; runs only in the build
container, where /root/reference exists; torch CPU, f32).  Inputs + expected outputs only; run by hand, not a test.

Per case: two smooth u8 images of 125 x 134 (the second the first shifted by (3, -2)), which InputPadder pads to 128 x 136: a
16 x 17 feature grid with pyramid levels 16 x 17, 8 x 8, 4 x 4 and 2 x 2.  The model runs with tests/flow_ref.py's
seeded_state_dict(gain); per stage k in {1, 4, 20} iterations the file holds the unpadded flow_up as demo_GauSTAR.py saves it
and the sensitivity s_k: the largest change of the reference's own output over DRAWS draws of every weight scaled by
1 + 2^-23 xi, xi uniform in [-1, 1].
  case A, gain 0.6: the flows stay inside the lookup windows;   asserted: s_20 <= 1e-4 px, 2 <= max|flow_20| <= 32 px
  case B, gain 1.0: the flows leave every level (zero padding);   asserted: s_20 <= 1e-3 px, max|flow_20| >= 64 px"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, os.path.join(HERE, "..", ".."))
sys.path.insert(0, "/root/reference/data_process/RAFT/core")
from raft import RAFT                      # noqa: E402
from utils.utils import InputPadder        # noqa: E402
import flow_ref                            # noqa: E402

STAGES = (1, 4, 20)
DRAWS = 3
H, W = 125, 134
SHIFT = (3, -2)                            # (x, y) of the second image's content


def smooth_pair(seed):
    g = torch.Generator().manual_seed(seed)
    m = 8
    base = torch.rand(1, 3, (H + 2 * m) // 6 + 2, (W + 2 * m) // 6 + 2, generator=g)
    big = torch.nn.functional.interpolate(base, size=(H + 2 * m, W + 2 * m), mode="bicubic", align_corners=True).clamp(0, 1)[0]
    u8 = (big * 255.0).round().to(torch.uint8).permute(1, 2, 0).numpy()
    a = u8[m:m + H, m:m + W]
    b = u8[m - SHIFT[1]:m - SHIFT[1] + H, m - SHIFT[0]:m - SHIFT[0] + W]
    return np.ascontiguousarray(a), np.ascontiguousarray(b)


def model_of(sd):
    m = RAFT(argparse.Namespace(small=False, mixed_precision=False, alternate_corr=False))
    res = m.load_state_dict(sd, strict=False)
    assert not res.unexpected_keys and all(k.endswith("num_batches_tracked") for k in res.missing_keys), res
    return m.eval()


def run(sd, a, b):
    m = model_of(sd)
    t = [torch.from_numpy(x).permute(2, 0, 1).float()[None] for x in (a, b)]
    padder = InputPadder(t[0].shape)
    i1, i2 = padder.pad(*t)
    out = {}
    with torch.no_grad():
        for k in STAGES:
            _, up = m(i1, i2, iters=k, test_mode=True)
            out[k] = padder.unpad(up[0]).permute(1, 2, 0).contiguous().numpy()
    return out


out = {"stages": np.array(STAGES)}
for case, gain, seed in (("A", 0.6, 11), ("B", 1.0, 23)):
    a, b = smooth_pair(seed)
    sd = flow_ref.seeded_state_dict(gain)
    base = run(sd, a, b)
    s = {k: 0.0 for k in STAGES}
    for d in range(DRAWS):
        g = torch.Generator().manual_seed(1000 + d)
        pert = {k: v * (1.0 + 2.0 ** -23 * (2.0 * torch.rand(v.shape, generator=g, dtype=torch.float64) - 1.0)).to(torch.float32)
                for k, v in sd.items()}
        res = run(pert, a, b)
        for k in STAGES:
            s[k] = max(s[k], float(np.abs(res[k].astype(np.float64) - base[k]).max()))
    mx = float(np.abs(base[20]).max())
    print(f"case {case}: gain {gain}  s = {[s[k] for k in STAGES]}  max|flow| = {[float(np.abs(base[k]).max()) for k in STAGES]}")
    if case == "A":
        assert s[20] <= 1e-4 and 2.0 <= mx <= 32.0, (s, mx)
    else:
        assert s[20] <= 1e-3 and mx >= 64.0, (s, mx)
    out[f"{case}_gain"] = np.float64(gain)
    out[f"{case}_image1"], out[f"{case}_image2"] = a, b
    for k in STAGES:
        out[f"{case}_flow_{k}"] = base[k]
        out[f"{case}_s_{k}"] = np.float64(s[k])

# (in a directory of its own: conftest.golden_names() takes every .npz directly under tests/golden/ for a rasterizer case)
os.makedirs(os.path.join(HERE, "flow"), exist_ok=True)
path = os.path.join(HERE, "flow", "flow_kat.npz")
np.savez_compressed(path, **out)
print(path, os.path.getsize(path), "bytes")
assert os.path.getsize(path) < 1_000_000
