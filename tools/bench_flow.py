"""RAFT optical flow (gsr_flow.hip) at config C's size: one camera's pair of flows between two 960 x 540 images (the
reference's half resolution of 1080p, so factor 1 here), 20 iterations: a 120 x 68 feature grid.

    python tools/bench_flow.py --out profiles/flow_config_c.txt

Timed between device events, medians (and the spread) of --reps repeats: model.pair, two single calls, and in the same run
tests/flow_ref.py's f32 model on the device through torch's own convolutions, once per direction (it shares nothing between
the directions; its feature encoder is timed alone so that a composition that shares it can be read off).  Then the parts of
a pair (image preparation and feature encoder, a direction's volume, pyramid and context encoder, one iteration, the mask
head and upsampling) and every launch of one iteration on its own, with the rate of each convolution.  The device's result
is compared with the f32 composition's (not a pin: both are f32 in different summation orders)."""
from __future__ import annotations

import argparse
import ctypes
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, ITERS = 540, 960, 20
F32_PEAK_TF = 157.0


def timed(fn, reps, inner=1):
    import torch
    fn()      # warm-up
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _i in range(inner):
            fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    return dict(ms=statistics.median(ms), lo=min(ms), hi=max(ms))


def describe(name, args):
    """(label, flop) of one launch of a _Work list."""
    from gaustar_amd._lib import FlowConvDesc
    if name != "gsr_flow_conv":
        return name[9:], 0.0
    d = ctypes.cast(args[0], ctypes.POINTER(FlowConvDesc)).contents
    cin = sum(d.inputs[i].channels for i in range(d.n_in))
    ho, wo = (d.H - 1) // d.stride + 1, (d.W - 1) // d.stride + 1
    return (f"conv {d.KH}x{d.KW} {cin:>3} -> {d.Cout:>3} on {d.N}x{d.H}x{d.W}" + (f" /{d.stride}" if d.stride > 1 else ""),
            2.0 * d.N * ho * wo * d.KH * d.KW * cin * d.Cout)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description=__doc__)
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--ref-reps", type=int, default=3)
    a = ap.parse_args(argv)
    import numpy as np
    import torch
    import flow_ref
    from gaustar_amd import flow
    assert torch.cuda.is_available(), "bench_flow needs a GPU"
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    base = torch.rand(1, 3, H // 16 + 3, W // 16 + 3, generator=g)
    big = torch.nn.functional.interpolate(base, size=(H + 8, W + 8), mode="bicubic", align_corners=True).clamp(0, 1)[0]
    u8 = (big * 255).round().to(torch.uint8).permute(1, 2, 0).numpy()
    im1, im2 = np.ascontiguousarray(u8[4:4 + H, 4:4 + W]), np.ascontiguousarray(u8[6:6 + H, 1:1 + W])
    d1, d2 = torch.from_numpy(im1).to(dev), torch.from_numpy(im2).to(dev)
    sd = flow_ref.seeded_state_dict(0.6)
    model = flow.RaftFlow(flow.RaftWeights.from_state_dict(sd, dev), iters=ITERS)
    lines = [f"RAFT basic model, {ITERS} iterations, {W} x {H} (factor 1): feature grid {(W + 7) // 8} x {(H + 7) // 8}; medians of {a.reps} "
             f"(low .. high), device events, ms"]

    def row(label, t, extra=""):
        lines.append(f"  {label:<58} {t['ms']:9.3f}  ({t['lo']:.3f} .. {t['hi']:.3f}){extra}")

    pair = timed(lambda: model.pair(d1, d2, factor=1), a.reps)
    row("model.pair (both directions, feature encoder shared)", pair)
    two = timed(lambda: (model(d1, d2, factor=1), model(d2, d1, factor=1)), a.reps)
    row("two single calls", two)

    sd32 = {k: v.to(dev) for k, v in sd.items()}
    ref = timed(lambda: (flow_ref.raft(sd32, im1, im2, ITERS, 1, torch.float32, device=dev), flow_ref.raft(sd32, im2, im1, ITERS, 1, torch.float32, device=dev)),
                a.ref_reps)
    row("flow_ref f32 on the device (torch), two directions", ref)
    x = torch.cat([flow_ref.prep_image(i, 1, torch.float32).to(dev).permute(2, 0, 1)[None] for i in (im1, im2)], 0)
    enc = timed(lambda: flow_ref.encoder(sd32, "fnet", x, False), a.ref_reps)
    row("  of which one feature-encoder pass (both images)", enc)
    row("  => the composition with the feature encoder shared", dict(ms=ref["ms"] - enc["ms"], lo=ref["lo"] - enc["hi"], hi=ref["hi"] - enc["lo"]))
    lines.append(f"  aim: pair no slower than that composition and under 40 ms -> "
                 f"{'met' if pair['ms'] <= ref['ms'] - enc['ms'] and pair['ms'] < 40 else 'MISSED'} ({pair['ms']:.1f} ms)")

    got = model(d1, d2, factor=1).cpu().numpy()
    want = flow_ref.raft(sd32, im1, im2, ITERS, 1, torch.float32, device=dev)[ITERS].cpu().numpy()
    lines.append(f"  max|device - f32 composition| = {np.abs(got - want).max():.3e} px at max|flow| = {np.abs(want).max():.2f} px")

    wk = next(iter(model._work.values()))
    lines.append("parts of a pair")
    parts = {"image preparation + feature encoder (once)": wk.prep + wk.features, "volume, pyramid, context encoder (per direction)": wk.direction[0],
             "one iteration (x 20 per direction)": wk.iteration, "mask head (per direction)": wk.tail}
    for label, prog in parts.items():
        t = timed(lambda prog=prog: wk.run(prog), a.reps)
        flop = sum(describe(n, ar)[1] for _f, n, ar in prog)
        row(label, t, f"  {flop / t['ms'] * 1e-9:7.1f} TF of the convolutions' {flop * 1e-9:.2f} GFLOP" if flop else "")
    up = timed(lambda: wk.upsample(), a.reps)
    row("upsampling (per direction)", up)
    for title, prog in (("every launch of one iteration", wk.iteration), ("every launch of a direction's set-up", wk.direction[0]),
                        ("every launch of the feature encoder", wk.features)):
        lines.append(title + f" (share of the list's sum; TF against the f32 matrix peak of {F32_PEAK_TF:.0f})")
        rows = []
        for fn, name, args in prog:
            t = timed(lambda fn=fn, args=args: fn(*args), a.reps, inner=5)
            rows.append((*describe(name, args), t))
        total = sum(r[2]["ms"] for r in rows)
        for label, flop, t in rows:
            row("  " + label, t, f"  {100 * t['ms'] / total:5.1f} %" + (f"  {flop / t['ms'] * 1e-9:6.1f} TF" if flop else ""))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(text)
    return 0


if __name__ == "__main__":
    raise SystemExit(main())
