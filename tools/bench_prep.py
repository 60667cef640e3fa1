"""The data-preparation kernels (gsr_prep.hip) at the sizes of a capture: rectify_image at 1920 x 1080 x 3 and at ActorsHQ's full
4112 x 3008 x 3, color_mesh_from_views for config C's rig (the 160 cameras of scene.ring_cameras() at 1920 x 1080, the level-6
icosphere's 40 962 vertices) and finish_colors at 8 sweeps.

    python tools/bench_prep.py --out profiles/prep_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.
rectify_image is timed through the C entry point on buffers made beforehand, with device events around --inner back-to-back
calls and no host read between them (medians and the spread of --reps repeats), beside two yardsticks measured in the same run
the same way: a plain torch copy of the image (the 2 H W C bytes the kernel has to move, at the bandwidth a copy of that size
reaches) and torch.nn.functional.grid_sample doing the same warp on an f32 image with a grid made beforehand.  The colours are
timed with the host clock around a call that ends in a synchronise (the Python front end included), inputs on the device, with
the depth maps handed in and with them rendered; finish_colors between device events.  The 1080p distorted image is checked
against the numpy restatement tests/prep_ref.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_LIMIT_S = 420
SIZES = {"1080p": (1080, 1920, 3), "ActorsHQ full": (3008, 4112, 3)}
DIST = (-0.05, 0.01, 1e-4, -2e-4, 0.001)
SHIFT = (3.25, -2.5)


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
    return statistics.median(ms), min(ms), max(ms)


def host_timed(fn, reps):
    import torch
    runs = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        runs.append(1e3 * (time.perf_counter() - t0))
    runs = runs[1:]      # (the first is the warm-up)
    return statistics.median(runs), min(runs), max(runs)


def _source_grid(H, W, fx, cx, cy, dist, dev):
    """The warp of rectify_image as grid_sample's normalised grid [1,H,W,2] in f32 (align_corners=True)."""
    import torch
    r, c = torch.meshgrid(torch.arange(H, dtype=torch.float64, device=dev), torch.arange(W, dtype=torch.float64, device=dev), indexing="ij")
    if dist is None:
        su, sv = c + (cx - 0.5 * W), r + (cy - 0.5 * H)
    else:
        k1, k2, p1, p2, k3 = dist
        x, y = (c - 0.5 * W) / fx, (r - 0.5 * H) / fx
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        su = fx * (x * rad + (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) + cx
        sv = fx * (y * rad + (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) + cy
    return torch.stack([2.0 * su / (W - 1) - 1.0, 2.0 * sv / (H - 1) - 1.0], -1)[None].float().contiguous()


def step(reps: int, inner: int) -> dict:
    import ctypes
    import numpy as np
    import torch
    import prep_ref as ref
    from gaustar_amd import _host, _lib, dataprep, harness, scene, topology
    from gaustar_amd.meshes import MeshTopology
    assert torch.cuda.is_available(), "bench_prep needs a GPU"
    dev = torch.device("cuda:0")
    lib, p, st = _lib.load(), _lib.ptr, _host.raw_stream(dev.index)
    out = dict(rectify={}, colors={}, finish={})
    border = (ctypes.c_ubyte * 3)(0, 0, 0)
    for name, (H, W, C) in SIZES.items():
        fx = 0.9 * W
        cx, cy = W / 2 + SHIFT[0], H / 2 + SHIFT[1]
        src = torch.randint(0, 256, (H, W, C), dtype=torch.uint8, device=dev)
        dst = torch.empty_like(src)
        cam4 = (ctypes.c_double * 4)(fx, fx, cx, cy)
        row = dict(bytes=2 * H * W * C)
        for path, dist in (("plain", None), ("distorted", DIST)):
            d5 = None if dist is None else (ctypes.c_double * 5)(*dist)

            def call():
                rc = lib.gsr_image_rectify(H, W, C, p(src), p(dst), cam4, d5, border, st)
                assert rc == 0, lib.gsr_last_error()
            row[path] = timed(call, reps, inner)
            img = src.permute(2, 0, 1)[None].float().contiguous()
            grid = _source_grid(H, W, fx, cx, cy, dist, dev)
            row["grid_sample " + path] = timed(lambda: torch.nn.functional.grid_sample(img, grid, mode="bilinear", padding_mode="zeros",
                                                                                        align_corners=True), reps, inner)
            del img, grid
        row["copy"] = timed(lambda: dst.copy_(src), reps, inner)
        if name == "1080p":
            rc = lib.gsr_image_rectify(H, W, C, p(src), p(dst), cam4, (ctypes.c_double * 5)(*DIST), border, st)
            assert rc == 0
            out["same"] = bool(np.array_equal(dst.cpu().numpy(), ref.rectify(src.cpu().numpy(), (fx, fx, cx, cy), DIST, 0)))
        out["rectify"][name] = row
        del src, dst

    H, W = 1080, 1920
    v, f = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    rig = topology.rig_from_cameras([harness.nerf_camera_from_scene(c) for c in scene.ring_cameras(W=W, H=H)])
    C = len(rig["shape"])
    tv = torch.from_numpy(np.asarray(v, np.float64)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev)
    images = torch.randint(0, 256, (C, H, W, 3), dtype=torch.uint8, device=dev)
    depths = torch.empty(C, H, W, dtype=torch.float32, device=dev)
    from gaustar_amd import mesh_depth
    mesh_depth.render_mesh_depth(tv, tf, rig, lambda i, view: depths[i].copy_(view.depth), views_in_flight=1)
    out["C"], out["V"] = C, len(v)
    few = max(3, reps // 2)
    for vif in (1, 2):
        out["colors"][f"depths given, views_in_flight = {vif}"] = host_timed(
            lambda: dataprep.color_mesh_from_views(tv, tf, rig, images, depths, views_in_flight=vif, rank=0, world=1), few)
        out["colors"][f"depths rendered, views_in_flight = {vif}"] = host_timed(
            lambda: dataprep.color_mesh_from_views(tv, tf, rig, images, None, views_in_flight=vif, rank=0, world=1), few)
    sums = dataprep.view_color_sums(tv, rig, images, depths, views_in_flight=1, rank=0, world=1)
    cols = dataprep.finish_colors(sums, tf, 8)
    out["seen"] = [int((sums[:, 3] > 0).sum()), cols.n_unseen, cols.n_unfilled]
    V = len(v)
    off, nbr = MeshTopology.of(tf, V).vertex_neighbours
    mean = torch.empty(V, 3, dtype=torch.float64, device=dev)
    rgb = torch.empty(V, 3, dtype=torch.uint8, device=dev)
    at = torch.empty(V, dtype=torch.uint8, device=dev)
    cnt = torch.zeros(2, dtype=torch.int32, device=dev)
    ws = torch.empty(3 * V, dtype=torch.int32, device=dev)
    dc = (ctypes.c_ubyte * 3)(128, 128, 128)
    for sweeps in (0, 8):
        def call():
            rc = lib.gsr_mesh_color_finish(V, p(sums), p(off), p(nbr), sweeps, dc, p(ws), p(mean), p(rgb), p(at), p(cnt), st)
            assert rc == 0, lib.gsr_last_error()
        out["finish"][str(sweeps)] = timed(call, reps, inner)
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU work and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(step(args.reps, args.inner)))
        return
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--reps", str(args.reps), "--inner", str(args.inner)],
                           capture_output=True, text=True, timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_prep: the GPU step ran past {STEP_LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_prep: the GPU step ended with status {r.returncode}\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    lines = [f"# tools/bench_prep.py: GPU time between device events, median of {args.reps} x {args.inner} back-to-back calls (min, max), no host "
             f"read; shift {SHIFT}, distortion {DIST}, focal 0.9 W"]
    for name, row in res["rectify"].items():
        H, W, C = SIZES[name]
        nbytes = row["bytes"]
        copy = row["copy"]
        lines.append(f"{name} ({W} x {H} x {C}), torch copy of the image: {1e3 * copy[0]:.1f} us (min {1e3 * copy[1]:.1f}, max {1e3 * copy[2]:.1f}); "
                     f"{nbytes / 1e6:.1f} MB read + written, {nbytes / copy[0] / 1e9:.2f} TB/s")
        for path in ("plain", "distorted"):
            k, g = row[path], row["grid_sample " + path]
            lines.append(f"{name}, gsr_image_rectify, {path} path: {1e3 * k[0]:.1f} us (min {1e3 * k[1]:.1f}, max {1e3 * k[2]:.1f}); "
                         f"{nbytes / k[0] / 1e9:.2f} TB/s of the bytes it must move = {100 * copy[0] / k[0]:.0f} % of the copy's bandwidth; "
                         f"grid_sample (f32 image, grid made beforehand): {1e3 * g[0]:.1f} us (min {1e3 * g[1]:.1f}, max {1e3 * g[2]:.1f})")
    lines.append(f"# colours: config C's rig, {res['C']} cameras at 1920 x 1080, {res['V']} vertices, images (and depth maps) on the device; "
                 f"host clock to the final synchronise, Python front end included")
    for name, k in res["colors"].items():
        lines.append(f"color_mesh_from_views, {name}: {k[0]:.2f} ms (min {k[1]:.2f}, max {k[2]:.2f}) = {1e3 * k[0] / res['C']:.1f} us per camera")
    lines.append(f"vertices seen by a camera: {res['seen'][0]} of {res['V']}; unseen {res['seen'][1]}, left after 8 sweeps {res['seen'][2]}")
    for sweeps, k in res["finish"].items():
        lines.append(f"gsr_mesh_color_finish, fill_sweeps = {sweeps}: {1e3 * k[0]:.1f} us (min {1e3 * k[1]:.1f}, max {1e3 * k[2]:.1f})")
    lines.append(f"1080p distorted image equal to the restatement byte for byte: {res['same']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert res["same"], "the kernel and the restatement disagree"


if __name__ == "__main__":
    main()
