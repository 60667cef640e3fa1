"""Plane-sweep stereo (gsr_stereo.hip) at config C's sizes: the level-6 icosphere's depth over scene.ring_cameras() at 1920 x 1080
as the prior, seeded noise as the images (the work of a plane does not depend on what the images show: every window passes
min_var and every plane of every band is scored).

    python tools/bench_stereo.py --out profiles/stereo_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  Timed
between device events, medians (and the spread) of --reps repeats, inputs on the device: luma of one image; sweep_view of three
cameras with S = 4 and R = 3, with the plane-range statistics of their tiles; the consistency pass of one camera; the merge of
two volumes at voxel 0.008.  sweep_rig over the 160 cameras and refine_hull as a whole are timed by the host clock around a run
that ends in a synchronise.  The yardstick, in the same run on the same GPU: an f32 torch composition of the same sweep
(grid_sample per plane and source, avg_pool2d window sums, topk), over the image's whole plane range."""
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

STEP_LIMIT_S = 540
H, W = 1080, 1920
HBM_BPS = 6.29e12          # a float4 copy, measured
CAMERAS = (0, 53, 159)
VOXEL, TRUNC = 0.008, 0.02


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


def torch_sweep(gl, prior, refc, rows, lumas, cfg):
    """The same sweep as an f32 torch composition: (best cost, its plane).  Not bit for bit -- the yardstick for time."""
    import torch
    import torch.nn.functional as F
    R = cfg.radius
    K, N = 2 * R + 1, (2 * R + 1) ** 2
    fx, fy, cx, cy = refc
    dev = gl.device
    g = gl.float()[None, None]
    pool = lambda x: F.avg_pool2d(x, K, 1, R) * N
    A, B = pool(g), pool(g * g)
    Vr = N * B - A * A
    thr = N * N * cfg.min_var
    covered = (prior > 0.01) & (prior < cfg.background)
    k_lo = torch.ceil((prior - cfg.near) / cfg.step).clamp_min(float(int(0.01 / cfg.step) + 1))      # k_min = floor(znear / step) + 1
    k_hi = torch.floor((prior + cfg.far) / cfg.step)
    rr, cc = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32), torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    ray = torch.stack([(cc - cx) / fx, (rr - cy) / fy, torch.ones_like(cc)], -1)
    best = torch.full((H, W), -2.0, device=dev)
    kb = torch.full((H, W), -1.0, device=dev)
    lo, hi = int(k_lo[covered].min()), int(k_hi[covered].max())
    for k in range(lo, hi + 1):
        L = ray * (k * cfg.step)
        scores = []
        for (Rs, ts, sfx, sfy, scx, scy), img in zip(rows, lumas):
            loc = L @ Rs.T + ts
            u, v = sfx * loc[..., 0] / loc[..., 2] + scx, sfy * loc[..., 1] / loc[..., 2] + scy
            grid = torch.stack([(u + 0.5) / img.shape[1] * 2 - 1, (v + 0.5) / img.shape[0] * 2 - 1], -1)[None]
            w = F.grid_sample(img.float()[None, None], grid, mode="bilinear", padding_mode="zeros", align_corners=False)
            Sw, Sww, Swg = pool(w), pool(w * w), pool(w * g)
            Vs = N * Sww - Sw * Sw
            sc = (N * Swg - Sw * A) / torch.sqrt(Vs * Vr)
            scores.append(torch.where((Vs >= thr) & (Vr >= thr) & (loc[..., 2] > 0.01)[None, None], sc, torch.full_like(sc, -2.0))[0, 0])
        cost = torch.topk(torch.stack(scores), cfg.keep, dim=0).values.mean(0)
        upd = covered & (k >= k_lo) & (k <= k_hi) & (cost > best)
        best, kb = torch.where(upd, cost, best), torch.where(upd, torch.full_like(kb, float(k)), kb)
    return best, kb, hi - lo + 1


def step(reps: int) -> dict:
    import numpy as np
    import torch
    from gaustar_amd import fusion, harness, hull, mesh_depth, scene, stereo, topology
    assert torch.cuda.is_available(), "bench_stereo needs a GPU"
    dev = torch.device("cuda:0")
    v, f = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    rig = topology.rig_from_cameras([harness.nerf_camera_from_scene(c) for c in scene.ring_cameras(W=W, H=H)])
    C = len(rig["shape"])
    priors, masks = [None] * C, [None] * C

    def sink(i, view):
        priors[i], masks[i] = view.depth, view.mask

    mesh_depth.render_mesh_depth(v, f, rig, sink, views_in_flight=1)
    gen = torch.Generator(device=dev).manual_seed(7)
    lumas = [torch.randint(0, 256, (H, W), dtype=torch.uint8, device=dev, generator=gen) for _ in range(C)]
    rgb = torch.randint(0, 256, (H, W, 3), dtype=torch.uint8, device=dev, generator=gen)
    torch.cuda.synchronize()
    focus = np.asarray(scene.SUBJECT_CENTER, np.float64)
    sources = stereo.select_sources(rig, 4, 1.0, 180.0, focus=focus)      # (every camera gets four, whatever the ring's spacing)
    cfg = stereo.StereoConfig()
    c4 = cfg.resolved(4)
    out = dict(C=C, F=len(f), sweep={}, torch={}, planes={})
    out["luma"] = dict(timed(lambda: stereo.luma(rgb), reps, 20), bytes=4 * H * W)

    for r in CAMERAS:
        out["sweep"][str(r)] = timed(lambda: stereo.sweep_view(rig, r, sources[r], lumas, priors[r], cfg), reps)
        d = priors[r].double()
        cov = (d > 0.01) & (d < cfg.background)
        k_lo = torch.clamp(torch.ceil((d - cfg.near) / cfg.step), min=float(int(0.01 / cfg.step) + 1))
        k_hi = torch.floor((d + cfg.far) / cfg.step)
        pad = lambda x, fill: torch.nn.functional.pad(x, (0, (-W) % 16, 0, (-H) % 16), value=fill)
        tiles = lambda x: x.reshape(x.shape[0] // 16, 16, x.shape[1] // 16, 16).permute(0, 2, 1, 3).reshape(-1, 256)
        lo = tiles(pad(torch.where(cov, k_lo, torch.full_like(d, 1e9)), 1e9)).min(1).values
        hi = tiles(pad(torch.where(cov, k_hi, torch.full_like(d, -1e9)), -1e9)).max(1).values
        live = hi >= lo
        n = (hi - lo + 1)[live]
        out["planes"][str(r)] = dict(covered=int(cov.sum()), tiles=int(live.numel()), live_tiles=int(live.sum()), mean=float(n.mean()),
                                     max=int(n.max()), band=int(((k_hi - k_lo + 1)[cov]).double().mean().round()),
                                     plane_pixels=float(((k_hi - k_lo + 1)[cov]).sum()))
    r = CAMERAS[0]
    rows = []
    for s in sources[r]:
        Rs, ts = stereo.relative_pose(rig, r, int(s))
        rows.append((torch.from_numpy(Rs).float().to(dev), torch.from_numpy(ts).float().to(dev), float(rig["intrinsics"][s][0, 0]),
                     float(rig["intrinsics"][s][1, 1]), W / 2, H / 2))
    refc = (float(rig["intrinsics"][r][0, 0]), float(rig["intrinsics"][r][1, 1]), W / 2, H / 2)
    srcs = [lumas[int(s)] for s in sources[r]]
    n_planes = torch_sweep(lumas[r], priors[r], refc, rows, srcs, c4)[2]
    out["torch"] = dict(timed(lambda: torch_sweep(lumas[r], priors[r], refc, rows, srcs, c4), reps), planes=n_planes)

    # ---- the rig, consistency, merge, the whole path
    def rig_run():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        views = stereo.sweep_rig(rig, lumas, priors, sources, cfg, views_in_flight=2, device=dev)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, views

    rig_run()
    runs = [rig_run() for _ in range(2)]
    views = runs[-1][1]
    out["rig"] = dict(s=statistics.median(t for t, _ in runs), lo=min(t for t, _ in runs), hi=max(t for t, _ in runs))
    one = [[int(s) for s in sources[i]] for i in range(C)]
    t = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        stereo.check_consistency(rig, views, np.array(one), cfg)
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    out["consistency_rig"] = dict(s=statistics.median(t[1:]), lo=min(t[1:]), hi=max(t[1:]))
    del views
    lo_box, hi_box = focus - scene.SUBJECT_RADIUS, focus + scene.SUBJECT_RADIUS
    a, b = fusion.TSDFVolume(lo_box, hi_box, VOXEL, TRUNC, dev), fusion.TSDFVolume(lo_box, hi_box, VOXEL, TRUNC, dev)
    a.weight.fill_(1.0), b.weight.fill_(3.0), a.tsdf.uniform_(-1, 1), b.tsdf.uniform_(-1, 1)
    n = a.tsdf.numel()
    out["merge"] = dict(timed(lambda: stereo.merge_volumes(a, b), reps), voxels=n, bytes=(4 + 3 + 5) * 4 * n)
    del a, b
    torch.cuda.empty_cache()
    runs = []
    for _ in range(2):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts, faces, info = stereo.refine_hull(rig, lumas, masks, voxel_size=VOXEL, sdf_trunc=TRUNC, taubin_iterations=0, target_faces=0,
                                                sources=sources, cfg=cfg, device=dev)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    out["refine_hull"] = dict(s=statistics.median(runs[1:]), lo=min(runs[1:]), hi=max(runs[1:]), faces=int(faces.shape[0]),
                              states=[int(x) for x in info["states"].sum(0)])
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU work and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(step(args.reps)))
        return
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--reps", str(args.reps)], capture_output=True, text=True,
                           timeout=STEP_LIMIT_S)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_stereo: the GPU step ran past {STEP_LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_stereo: the GPU step ended with status {r.returncode}\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    bound = lambda nbytes: f"{1e6 * nbytes / HBM_BPS:.1f} us at {HBM_BPS / 1e12:.2f} TB/s for {nbytes / 1e6:.1f} MB"
    lines = [f"# tools/bench_stereo.py: config C's mesh (icosphere level 6, {res['F']} faces) rendered to {res['C']} depth maps of {W} x {H} "
             f"by mesh_depth over scene.ring_cameras() as the priors, seeded noise as the images; S = 4, R = 3, step 0.004, band "
             f"[-0.008, +0.12]; GPU time between device events unless stated, medians of {args.reps}"]
    k = res["luma"]
    lines.append(f"luma, one image (20 back-to-back calls a repeat): {1e3 * k['ms']:.1f} us (min {1e3 * k['lo']:.1f}, max {1e3 * k['hi']:.1f}); "
                 f"traffic bound {bound(k['bytes'])}")
    for cam, k in res["sweep"].items():
        p = res["planes"][cam]
        lines.append(f"sweep_view, camera {cam}: {k['ms']:.2f} ms (min {k['lo']:.2f}, max {k['hi']:.2f}); {p['covered']} covered pixels, "
                     f"{p['live_tiles']} of {p['tiles']} tiles swept, planes per swept tile mean {p['mean']:.1f} max {p['max']} (a pixel's band: "
                     f"{p['band']}), {p['plane_pixels'] / 1e6:.1f} M (pixel, plane) pairs = {1e6 * k['ms'] / p['plane_pixels']:.2f} ns each")
    k = res["torch"]
    first = res["sweep"][str(CAMERAS[0])]["ms"]
    lines.append(f"the f32 torch composition of camera {CAMERAS[0]}'s sweep (grid_sample, avg_pool2d, topk over the image's {k['planes']} planes): "
                 f"{k['ms']:.1f} ms (min {k['lo']:.1f}, max {k['hi']:.1f}) = {k['ms'] / first:.1f} x the HIP sweep's {first:.2f} ms")
    k = res["rig"]
    lines.append(f"sweep_rig, {res['C']} cameras, two views in flight, lumas and priors on the device, host clock to the final synchronise "
                 f"(two runs after a warm-up): {k['s']:.2f} s (min {k['lo']:.2f}, max {k['hi']:.2f}) = {1e3 * k['s'] / res['C']:.1f} ms per camera")
    k = res["consistency_rig"]
    lines.append(f"check_consistency, {res['C']} cameras, host clock (median of 3): {1e3 * k['s']:.1f} ms (min {1e3 * k['lo']:.1f}, max "
                 f"{1e3 * k['hi']:.1f}) = {1e3 * k['s'] / res['C']:.2f} ms per camera, table upload included")
    k = res["merge"]
    lines.append(f"merge_volumes, voxel {VOXEL} ({k['voxels'] / 1e6:.1f} M voxels; the output volume's allocation included): {k['ms']:.3f} ms "
                 f"(min {k['lo']:.3f}, max {k['hi']:.3f}); traffic bound {bound(k['bytes'])}")
    k = res["refine_hull"]
    lines.append(f"refine_hull, voxel {VOXEL}, bounds from the rig alone, no smoothing or decimation, host clock (the second of two runs): {k['s']:.2f} s "
                 f"(min {k['lo']:.2f}, max {k['hi']:.2f}); {k['faces']} faces; pixels by state over the rig {k['states']} (noise: nothing is accepted)")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
