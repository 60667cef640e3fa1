"""Scene-flow mesh warping at config C (160 cameras at 1080p, level-6 icosphere): gaustar_amd.warp.

    python tools/bench_warp.py --out profiles/warp_config_c.txt        # wall time, launches, counts, restatement
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o warp -- python tools/bench_warp.py --warp-only
    python tools/bench_warp.py --kernel-stats DIR --out profiles/warp_config_c.txt     # appends the GPU-time split

The inputs are the analytic scene of the tests (tests/warp_scene.py: the sphere turns 4 degrees and moves by 2-3 cm),
generated on the device before the timing.  The wall time is one warp (the host waits only in the view pipelines and at the
end), median of --reps after a warm-up.  The restatement timed here is the tests' numpy restatement (tests/warp_ref.py) on this host's CPUs
-- NOT the reference, which needs libraries this project does not have."""
from __future__ import annotations

import argparse
import csv
import glob
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _setup():
    import torch
    import test_gpu_warp as t
    from gaustar_amd import scene
    rig = t._rig(scene.ring_cameras())
    v, f = t._mesh(6)
    fr = t._frames(rig)
    torch.cuda.synchronize()
    return rig, v, f, t._faces_t(f), fr


def run(args) -> None:
    import numpy as np
    import torch
    import warp_ref as wr
    import warp_scene as ws
    from gaustar_amd import scene, warp
    rig, v, f, ft, fr = _setup()
    res = warp.warp_mesh(v, ft, rig, lambda i: fr[i], return_stages=True)     # warm-up
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = warp.warp_mesh(v, ft, rig, lambda i: fr[i])
        times.append(time.perf_counter() - t0)
    assert torch.equal(r.move_propagated, res.move_propagated)
    C, V, F = len(rig["shape"]), len(v), len(f)
    H, W = (int(x) for x in rig["shape"][0])
    cnt = res.count.cpu().numpy()
    want = ws.moved(v, scene.SUBJECT_CENTER)
    r1k = warp.warp_mesh(v, ft, rig, lambda i: fr[i], warp.WarpConfig(edge_scalar=1000))      # (untimed: the accuracy line)
    good = r1k.count.cpu().numpy() >= 4
    e_raw = np.linalg.norm(r1k.verts_raw.cpu().numpy() - want, axis=1)
    e_sm = np.linalg.norm(r1k.verts_smoothed.cpu().numpy() - want, axis=1)
    lines = [f"# tools/bench_warp.py at config C: {C} cameras {W}x{H}, V={V} F={F}, analytic scene (4 deg turn + (2, -1, 3) cm)",
             f"warp wall time (inputs on the device, host waits only in the view pipelines and at the end), median of {args.reps}: "
             f"{1e3 * statistics.median(times):.1f} ms (min {1e3 * min(times):.1f}, max {1e3 * max(times):.1f})",
             "launches per camera: 3 (warp_depth_max, warp_var_max, warp_view)",
             "rig-wide launches: 2 normals (face, vertex) + 1 aggregate + 3 x 20 propagation sweeps + 5 smoothing sweeps, plus torch "
             "plumbing (transposes, adds)",
             f"table: {C} x {V} x 3 f64 = {C * V * 24 / 1e6:.0f} MB",
             f"default config (edge_scalar 10000): max observed {int(res.observed.max())} cameras, vertices with count >= 4: "
             f"{(cnt >= 4).mean():.4f}",
             f"edge_scalar 1000: count >= 4 {good.mean():.4f}; error vs the known motion: raw median {1e3 * np.median(e_raw[good]):.3f} mm, "
             f"p99 {1e3 * np.percentile(e_raw[good], 99):.3f} mm (count >= 4); smoothed median {1e3 * np.median(e_sm):.3f} mm, "
             f"max {1e3 * e_sm.max():.3f} mm (all vertices)"]
    normals = wr.vertex_normals(v, f)
    sample = list(range(0, C, C // args.restated_cams))[:args.restated_cams]
    maps = [[x.cpu().numpy() for x in fr[i]] for i in sample]
    t0 = time.perf_counter()
    for i, (a, b, c, d) in zip(sample, maps):
        wr.camera_row(v, normals, a, b, None, c, d, rig["intrinsics"][i], rig["extrinsics"][i], rig["shape"][i])
    per_cam = (time.perf_counter() - t0) / len(sample)
    table = res.table.cpu().numpy()
    t0 = time.perf_counter()
    move, _, count = wr.aggregate(table)
    t_agg = time.perf_counter() - t0
    nb = wr.neighbours(f, V)
    t0 = time.perf_counter()
    prop = np.stack([wr.propagate_sequential(nb, count >= 4, move[:, k], 20) for k in range(3)], -1)
    t_prop = time.perf_counter() - t0
    t0 = time.perf_counter()
    wr.smooth(nb, prop, 5)
    t_sm = time.perf_counter() - t0
    lines += [f"numpy RESTATEMENT (tests/warp_ref.py, not the reference) on this host ({os.cpu_count()} CPUs visible, "
              f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}):",
              f"  per-camera rows: {1e3 * per_cam:.0f} ms per camera (mean of {len(sample)}), x {C} = {per_cam * C:.1f} s",
              f"  aggregate: {t_agg:.2f} s, propagation (sequential, 20 sweeps max, per component): {t_prop:.2f} s, "
              f"smoothing (5 sweeps): {t_sm:.2f} s"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


def warp_only(args) -> None:
    import torch
    from gaustar_amd import warp
    rig, v, f, ft, fr = _setup()
    for _ in range(1 + args.reps):
        warp.warp_mesh(v, ft, rig, lambda i: fr[i])
    torch.cuda.synchronize()
    print(f"warps: {1 + args.reps}")


def kernel_stats(args) -> None:
    """Split the kernel GPU time of a --warp-only run into the warp kernels, the propagation kernel and the rest (torch)."""
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {args.kernel_stats}")
    groups = {"warp": [0.0, 0], "other": [0.0, 0]}
    rows = []
    with open(files[0]) as fh:
        for r in csv.DictReader(fh):
            n = r["Name"].replace("(anonymous namespace)::", "")
            ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
            g = "warp" if ("warp_" in n or "topo_propagate" in n) else "other"
            groups[g][0] += ns
            groups[g][1] += calls
            if g == "warp":
                rows.append((n.split("(")[0].replace("gsr::", ""), calls, ns / calls / 1e3, ns / 1e6))
    reps = 1 + args.reps
    warp_ms = groups["warp"][0] / 1e6 / reps
    other_ms = groups["other"][0] / 1e6 / reps
    lines = ["", f"# rocprofv3 --kernel-trace --stats of tools/bench_warp.py --warp-only ({reps} warps), per warp:",
             f"warp_* kernels + topo_propagate_kernel: {warp_ms:.3f} ms (estimate in the issue: <= 8 ms)",
             f"other kernels (torch: the set-up's scene generation included, transposes, adds): {other_ms:.3f} ms (all runs / {reps})",
             "kernel, calls (all runs), mean us, total ms (all runs):"]
    lines += [f"  {n:<28} {c:>6} {a:>9.2f} {t:>9.3f}" for n, c, a, t in sorted(rows, key=lambda x: -x[3])]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--restated-cams", type=int, default=2)
    ap.add_argument("--warp-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_stats(args)
    elif args.warp_only:
        warp_only(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
