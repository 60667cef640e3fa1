"""Rig-wide topology-error detection at config C (160 cameras at 1080p, level-6 icosphere): gaustar_amd.topology.

    python tools/bench_topology.py --out profiles/topology_config_c.txt        # wall time, voxels, launches, restatement
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o topo -- python tools/bench_topology.py --detect-only
    python tools/bench_topology.py --kernel-stats DIR --out profiles/topology_config_c.txt     # appends the GPU-time split

The GT depth is the depth render of the same model with a cap pushed 5 cm inward (tests/test_gpu_topology.py), so the
detection has work to do.  The wall time is one detection (one host synchronisation, at its end), median of --reps after a
warm-up.  The restatement timed here is the tests' numpy restatement (tests/topo_ref.py) on this host's CPUs -- NOT the
reference, which needs libraries this project does not have; its kNN step is not timed (a brute-force numpy argsort)."""
from __future__ import annotations

import argparse
import csv
import glob
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def _setup():
    import torch
    import test_gpu_topology as t
    model, cams = t._model(6), t._ring_cams()
    gt = t._gt_depth(model, cams, True)
    torch.cuda.synchronize()
    return model, cams, gt


def run(args) -> None:
    import torch
    import topo_ref as tr
    from gaustar_amd import topology
    model, cams, gt = _setup()
    res = topology.detect_topology_errors(model, cams, gt, return_stages=True)    # warm-up
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = topology.detect_topology_errors(model, cams, gt)
        times.append(time.perf_counter() - t0)
    assert torch.equal(r.face_loss, res.face_loss)
    V, F, C = model._points.shape[0], res.face_loss.shape[0], len(cams)
    lines = [f"# tools/bench_topology.py at config C: {C} cameras {cams[0].width}x{cams[0].height}, V={V} F={F} "
             f"N={model.n_points}, planted 5 cm cap",
             f"detection wall time (one host sync at the end), median of {args.reps}: {1e3 * statistics.median(times):.1f} ms "
             f"(min {1e3 * min(times):.1f}, max {1e3 * max(times):.1f})",
             f"launches per camera: 2 renders + 3 (topo_gt_max, topo_var_max, topo_view)",
             f"rig-wide launches: 1 aggregate + 20 propagation sweeps + 1 voxel key + 1 voxel reduce + 3 kNN (bound, part, merge) + 1 face, plus torch "
             f"plumbing (min, amin, stable sort, key changes, cumsum, unbind weights, count)",
             f"voxels: {res.n_voxels}",
             f"topo_change_num: {res.topo_change_num} (decision {res.decision}), faces at 1: {int((res.face_loss == 1).sum())}"]
    # the numpy restatement (tests/topo_ref.py) on this host: per-camera rows on a few cameras, then steps 8-10 on the table
    rig = topology.rig_from_cameras(cams)
    rend = topology.DepthRenders(model)
    verts = model._points.detach().cpu().numpy()
    faces = model._surface_mesh_faces.cpu().numpy()
    sample = list(range(0, C, C // args.restated_cams))[:args.restated_cams]
    maps = [(gt[i].cpu().numpy(), *(x.cpu().numpy() for x in rend(cams[i]))) for i in sample]
    t0 = time.perf_counter()
    for i, (g, a, b) in zip(sample, maps):
        tr.camera_row(verts, g, a, b, rig["intrinsics"][i], rig["extrinsics"][i], rig["shape"][i])
    per_cam = (time.perf_counter() - t0) / len(sample)
    table = res.table.cpu().numpy()
    t0 = time.perf_counter()
    value, cnt = tr.aggregate(table, verts)
    t_agg = time.perf_counter() - t0
    t0 = time.perf_counter()
    tr.propagate_sequential(tr.neighbours(faces, V), cnt >= 4, value, 20)
    t_prop = time.perf_counter() - t0
    lines += [f"numpy RESTATEMENT (tests/topo_ref.py, not the reference) on this host ({os.cpu_count()} CPUs visible, "
              f"OMP_NUM_THREADS={os.environ.get('OMP_NUM_THREADS', 'unset')}):",
              f"  per-camera rows: {1e3 * per_cam:.0f} ms per camera (mean of {len(sample)}), x {C} = {per_cam * C:.1f} s",
              f"  aggregate: {t_agg:.2f} s, propagation (sequential, 20 sweeps max): {t_prop:.2f} s; voxel kNN: not timed"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


def detect_only(args) -> None:
    import torch
    from gaustar_amd import topology
    model, cams, gt = _setup()
    for _ in range(1 + args.reps):
        topology.detect_topology_errors(model, cams, gt)
    torch.cuda.synchronize()
    print(f"renders: {len(cams)} GT + {2 * len(cams) * (1 + args.reps)} detection")


def kernel_stats(args) -> None:
    """Split the kernel GPU time of a --detect-only run into the new kernels, the rasterizer's and the rest (torch)."""
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {args.kernel_stats}")
    names = set()
    for f in glob.glob(os.path.join(ROOT, "gaustar_amd", "csrc", "*.hip")):
        if not f.endswith("gsr_topo.hip"):
            names |= set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)", open(f).read()))
    groups = {"topo": [0.0, 0], "rasterizer": [0.0, 0], "other": [0.0, 0]}
    rows = []
    with open(files[0]) as fh:
        for r in csv.DictReader(fh):
            n = r["Name"].replace("(anonymous namespace)::", "")
            ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
            g = "topo" if n.startswith("topo_") or "::topo_" in n else (
                "rasterizer" if any(k in n for k in names) else "other")
            groups[g][0] += ns
            groups[g][1] += calls
            if g == "topo":
                rows.append((n.split("(")[0].replace("gsr::", ""), calls, ns / calls / 1e3, ns / 1e6))
    C, reps = 160, 1 + args.reps
    det_share = 2 * C * reps / (C + 2 * C * reps)      # the GT renders of the set-up are not the detection's
    render_ms = groups["rasterizer"][0] / 1e6 * det_share / reps
    topo_ms = groups["topo"][0] / 1e6 / reps
    other_ms = groups["other"][0] / 1e6 / reps
    lines = ["", f"# rocprofv3 --kernel-trace --stats of tools/bench_topology.py --detect-only ({reps} detections), per detection:",
             f"renders (320, rasterizer kernels, GT renders of the set-up subtracted pro rata): {render_ms:.2f} ms",
             f"new topo_* kernels: {topo_ms:.3f} ms = {100 * topo_ms / render_ms:.1f} % of the renders (target <= 10 %)",
             f"other kernels (torch: the per-camera view-space z of the render colours, copies, sort, cumsum, fills; "
             f"the set-up's included): {other_ms:.3f} ms",
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
    ap.add_argument("--restated-cams", type=int, default=4)
    ap.add_argument("--detect-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_stats(args)
    elif args.detect_only:
        detect_only(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
