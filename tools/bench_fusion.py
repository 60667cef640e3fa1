"""TSDF fusion and mesh extraction at config C (60 sampled + 160 rig cameras at 1080p, level-6 icosphere): gaustar_amd.fusion.

    python tools/bench_fusion.py --out profiles/fusion_config_c.txt          # ms per fusion, mesh size, touched units
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o fusion -- python tools/bench_fusion.py --fuse-only
    python tools/bench_fusion.py --kernel-stats DIR --out profiles/fusion_config_c.txt      # appends the GPU-time split

The wall time is one fuse_mesh call (440 renders, 220 integrations, one extraction), median of --reps after a warm-up.  The
kernel split gives the GPU time of the new fusion_* kernels, their share of the 440 renders' GPU time, and the integrate
kernel's achieved bytes/s against its algorithmic bytes: touched voxels x 20 B x 2 (every plane read and written once)."""
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
    torch.cuda.synchronize()
    return model, cams


def _touched_units(model, cams) -> int:
    """Units touched, summed over the views (an instrumented pass over the same calls fuse_mesh makes; one read per view)."""
    from gaustar_amd import fusion
    renders = fusion.FusionRenders(model)
    lo, hi = renders.pts.amin(0).cpu().numpy(), renders.pts.amax(0).cpu().numpy()
    vol = fusion.TSDFVolume(lo, hi, 0.008, 0.02, model.device)
    intr0 = fusion.open3d_camera(cams[0])[0]
    views = [(cams[0].with_extrinsic(E), intr0, E) for E in fusion.sample_extrinsics()]
    views += [(c,) + fusion.open3d_camera(c) for c in cams]
    total = 0
    for cam, intr, extr in views:
        fusion.integrate_views(vol, *fusion.prepare_images(*renders(cam)), intr, extr)
        total += int(vol.touched.sum())
    return total


def run(args) -> None:
    import torch
    from gaustar_amd import fusion
    model, cams = _setup()
    res = fusion.fuse_mesh(model, cams, return_volume=True)    # warm-up
    times = []
    for _ in range(args.reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fusion.fuse_mesh(model, cams)
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    assert torch.equal(r.verts, res.verts) and torch.equal(r.faces, res.faces)
    touched = _touched_units(model, cams)
    voxels = res.tsdf.numel()
    lines = [f"# tools/bench_fusion.py at config C: {res.n_views} views ({res.n_views - len(cams)} sampled + {len(cams)} rig) "
             f"{cams[0].width}x{cams[0].height}, N={model.n_points}, voxel 0.008, sdf_trunc 0.02",
             f"fusion wall time (renders + preparation + integration + extraction), median of {args.reps}: "
             f"{1e3 * statistics.median(times):.1f} ms (min {1e3 * min(times):.1f}, max {1e3 * max(times):.1f})",
             f"volume: {res.dims} voxels = {voxels / 1e6:.1f} M, {voxels * 20 / 1e6:.0f} MB; units touched by any view: {res.n_blocks}",
             f"touched units summed over the views: {touched}",
             f"mesh: {res.verts.shape[0]} vertices, {res.faces.shape[0]} triangles",
             "launches per view: 2 renders + 4 preparation (depth, 2 max passes, prep) + memset + touch + integrate; "
             "extraction: count + 2 cumsum + emit"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)


def fuse_only(args) -> None:
    import torch
    from gaustar_amd import fusion
    model, cams = _setup()
    for _ in range(1 + args.reps):
        fusion.fuse_mesh(model, cams)
    torch.cuda.synchronize()
    print(f"fusions: {1 + args.reps}")


def kernel_stats(args) -> None:
    """Split the kernel GPU time of a --fuse-only run into the new kernels, the rasterizer's and the rest (torch)."""
    files = glob.glob(os.path.join(args.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {args.kernel_stats}")
    names = set()
    for f in glob.glob(os.path.join(ROOT, "gaustar_amd", "csrc", "*.hip")):
        if not f.endswith("gsr_fusion.hip"):
            names |= set(re.findall(r"__global__\s+void\s+(?:__launch_bounds__\([^)]*\)\s+)?(\w+)", open(f).read()))
    groups = {"fusion": [0.0, 0], "rasterizer": [0.0, 0], "other": [0.0, 0]}
    rows, integrate_ns = [], 0.0
    with open(files[0]) as fh:
        for r in csv.DictReader(fh):
            n = r["Name"].replace("(anonymous namespace)::", "")
            ns, calls = float(r["TotalDurationNs"]), int(r["Calls"])
            g = "fusion" if "fusion_" in n else ("rasterizer" if any(k in n for k in names) else "other")
            groups[g][0] += ns
            groups[g][1] += calls
            if g == "fusion":
                rows.append((n.split("(")[0].replace("gsr::", ""), calls, ns / calls / 1e3, ns / 1e6))
                if "fusion_integrate_kernel" in n:
                    integrate_ns += ns
    reps = 1 + args.reps
    render_ms, fusion_ms, other_ms = (groups[k][0] / 1e6 / reps for k in ("rasterizer", "fusion", "other"))
    lines = ["", f"# rocprofv3 --kernel-trace --stats of tools/bench_fusion.py --fuse-only ({reps} fusions), per fusion:",
             f"renders (440, rasterizer kernels): {render_ms:.2f} ms",
             f"new fusion_* kernels: {fusion_ms:.3f} ms = {100 * fusion_ms / render_ms:.1f} % of the renders",
             f"other kernels (torch: render colours, cumsum, fills, copies; the set-up's included): {other_ms:.3f} ms"]
    touched = None
    if args.out and os.path.exists(args.out):
        m = re.search(r"touched units summed over the views: (\d+)", open(args.out).read())
        touched = int(m.group(1)) if m else None
    if touched and integrate_ns:
        byts = touched * 4096 * 20 * 2
        lines.append(f"fusion_integrate_kernel: {integrate_ns / 1e6 / reps:.3f} ms per fusion for {byts / 1e9:.2f} GB of algorithmic "
                     f"traffic (touched voxels x 20 B x 2) = {byts / (integrate_ns / reps):.1f} GB/s")
    lines.append("kernel, calls (all runs), mean us, total ms (all runs):")
    lines += [f"  {n:<28} {c:>6} {a:>9.2f} {t:>9.3f}" for n, c, a, t in sorted(rows, key=lambda x: -x[3])]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "a") as fh:
            fh.write(text)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--fuse-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.kernel_stats:
        kernel_stats(args)
    elif args.fuse_only:
        fuse_only(args)
    else:
        run(args)


if __name__ == "__main__":
    main()
