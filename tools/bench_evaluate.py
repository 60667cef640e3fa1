"""gaustar_amd.evaluate at config C's size: the updated mesh tools/bench_splice.py builds (98 288 faces) scored against the base
mesh it came from (a level-6 icosphere, 81 920 faces), and the model on that base mesh scored over the 160-camera rig.
Measurement only; it gates nothing.

    python tools/bench_evaluate.py --out profiles/evaluate_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  Timed
with device events around the calls (their one host read included), after a warm-up; medians and the spread of --reps repeats.
  * surface_distance: 100 000 samples of the base mesh against the updated mesh, about 10^10 point-triangle pairs; and the
    search kernel alone, its face records gathered before and nothing read back.
  * For scale, tracking's nearest-centre search (track_nn_kernel) for the same queries over the same faces' centres.
  * mesh_distance both ways with 100 000 samples each; image_metrics at 1080p; evaluate_views over the rig, two views in flight,
    against one constant ground-truth image (the renders are what costs).
  * The numpy restatement (tests/eval_ref.py) of surface_distance on the host for --host-queries of the queries, once, and
    whether the device gave those queries the same bits."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMIT_S = 900
N_SAMPLES = 100_000


def step(reps: int, host_queries: int, views: int) -> dict:
    import numpy as np
    import torch
    import eval_ref as ref
    from bench_splice import inputs, timed
    from gaustar_amd import _lib, evaluate, harness, regions, scene
    from gaustar_amd._host import stream_of
    from gaustar_amd._lib import ptr as p
    assert torch.cuda.is_available(), "bench_evaluate needs a GPU"
    dev = torch.device("cuda:0")
    bv, bf, fv, ff, raw = inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    sel = regions.UpdateRegions(component=none, region=none, n_components=2, n_regions=2, labels=np.arange(2, dtype=np.int32),
                                counts=np.full(2, 100, np.int32), raw_boxes=raw.copy())

    class Mesh:
        verts, faces = t(fv), t(ff)

    tv, tf = t(bv), t(bf)
    upd = regions.update_mesh_topology(tv, tf, sel, Mesh)
    base, result = (tv.double(), tf), (upd.verts.double(), upd.faces)
    F = int(upd.faces.shape[0])
    out = dict(F_base=len(bf), F=F, n=N_SAMPLES)

    smp = evaluate.sample_surface(*base, N_SAMPLES, seed=0)
    hit, *out["surface_distance"] = timed(lambda: evaluate.surface_distance(smp.points, *result), reps)
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    tri = evaluate._face_records(*result, err)
    _, *out["closest_kernel"] = timed(lambda: evaluate._closest(smp.points, tri, err), reps)

    lib, centres = _lib.load(), torch.empty(F, 3, dtype=torch.float64, device=dev)
    idx = torch.empty(N_SAMPLES, dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_track_centres(F, int(result[0].shape[0]), p(result[1]), p(result[0]), p(centres), p(err), stream_of(centres)), "centres")
    nn = lambda: _lib.check(lib.gsr_track_nearest(N_SAMPLES, None, None, F, p(smp.points), p(centres), p(idx), stream_of(idx)), "nearest")
    _, *out["track_nn"] = timed(nn, reps)

    md, *out["mesh_distance"] = timed(lambda: evaluate.mesh_distance(result, base, n_samples=N_SAMPLES), reps)
    out["md"] = dict(chamfer=md.chamfer, mean_ab=md.a_to_b.mean, mean_ba=md.b_to_a.mean, max_ab=md.a_to_b.max, max_ba=md.b_to_a.max,
                     fscore=list(md.fscore), thresholds=list(md.thresholds))

    g = torch.Generator(device=dev).manual_seed(0)
    a, b = (torch.rand(3, 1080, 1920, device=dev, generator=g) for _ in range(2))
    im, *out["image_metrics"] = timed(lambda: evaluate.image_metrics(a, b), reps)
    out["psnr_1080p"] = im.psnr

    model = harness.SurfaceGaussians(tv, tf.long(), n_gaussians_per_surface_triangle=6, sh_levels=4).to(dev)
    cams = [harness.nerf_camera_from_scene(c) for c in scene.ring_cameras()][:views]
    grey = torch.full((3, cams[0].rasterizer_camera().H, cams[0].rasterizer_camera().W), 0.5, device=dev)
    vm, *out["evaluate_views"] = timed(lambda: evaluate.evaluate_views(model, cams, lambda i: grey), reps)
    out["views"], out["gaussians"], out["mean_psnr"] = len(cams), int(model.n_points), vm.mean_psnr

    rows = np.linspace(0, N_SAMPLES - 1, host_queries).astype(np.int64)
    pts_h, v_h, f_h = smp.points.cpu().numpy()[rows], result[0].cpu().numpy(), result[1].cpu().numpy()
    t0 = time.perf_counter()
    want = ref.surface_distance(pts_h, v_h, f_h, block=16)
    out["host_ms"], out["host_queries"] = 1e3 * (time.perf_counter() - t0), host_queries
    got = [x.cpu().numpy()[rows] for x in hit]
    out["same"] = bool(np.array_equal(got[1], want[1]) and all(g_.tobytes() == w_.tobytes() for g_, w_ in zip(got, want)))
    return out


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--host-queries", type=int, default=64)
    ap.add_argument("--views", type=int, default=160)
    ap.add_argument("--step", action="store_true", help="(internal) run the GPU work and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(step(args.reps, args.host_queries, args.views)))
        return
    try:
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", "--reps", str(args.reps), "--host-queries",
                            str(args.host_queries), "--views", str(args.views)], capture_output=True, text=True, timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_evaluate: ran past {LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_evaluate: ended with status {r.returncode}\n{r.stderr[-2000:]}")
    o = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    f = lambda x: f"{x[0]:.3f} ms (min {x[1]:.3f}, max {x[2]:.3f})"
    pairs = o["n"] * o["F"]
    md = o["md"]
    lines = [f"# tools/bench_evaluate.py at config C's size: the updated mesh tools/bench_splice.py builds ({o['F']} faces) against its base "
             f"mesh ({o['F_base']} faces); float64 throughout; median of {args.reps}",
             f"surface_distance, {o['n']} samples of the base mesh against the updated mesh, {pairs / 1e9:.2f} x 10^9 point-triangle pairs, "
             f"face records and host read included: {f(o['surface_distance'])}",
             f"the search kernel alone (eval_closest_kernel): {f(o['closest_kernel'])} = "
             f"{pairs / o['closest_kernel'][0] / 1e6:.0f} x 10^9 pairs/s",
             f"for scale, tracking's nearest-centre search (track_nn_kernel), the same queries over the same faces' centres: {f(o['track_nn'])}",
             f"mesh_distance both ways, {o['n']} samples each, one host read: {f(o['mesh_distance'])}",
             f"  its result: chamfer {md['chamfer']:.6g}, mean result->base {md['mean_ab']:.6g} (max {md['max_ab']:.6g}), base->result "
             f"{md['mean_ba']:.6g} (max {md['max_ba']:.6g}), F-score {md['fscore']} at {md['thresholds']}",
             f"image_metrics at 3 x 1080 x 1920 (SSE, SSIM, one host read): {f(o['image_metrics'])}; psnr of two uniform noise images "
             f"{o['psnr_1080p']:.4f} dB",
             f"evaluate_views, {o['views']} cameras of the rig at 1080p, {o['gaussians']} Gaussians, two views in flight: {f(o['evaluate_views'])} = "
             f"{o['evaluate_views'][0] / o['views']:.3f} ms per view; mean psnr against a grey image {o['mean_psnr']:.3f} dB",
             f"numpy restatement of surface_distance for {o['host_queries']} of the queries, on the host, once: {o['host_ms']:.0f} ms "
             f"= {o['host_ms'] / o['host_queries'] * o['n'] / 1e3:.0f} s for all {o['n']}",
             f"those queries equal to the restatement, bit for bit: {o['same']}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert o["same"], "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
