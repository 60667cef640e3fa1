"""The mesh depth rasterizer (gsr_meshdepth.hip) at config C's sizes: the level-6 icosphere (81 920 faces) over the 160 cameras
of scene.ring_cameras() at 1920 x 1080.

    python tools/bench_mesh_depth.py --out profiles/mesh_depth_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  One
camera is timed through the C entry point on buffers made beforehand, with device events around --inner back-to-back calls and
no host read between them, with and without the face image: medians and the spread of --reps repeats, for three cameras of the
rig (and camera 0 for several values of the tuning parameter small_max), beside the bytes a call has to move at the least (key
image set and read, outputs written).  The rig is the 160 calls back to back between two device events, and mesh_depth.render_mesh_depth over the rig with an empty sink (its Python front end and
per-view allocations included; host clock around a run that ends in a synchronise) at 1 and 2 views in flight.  Camera 0's
images are checked against the numpy restatement tests/meshdepth_ref.py."""
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
H, W = 1080, 1920
ONE_BY_ONE = (0, 53, 159)      # cameras timed on their own
SMALL_MAX = (8, 16, 32, 64, 128, 256, 10 ** 9)      # the tuning parameter, on camera 0 (the default is 256)


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


def step(reps: int, inner: int) -> dict:
    import numpy as np
    import torch
    import meshdepth_ref as ref
    from gaustar_amd import _host, _lib, harness, mesh_depth, scene, topology
    assert torch.cuda.is_available(), "bench_mesh_depth needs a GPU"
    dev = torch.device("cuda:0")
    lib, p, st = _lib.load(), _lib.ptr, _host.raw_stream(dev.index)
    v, f = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    rig = topology.rig_from_cameras([harness.nerf_camera_from_scene(c) for c in scene.ring_cameras(W=W, H=H)])
    C, V, F = len(rig["shape"]), len(v), len(f)
    tv = torch.from_numpy(np.asarray(v, np.float64)).to(dev)
    tf = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev)
    blocks = [mesh_depth.cam16(rig["extrinsics"][i], rig["intrinsics"][i], W / 2, H / 2) for i in range(C)]
    ws = torch.empty(int(lib.gsr_mesh_depth_workspace_bytes(H, W, F)), dtype=torch.uint8, device=dev)
    depth = torch.empty(H, W, dtype=torch.float32, device=dev)
    mask = torch.empty(H, W, dtype=torch.uint8, device=dev)
    face = torch.empty(H, W, dtype=torch.int32, device=dev)
    ncl = torch.empty(1, dtype=torch.int32, device=dev)

    def call(i, faces_too, small_max=0):
        rc = lib.gsr_mesh_depth_view(H, W, V, F, p(tv), p(tf), blocks[i], 0.01, 100.0, small_max, p(ws), p(depth), p(mask),
                                     p(face) if faces_too else None, p(ncl), st)
        assert rc == 0, lib.gsr_last_error()

    out = dict(C=C, V=V, F=F, cameras={}, rig={}, front_end={}, small_max={})
    for sm in SMALL_MAX:
        ms, lo, hi = timed(lambda: call(0, False, sm), reps, inner)
        out["small_max"][str(sm)] = dict(ms=ms, lo=lo, hi=hi)
    for faces_too in (False, True):
        key = "with_faces" if faces_too else "depth_mask"
        for i in ONE_BY_ONE:
            ms, lo, hi = timed(lambda: call(i, faces_too), reps, inner)
            call(i, True)
            covered = int((face >= 0).sum())
            out["cameras"].setdefault(str(i), dict(covered=covered))[key] = dict(ms=ms, lo=lo, hi=hi)

        def whole_rig():
            for i in range(C):
                call(i, faces_too)
        ms, lo, hi = timed(whole_rig, reps)
        out["rig"][key] = dict(ms=ms, lo=lo, hi=hi)
    for vif in (1, 2):
        runs = []
        for _ in range(max(3, reps // 2) + 1):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            mesh_depth.render_mesh_depth(tv, tf, rig, lambda i, view: None, views_in_flight=vif)
            torch.cuda.synchronize()
            runs.append(1e3 * (time.perf_counter() - t0))
        runs = runs[1:]      # (the first is the warm-up)
        out["front_end"][str(vif)] = dict(ms=statistics.median(runs), lo=min(runs), hi=max(runs))
    call(0, True)
    got = (depth.cpu().numpy(), mask.cpu().numpy(), face.cpu().numpy(), int(ncl.cpu()))
    want = ref.render(np.asarray(v, np.float64), f, np.array(blocks[0][:]), H, W)
    out["same"] = bool(got[0].tobytes() == want[0].tobytes() and np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2])
                       and got[3] == want[3])
    # bytes a call has to move at the least: the key image set and read once, the outputs written once
    out["bytes"] = dict(depth_mask=8 * H * W * 2 + 5 * H * W, with_faces=8 * H * W * 2 + 9 * H * W)
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
        sys.exit(f"bench_mesh_depth: the GPU step ran past {STEP_LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_mesh_depth: the GPU step ended with status {r.returncode}\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    names = {"depth_mask": "depth + mask", "with_faces": "depth + mask + face"}
    lines = [f"# tools/bench_mesh_depth.py: config C's mesh (icosphere level 6, {res['F']} faces / {res['V']} vertices) over the {res['C']} "
             f"cameras of scene.ring_cameras() at {W} x {H}; GPU time between device events, no host read",
             f"# one camera: median of {args.reps} x {args.inner} back-to-back calls of gsr_mesh_depth_view (2 memsets + 3 kernels); "
             f"the rig: median of {args.reps} runs of {res['C']} calls back to back"]
    for i, cam in res["cameras"].items():
        for key, name in names.items():
            k, nbytes = cam[key], res["bytes"][key]
            lines.append(f"camera {i} ({cam['covered']} pixels covered), {name}: {1e3 * k['ms']:.1f} us (min {1e3 * k['lo']:.1f}, max "
                         f"{1e3 * k['hi']:.1f}); {nbytes / 1e6:.1f} MB at the least, {nbytes / k['ms'] / 1e9:.2f} TB/s")
    for key, name in names.items():
        k = res["rig"][key]
        lines.append(f"rig of {res['C']} cameras, {name}: {k['ms']:.3f} ms (min {k['lo']:.3f}, max {k['hi']:.3f}) = {1e3 * k['ms'] / res['C']:.1f} us "
                     f"per camera")
    for vif, k in res["front_end"].items():
        lines.append(f"mesh_depth.render_mesh_depth over the rig, empty sink, views_in_flight = {vif} (host clock to the final synchronise): "
                     f"{k['ms']:.2f} ms (min {k['lo']:.2f}, max {k['hi']:.2f})")
    lines.append("camera 0, depth + mask, by small_max (pixels of a range that md_face_kernel's 8 lanes still walk; the result does not depend on it): " +
                 ", ".join(f"{sm}: {1e3 * k['ms']:.1f} us" for sm, k in res["small_max"].items()))
    lines.append(f"camera 0 equal to the restatement bit for bit: {res['same']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert res["same"], "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
