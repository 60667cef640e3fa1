"""Shape from silhouettes (gsr_hull.hip) at config C's sizes: the level-6 icosphere rendered to 160 masks of 1920 x 1080 by
mesh_depth over scene.ring_cameras(), then carved back out of them.

    python tools/bench_hull.py --out profiles/hull_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  Timed
between device events, medians (and the spread) of --reps repeats: one image's distance map through the C entry point (--inner
back-to-back calls per repeat, three cameras); the carve of all 160 cameras in one launch at voxel 0.008 and 0.004 over the
subject's box; finish and the fusion's extraction.  hull.hull_mesh as a whole (bounds, distance maps, carve, extraction, no
smoothing or decimation) is timed by the host clock around a run that ends in a synchronise.  Beside each: the time its
least memory traffic would take at the HBM bandwidth measured for a float4 copy (6.29 TB/s), and what the numpy restatement
tests/hull_ref.py takes on the host for the same work (the carve: one camera over the 0.008 volume, times 160).  One distance
map and a 48^3 block of the 0.008 volume's state across the surface are checked against the restatement."""
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

STEP_LIMIT_S = 540
H, W = 1080, 1920
HBM_BPS = 6.29e12          # a float4 copy, measured
ONE_BY_ONE = (0, 53, 159)
VOXELS = (0.008, 0.004)
TRUNC = 0.02


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


def step(reps: int, inner: int) -> dict:
    import numpy as np
    import torch
    import hull_ref as hr
    from gaustar_amd import _host, _lib, fusion, harness, hull, mesh_depth, scene, topology
    assert torch.cuda.is_available(), "bench_hull needs a GPU"
    dev = torch.device("cuda:0")
    lib, p, st = _lib.load(), _lib.ptr, _host.raw_stream(dev.index)
    v, f = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    rig = topology.rig_from_cameras([harness.nerf_camera_from_scene(c) for c in scene.ring_cameras(W=W, H=H)])
    C = len(rig["shape"])
    masks = [None] * C
    mesh_depth.render_mesh_depth(v, f, rig, lambda i, view: masks.__setitem__(i, view.mask), views_in_flight=1)
    torch.cuda.synchronize()
    centre = np.asarray(scene.SUBJECT_CENTER, np.float64)
    lo, hi = centre - scene.SUBJECT_RADIUS, centre + scene.SUBJECT_RADIUS
    out = dict(C=C, F=len(f), distance={}, carve={}, finish={}, extract={}, same={})

    # ---- one image's distance map
    vol8 = hull.HullVolume(lo, hi, VOXELS[0], TRUNC, dev)
    top = vol8.origin + np.asarray(vol8.dims, np.float64) * vol8.voxel_size
    R = hull.radius_for(rig, vol8.origin, top, TRUNC)
    out["R"] = R
    ws = torch.empty(H * W, dtype=torch.uint8, device=dev)
    d2 = torch.empty(H, W, dtype=torch.int16, device=dev)

    def dist(i, radius):
        rc = lib.gsr_hull_mask_distance(H, W, p(masks[i]), 128, radius, p(ws), p(d2), st)
        assert rc == 0, lib.gsr_last_error()

    for radius in (R, 127):
        for i in ONE_BY_ONE:
            out["distance"][f"{i}/{radius}"] = timed(lambda: dist(i, radius), reps, inner)
    # bytes at the least: the mask read, s written and read (the column tiles' halo rows again), d2 written
    out["distance_bytes"] = {str(r): H * W * (1 + 1 + (64 + 2 * r) / 64 + 2) for r in (R, 127)}
    m0 = masks[0].cpu().numpy()
    t0 = time.perf_counter()
    want = hr.mask_distance(m0, 128, R)
    out["distance_host_s"] = time.perf_counter() - t0
    dist(0, R)
    out["same"]["distance"] = bool(np.array_equal(d2.cpu().numpy(), want))
    out["inside_pixels"] = int((m0 > 0).sum())

    # ---- the carve, finish, extraction
    maps = [hull.mask_distance(m, 128, R) for m in masks]
    shape, intr, extr = np.asarray(rig["shape"]), np.asarray(rig["intrinsics"], np.float64), np.asarray(rig["extrinsics"], np.float64)
    table = np.zeros(C, hull.CAMERA_DTYPE)
    for i in range(C):
        table[i] = (extr[i][:3, :3].reshape(-1), extr[i][:3, 3], intr[i][0, 0], intr[i][1, 1], W / 2, H / 2, maps[i].data_ptr(), H, W)
    cams = torch.from_numpy(table.view(np.uint8).reshape(-1)).to(dev)
    min_views = hull.default_min_views(C)
    for voxel in VOXELS:
        vol = vol8 if voxel == VOXELS[0] else hull.HullVolume(lo, hi, voxel, TRUNC, dev)
        n = vol.tsdf.numel()

        def carve():
            rc = lib.gsr_hull_carve(C, table.ctypes.data, p(cams), vol.voxel_size, vol.grid, p(vol.field), p(vol.count), st)
            assert rc == 0, lib.gsr_last_error()

        key = f"{voxel}"
        out["carve"][key] = dict(timed(carve, reps), voxels=n, bytes=16 * n)      # field and count read and written once
        vol.field.fill_(float("inf"))
        vol.count.zero_()
        carve()
        out["finish"][key] = dict(timed(lambda: hull.finish(vol, min_views), reps), bytes=16 * n + n // 4096)
        out["extract"][key] = dict(timed(lambda: fusion.extract_triangle_mesh(vol), reps), faces=int(fusion.extract_triangle_mesh(vol)[1].shape[0]))
        if voxel == VOXELS[0]:
            # the restatement: one camera over this volume on the host (x 160 for the rig), and a corner of the state for all
            rvol = hr.new_volume(lo, hi, voxel, TRUNC)
            cz, cy, cx = np.meshgrid(hr.centres(rvol, 2), hr.centres(rvol, 1), hr.centres(rvol, 0), indexing="ij")
            cam0 = hr.rig_cameras(rig, [want])[0]
            t0 = time.perf_counter()
            hr.view_distance(cam0, cx.reshape(-1), cy.reshape(-1), cz.reshape(-1))
            out["carve_host_s_per_camera"] = time.perf_counter() - t0
            k = 48
            mid = rvol["tsdf"].shape[0] // 2                       # (near the volume's middle in z and y, at its low end in x: the block straddles the surface)
            sub = (slice(mid, mid + k), slice(mid, mid + k), slice(0, k))
            px, py, pz = cx[sub].reshape(-1), cy[sub].reshape(-1), cz[sub].reshape(-1)
            field, count = np.full(px.shape, np.inf, np.float32), np.zeros(px.shape, np.int32)
            for cam in hr.rig_cameras(rig, [m.cpu().numpy() for m in maps]):
                ok, d = hr.view_distance(cam, px, py, pz)
                field = np.where(ok & (d < field), d, field)
                count = count + ok.astype(np.int32)
            out["same"]["carve"] = bool(vol.field[sub].cpu().numpy().reshape(-1).tobytes() == field.tobytes()
                                        and np.array_equal(vol.count[sub].cpu().numpy().reshape(-1), count))
        del vol
    del vol8, maps
    torch.cuda.empty_cache()

    # ---- the whole hull_mesh, host clock
    runs = []
    for _ in range(4):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        verts, faces = hull.hull_mesh(rig, masks, voxel_size=VOXELS[0], sdf_trunc=TRUNC, taubin_iterations=0, target_faces=0)
        torch.cuda.synchronize()
        runs.append(time.perf_counter() - t0)
    runs = runs[1:]      # (the first is the warm-up)
    out["hull_mesh"] = dict(s=statistics.median(runs), lo=min(runs), hi=max(runs), faces=int(faces.shape[0]))
    r = torch.linalg.norm(verts.double() - torch.tensor(centre, device=dev), dim=1)
    out["hull_radius"] = [float(r.min()), float(r.max())]
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
        sys.exit(f"bench_hull: the GPU step ran past {STEP_LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_hull: the GPU step ended with status {r.returncode}\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    bound = lambda nbytes: f"{1e6 * nbytes / HBM_BPS:.1f} us at {HBM_BPS / 1e12:.2f} TB/s for {nbytes / 1e6:.1f} MB"
    lines = [f"# tools/bench_hull.py: config C's mesh (icosphere level 6, {res['F']} faces) rendered to {res['C']} masks of {W} x {H} by "
             f"mesh_depth over scene.ring_cameras(), carved back; GPU time between device events unless stated, medians of {args.reps}",
             f"# distance cap R = {res['R']} (hull.radius_for the 0.008 volume); camera 0's mask has {res['inside_pixels']} inside pixels"]
    for key, k in res["distance"].items():
        i, radius = key.split("/")
        lines.append(f"distance map, camera {i}, R = {radius} (2 kernels; {args.inner} back-to-back calls a repeat): {1e3 * k['ms']:.1f} us (min "
                     f"{1e3 * k['lo']:.1f}, max {1e3 * k['hi']:.1f}); traffic bound {bound(res['distance_bytes'][radius])}")
    lines.append(f"distance map, camera 0, R = {res['R']}, numpy restatement on the host: {1e3 * res['distance_host_s']:.0f} ms")
    for key, k in res["carve"].items():
        lines.append(f"carve, voxel {key} ({k['voxels'] / 1e6:.1f} M voxels, {res['C']} cameras, one launch): {k['ms']:.2f} ms (min {k['lo']:.2f}, max "
                     f"{k['hi']:.2f}) = {1e9 * k['ms'] / k['voxels'] / res['C']:.1f} ps per voxel and camera; traffic bound {bound(k['bytes'])}")
    lines.append(f"carve, voxel {VOXELS[0]}, numpy restatement on the host: {res['carve_host_s_per_camera']:.2f} s for one camera, "
                 f"{res['carve_host_s_per_camera'] * res['C']:.0f} s for the rig at that rate")
    for key in res["finish"]:
        k, e = res["finish"][key], res["extract"][key]
        lines.append(f"finish, voxel {key}: {1e3 * k['ms']:.1f} us (min {1e3 * k['lo']:.1f}, max {1e3 * k['hi']:.1f}); traffic bound {bound(k['bytes'])}")
        lines.append(f"fusion.extract_triangle_mesh, voxel {key} ({e['faces']} faces; its scans and one host read included): {e['ms']:.2f} ms (min "
                     f"{e['lo']:.2f}, max {e['hi']:.2f})")
    k = res["hull_mesh"]
    lines.append(f"hull.hull_mesh, voxel {VOXELS[0]}, bounds from the rig alone, no smoothing or decimation, host clock to the final synchronise "
                 f"(median of 3): {k['s']:.2f} s (min {k['lo']:.2f}, max {k['hi']:.2f}); {k['faces']} faces, vertex distances from the subject's "
                 f"centre {res['hull_radius'][0]:.4f} .. {res['hull_radius'][1]:.4f} (the sphere: {0.9:.4f})")
    lines.append(f"equal to the restatement: camera 0's distance map {res['same']['distance']}, a 48^3 block of the 0.008 carve state across the surface bit for bit "
                 f"{res['same']['carve']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert all(res["same"].values()), "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
