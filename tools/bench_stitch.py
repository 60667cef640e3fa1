"""The stitch of a fused patch into the cut base mesh at config C's size (base mesh: level-6 icosphere = 81 920 faces; fused
surface: a level-7 icosphere a little outside it; the box: a slab around the equator, so both cuts have two boundary rings):
gaustar_amd.regions.connect_two_meshes and its nearest-vertex kernel.

    python tools/bench_stitch.py --out profiles/stitch_config_c.txt

Every GPU step runs in a child process of its own under a time limit; a step that fails, faults or runs out of time ends the
run there and nothing more is started.  Timed with device events around the calls (host reads included where the call has
them), after a warm-up; medians and the spread of --reps repeats.  Next to them the wall time of the numpy restatement
(tests/stitch_ref.py) on the same inputs on the host, once: it stands in for the reference's pytorch3d / trimesh / scipy path,
which is not installed here and so cannot be timed itself."""
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

STEP_LIMIT_S = {"nearest": 120, "stitch": 240}


def inputs():
    """The two cuts and their boundary lists, numpy, from the restatement of the front half."""
    import numpy as np
    import regions_ref as rr
    from gaustar_amd import scene
    c, r = np.asarray(scene.SUBJECT_CENTER, np.float64), float(scene.SUBJECT_RADIUS)
    bv, bf = scene.icosphere(6, r, scene.SUBJECT_CENTER)
    fv, ff = scene.icosphere(7, r * 1.004, scene.SUBJECT_CENTER)
    bv, fv, bf, ff = bv.astype(np.float32), fv.astype(np.float32), bf.astype(np.int32), ff.astype(np.int32)
    box = np.stack([c - [2 * r, 2 * r, 0.3 * r], c + [2 * r, 2 * r, 0.3 * r]])
    base = rr.cut_mesh_by_box(bv, bf, box, True)
    patch = rr.cut_mesh_by_box(fv, ff, box, False)

    def rim(m):         # the boundary vertices, without the restatement's per-face Python loop
        e = np.sort(np.concatenate([m["faces"][:, [0, 1]], m["faces"][:, [1, 2]], m["faces"][:, [2, 0]]]).astype(np.int64), axis=1)
        key = e[:, 0] << 32 | e[:, 1]
        uniq, count = np.unique(key, return_counts=True)
        once = uniq[count == 1]
        return np.unique(np.concatenate([once >> 32, once & 0xffffffff])).astype(np.int32)

    return base, rim(base), patch, rim(patch)


def timed(fn, reps):
    import torch
    out = fn()      # warm-up
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return out, statistics.median(ms), min(ms), max(ms)


def step(name: str, reps: int) -> dict:
    """One GPU step, in this (child) process."""
    import numpy as np
    import torch
    import stitch_ref as ref
    from gaustar_amd import regions
    assert torch.cuda.is_available(), "bench_stitch needs a GPU"
    dev = torch.device("cuda:0")
    base, b1, patch, b2 = inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if name == "nearest":
        q, c = t(patch["verts"][b2]), t(base["verts"][b1])
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        (idx, d2, _mx), ms, lo, hi = timed(lambda: regions._nearest(q, c, err), reps)          # the kernel alone: no host read
        g = torch.Generator().manual_seed(0)
        q4, c4 = torch.rand(4096, 3, generator=g).to(dev), torch.rand(4096, 3, generator=g).to(dev)
        _o, ms4, lo4, hi4 = timed(lambda: regions._nearest(q4, c4, err), reps)
        t0 = time.perf_counter()
        want_idx, want_d2 = ref.nearest_vertices(patch["verts"][b2], base["verts"][b1])
        host = time.perf_counter() - t0
        same = bool(np.array_equal(idx.cpu().numpy(), want_idx) and d2.cpu().numpy().tobytes() == want_d2.tobytes())
        return dict(Bq=len(b2), Bc=len(b1), ms=ms, lo=lo, hi=hi, ms4=ms4, lo4=lo4, hi4=hi4, host_ms=1e3 * host, same=same)
    args = [t(base["verts"]), t(base["faces"]), t(b1), t(patch["verts"]), t(patch["faces"]), t(b2)]
    got, ms, lo, hi = timed(lambda: regions.connect_two_meshes(*args), reps)
    t0 = time.perf_counter()
    want = ref.connect_two_meshes(base["verts"], base["faces"], b1, patch["verts"], patch["faces"], b2)
    host = time.perf_counter() - t0
    same = bool(np.array_equal(got.faces.cpu().numpy(), want["faces"]) and got.verts.cpu().numpy().tobytes() == want["verts"].tobytes()
                and np.array_equal(got.face_mask.cpu().numpy(), want["face_mask"]) and got.max_dist == want["max_dist"]
                and got.watertight == want["watertight"])
    return dict(F1=len(base["faces"]), V1=len(base["verts"]), F2=len(patch["faces"]), V2=len(patch["verts"]), B1=len(b1), B2=len(b2),
                F=int(got.faces.shape[0]), V=int(got.verts.shape[0]), watertight=got.watertight, max_dist=got.max_dist,
                dropped=int((~got.face_mask).sum()), ms=ms, lo=lo, hi=hi, host_ms=1e3 * host, same=same)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", default=None, choices=sorted(STEP_LIMIT_S), help="(internal) run one GPU step and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(step(args.step, args.reps)))
        return
    res = {}
    for name in ("nearest", "stitch"):       # a child per step; the first that fails ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S[name])
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_stitch: step {name} ran past {STEP_LIMIT_S[name]} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"bench_stitch: step {name} ended with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}")
        res[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    n, s = res["nearest"], res["stitch"]
    lines = [f"# tools/bench_stitch.py at config C's size: base cut {s['F1']} faces / {s['V1']} vertices (a level-6 icosphere of 81 920 "
             f"faces without an equatorial slab), patch {s['F2']} faces / {s['V2']} vertices (the slab of a level-7 icosphere); "
             f"boundary lists {s['B1']} (base) and {s['B2']} (patch) vertices",
             f"connect_two_meshes, median of {args.reps}: {s['ms']:.3f} ms (min {s['lo']:.3f}, max {s['hi']:.3f}), host reads included; "
             f"result {s['F']} faces / {s['V']} vertices, {s['dropped']} degenerate faces dropped, watertight {s['watertight']}, "
             f"max_dist {s['max_dist']:.6f}",
             f"nearest-vertex kernel alone, {n['Bq']} queries x {n['Bc']} candidates, median of {args.reps}: {n['ms']:.4f} ms "
             f"(min {n['lo']:.4f}, max {n['hi']:.4f}); 4096 x 4096: {n['ms4']:.4f} ms (min {n['lo4']:.4f}, max {n['hi4']:.4f})",
             f"numpy restatement on the host, once: connect_two_meshes {s['host_ms']:.0f} ms, nearest vertices {n['host_ms']:.1f} ms "
             "(the reference's pytorch3d / trimesh path is not installed and was not timed)",
             f"results equal to the restatement: stitch {s['same']}, nearest {n['same']}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert n["same"] and s["same"], "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
