"""Hole filling and the whole topology update at config C's size (base mesh: a level-6 icosphere = 81 920 faces; fused surface: a
level-7 icosphere a little outside it, rotated; two regions, around the poles): gaustar_amd.regions.fill_small_holes and
update_mesh_topology.

    python tools/bench_splice.py --out profiles/splice_config_c.txt

Every GPU step runs in a child process of its own under a time limit; a step that fails, faults or runs out of time ends the
run there and nothing more is started.  Timed with device events around the calls (host reads included where the call has
them), after a warm-up; medians and the spread of --reps repeats.  Next to them the wall time of the numpy restatement
(tests/splice_ref.py) on the same inputs on the host, once: it stands in for the reference's trimesh / networkx path, which is
not installed here and so cannot be timed itself."""
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

STEP_LIMIT_S = {"fill": 240, "update": 420}
HOLES = 400          # faces taken out of the base mesh for the hole-filling step, far apart


def inputs():
    """(base verts, base faces, fusion verts, fusion faces, raw boxes [2,2,3]), numpy."""
    import numpy as np
    from gaustar_amd import scene
    c, r = np.asarray(scene.SUBJECT_CENTER, np.float64), float(scene.SUBJECT_RADIUS)
    bv, bf = scene.icosphere(6, r, scene.SUBJECT_CENTER)
    fv, ff = scene.icosphere(7, r * 1.004, scene.SUBJECT_CENTER)
    a = 0.3
    rot = np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
    fv = (np.asarray(fv, np.float64) - c) @ rot.T + c
    h = 0.3 * r
    raw = np.stack([np.stack([c + [-h, -h, 0.8 * r], c + [h, h, 1.2 * r]]), np.stack([c + [-h, -h, -1.2 * r], c + [h, h, -0.8 * r]])])
    return bv.astype(np.float32), bf.astype(np.int32), fv.astype(np.float32), ff.astype(np.int32), raw


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
    import regions_ref as rr
    import splice_ref as ref
    from gaustar_amd import regions
    assert torch.cuda.is_available(), "bench_splice needs a GPU"
    dev = torch.device("cuda:0")
    bv, bf, fv, ff, raw = inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if name == "fill":
        holed = np.delete(bf, np.arange(HOLES) * (len(bf) // HOLES), axis=0)
        tf, V = t(holed), len(bv)
        got, ms, lo, hi = timed(lambda: regions.fill_small_holes(tf, V), reps)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        _o, ms_bare, lo_bare, hi_bare = timed(lambda: regions._fill(tf, V, err), reps)       # without the watertight pass
        t0 = time.perf_counter()
        want = ref.fill_small_holes(holed)
        host = time.perf_counter() - t0
        same = bool(np.array_equal(got.faces.cpu().numpy(), want["faces"]) and got.watertight == want["watertight"])
        return dict(F=len(holed), V=V, n_new=got.n_new, watertight=got.watertight, ms=ms, lo=lo, hi=hi, ms_bare=ms_bare, lo_bare=lo_bare,
                    hi_bare=hi_bare, host_ms=1e3 * host, same=same)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    sel = regions.UpdateRegions(component=none, region=none, n_components=2, n_regions=2, labels=np.arange(2, dtype=np.int32),
                                counts=np.full(2, 100, np.int32), raw_boxes=raw.copy())

    class Mesh:
        verts, faces = t(fv), t(ff)

    tv, tf = t(bv), t(bf)
    got, ms, lo, hi = timed(lambda: regions.update_mesh_topology(tv, tf, sel, Mesh), reps)
    t0 = time.perf_counter()
    want = ref.update_mesh_topology(bv, bf, 2, rr.padded_boxes(raw, 0.02), fv, ff)
    host = time.perf_counter() - t0
    same = bool(np.array_equal(got.faces.cpu().numpy(), want["faces"]) and np.array_equal(got.track_face_mask.cpu().numpy(), want["track_face_mask"])
                and got.n_spliced == want["n_spliced"] and got.max_dist_in_connection == want["max_dist_in_connection"])
    return dict(F0=len(bf), Ff=len(ff), F=int(got.faces.shape[0]), track=got.track_face_num, cc=got.cc_update_num, spliced=got.n_spliced,
                max_dist=got.max_dist_in_connection, ms=ms, lo=lo, hi=hi, host_ms=1e3 * host, same=same)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--step", default=None, choices=sorted(STEP_LIMIT_S), help="(internal) run one GPU step and print its JSON")
    args = ap.parse_args()
    if args.step:
        print("RESULT " + json.dumps(step(args.step, args.reps)))
        return
    res = {}
    for name in ("fill", "update"):       # a child per step; the first that fails ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S[name])
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_splice: step {name} ran past {STEP_LIMIT_S[name]} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"bench_splice: step {name} ended with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}")
        res[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    f, u = res["fill"], res["update"]
    lines = [f"# tools/bench_splice.py at config C's size: base mesh {u['F0']} faces (a level-6 icosphere), fused surface {u['Ff']} faces "
             "(a level-7 icosphere, rotated), two regions around the poles, aabb_pad 0.02",
             f"fill_small_holes on the base mesh without {HOLES} scattered faces ({f['F']} faces / {f['V']} vertices), median of {args.reps}: "
             f"{f['ms']:.3f} ms (min {f['lo']:.3f}, max {f['hi']:.3f}) with the watertight pass and its host reads; {f['ms_bare']:.3f} ms "
             f"(min {f['lo_bare']:.3f}, max {f['hi_bare']:.3f}) without it, as update_mesh_topology calls it; {f['n_new']} faces added, "
             f"watertight {f['watertight']}",
             f"update_mesh_topology, both boxes, median of {args.reps}: {u['ms']:.3f} ms (min {u['lo']:.3f}, max {u['hi']:.3f}), host reads "
             f"included; result {u['F']} faces, {u['track']} of them from the input, cc_update_num {u['cc']}, n_spliced {u['spliced']}, "
             f"max_dist_in_connection {u['max_dist']:.6f}",
             f"numpy restatement on the host, once: fill_small_holes {f['host_ms']:.0f} ms, update_mesh_topology {u['host_ms']:.0f} ms "
             "(the reference's trimesh / networkx path is not installed and was not timed)",
             f"results equal to the restatement: fill {f['same']}, update {u['same']}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert f["same"] and u["same"], "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
