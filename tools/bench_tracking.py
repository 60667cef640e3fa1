"""Dense surface tracking at config C's size: every face of the base mesh (a level-6 icosphere, K = 81 920 points) followed
through the update tools/bench_splice.py builds (81 920 -> 98 288 faces): gaustar_amd.tracking.SurfaceTracker.positions and
.rebind.  Measurement only; it gates nothing.

    python tools/bench_tracking.py --out profiles/tracking_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  Timed
with device events around the calls (rebind's one host read included), after a warm-up; medians and the spread of --reps
repeats.  rebind is timed on the update's own mask and on a mask that displaces every point, the search's worst case.  Next to
them the wall time of the numpy restatement (tests/tracking_ref.py) of the same rebind call on the host, once: it stands in for
the reference's trimesh loop, which is not installed here and so cannot be timed itself."""
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


def step(reps: int) -> dict:
    import numpy as np
    import torch
    import tracking_ref as ref
    from bench_splice import inputs, timed
    from gaustar_amd import regions, tracking
    assert torch.cuda.is_available(), "bench_tracking needs a GPU"
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
    K = len(bf)
    bary = np.random.default_rng(0).dirichlet(np.ones(3), size=K)
    tr = tracking.SurfaceTracker(np.arange(K, dtype=np.int32), bary, device=dev)
    ids0, bary0 = tr.face_ids, tr.face_bary                      # (rebind replaces the tensors, it does not write into them)
    v64 = tv.double()
    pos, ms_pos, lo_pos, hi_pos = timed(lambda: tr.positions(v64, tf), reps)
    nv64 = upd.verts.double()
    gone = torch.zeros_like(upd.track_face_mask)

    def rebind(mask):
        tr.face_ids, tr.face_bary = ids0, bary0
        return tr.rebind(pos, mask, nv64, upd.faces)

    out = dict(K=K, F1=int(upd.faces.shape[0]), pos=(ms_pos, lo_pos, hi_pos))
    for name, mask in (("update", upd.track_face_mask), ("all", gone)):
        stats, ms, lo, hi = timed(lambda: rebind(mask), reps)
        out[name], out[f"{name}_stats"] = (ms, lo, hi), list(stats)
    stats = rebind(upd.track_face_mask)
    got_ids, got_bary = tr.face_ids.cpu().numpy(), tr.face_bary.cpu().numpy()
    pos_h = pos.cpu().numpy()
    args = (np.arange(K, dtype=np.int32), bary, pos_h, upd.track_face_mask.cpu().numpy(), nv64.cpu().numpy(), upd.faces.cpu().numpy())
    t0 = time.perf_counter()
    want_ids, want_bary, want_stats = ref.rebind(*args)
    out["host_ms"] = 1e3 * (time.perf_counter() - t0)
    out["same"] = bool(np.array_equal(got_ids, want_ids) and got_bary.tobytes() == want_bary.tobytes() and tuple(stats) == want_stats
                       and pos_h.tobytes() == ref.positions(bv.astype(np.float64), bf, args[0], bary).tobytes())
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
                           timeout=LIMIT_S)
    except subprocess.TimeoutExpired:
        sys.exit(f"bench_tracking: ran past {LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_tracking: ended with status {r.returncode}\n{r.stderr[-2000:]}")
    o = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    K = o["K"]
    f = lambda x: f"{x[0]:.3f} ms (min {x[1]:.3f}, max {x[2]:.3f})"
    share = lambda s: " / ".join(f"{100.0 * v / K:.1f} %" for v in s)
    lines = [f"# tools/bench_tracking.py at config C's size: dense tracker, K = {K} points (every face of a level-6 icosphere), through the "
             f"update tools/bench_splice.py builds, {K} -> {o['F1']} faces; float64 throughout; median of {args.reps}",
             f"positions: {f(o['pos'])}",
             f"rebind on the update's mask, kept / moved / lost = {' / '.join(map(str, o['update_stats']))} ({share(o['update_stats'])}), "
             f"host read included: {f(o['update'])}",
             f"rebind with every face removed, kept / moved / lost = {' / '.join(map(str, o['all_stats']))}: all {K} points search all "
             f"{o['F1']} centres, {K * o['F1'] / 1e9:.2f} x 10^9 distances: {f(o['all'])}",
             f"numpy restatement of the rebind on the update's mask, on the host, once: {o['host_ms']:.0f} ms "
             "(the reference's trimesh loop is not installed and was not timed)",
             f"results equal to the restatement, bit for bit: {o['same']}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert o["same"], "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
