"""The exact K-nearest-neighbour search (gaustar_amd.knn, gsr_knn.hip) at config C's sizes: distCUDA2 and the self-search of
the 491 520 Gaussian centres of the bench scene at K = 4 and K = 16, and the K = 8 search of the config-C mesh's vertices among
their voxel centres (warp_mesh's voxel mode, voxel_size 0.04).  Measurement only; it gates nothing.

    python tools/bench_knn.py --out profiles/knn_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  Timed
with device events around the whole call -- the Morton codes, both torch.sort calls and the searchsorted included; there is
no host read in a call without return_stats -- after a warm-up; medians and the spread of --reps repeats.  Per case: the
culling mode against the exhaustive mode (cull=False) with the counters of both, the torch composition on the same GPU
(cdist + topk over chunks of 2 048 queries; at the 491 520-point cases it is timed on the first 16 384 queries and scaled by
N / 16 384, which is said in the line), and scipy's cKDTree on the host (build + query, 16 workers, once)."""
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

LIMIT_S = 540
CHUNK = 2048
TORCH_SAMPLE = 16384


def torch_knn(q, c, K, exclude_self, first):
    """cdist + topk in chunks, squared at the end (the composition a user without the kernel would write)."""
    import torch
    out = []
    for s in range(0, q.shape[0], CHUNK):
        d = torch.cdist(q[s:s + CHUNK], c)
        if exclude_self:
            r = torch.arange(d.shape[0], device=d.device)
            d[r, first + s + r] = float("inf")
        out.append(torch.topk(d, min(K, c.shape[0]), dim=1, largest=False).indices)
    return torch.cat(out)


def case(name, q, c, K, exclude_self, reps):
    import numpy as np
    import torch
    from bench_splice import timed
    from scipy.spatial import cKDTree
    from gaustar_amd import knn
    cand = None if c is None else c
    N, M = int(q.shape[0]), int(q.shape[0] if c is None else c.shape[0])
    o = dict(name=name, N=N, M=M, K=K, exclude_self=exclude_self)
    (idx, d2), *o["cull"] = timed(lambda: knn.nearest_neighbors(q, cand, K=K, exclude_self=exclude_self), reps)
    (idx0, d20), *o["full"] = timed(lambda: knn.nearest_neighbors(q, cand, K=K, exclude_self=exclude_self, cull=False), max(2, reps // 3))
    o["same_modes"] = bool(torch.equal(idx, idx0) and torch.equal(d2.view(torch.int32), d20.view(torch.int32)))
    o["stats_cull"] = knn.nearest_neighbors(q, cand, K=K, exclude_self=exclude_self, return_stats=True)[2]
    o["stats_full"] = knn.nearest_neighbors(q, cand, K=K, exclude_self=exclude_self, cull=False, return_stats=True)[2]
    cc = q if c is None else c
    n_t = min(N, TORCH_SAMPLE)
    ti, *o["torch"] = timed(lambda: torch_knn(q[:n_t], cc, K, exclude_self, 0), 2)
    o["torch_rows"] = n_t
    kk = min(K, M - (1 if exclude_self else 0))
    o["torch_rows_equal"] = float((ti[:, :kk] == idx[:n_t, :kk]).all(1).float().mean())
    qh, ch = q.cpu().numpy().astype(np.float64), cc.cpu().numpy().astype(np.float64)
    t0 = time.perf_counter()
    tree = cKDTree(ch)
    _, ki = tree.query(qh, k=K + 1 if exclude_self else K, workers=16)
    o["kdtree_ms"] = 1e3 * (time.perf_counter() - t0)
    ki = np.asarray(ki).reshape(N, -1)
    if exclude_self:        # drop the query itself where the tree lists it (a duplicate may stand in its place: such rows differ)
        ki = np.stack([r[r != i][:K] for i, r in enumerate(ki)]) if N <= 50000 else ki[:, 1:]
    o["kdtree_rows_equal"] = float((ki[:, :kk] == idx.cpu().numpy()[:, :kk]).all(1).mean())
    return o


def step(reps: int) -> list:
    import numpy as np
    import torch
    import topo_ref as tr
    from bench_splice import timed
    from gaustar_amd import knn, scene
    assert torch.cuda.is_available(), "bench_knn needs a GPU"
    dev = torch.device("cuda:0")
    gs, _, _ = scene.config_C()
    p = torch.from_numpy(np.ascontiguousarray(gs.means3D, np.float32)).to(dev)
    out = []
    d, *ms = timed(lambda: knn.dist_cuda2(p), reps)
    out.append(dict(name="dist_cuda2", N=int(p.shape[0]), ms=ms, finite=bool(torch.isfinite(d).all()), mean=float(d.mean())))
    out.append(case("distCUDA2's search: K = 3 without the point itself", p, None, 3, True, reps))
    out.append(case("self-search, K = 4 (sugar_model.py:49)", p, None, 4, False, reps))
    out.append(case("self-search, K = 16 (reset_neighbors)", p, None, 16, False, reps))
    v, _ = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    v32 = v.astype(np.float32)
    _, centre, _ = tr.voxel_grid(v32.astype(np.float64), np.zeros(len(v32)), 0.04)
    out.append(case("mesh vertices among their voxel centres (voxel_size 0.04), K = 8", torch.from_numpy(v32).to(dev),
                    torch.from_numpy(centre.astype(np.float32)).to(dev), 8, False, reps))
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
        sys.exit(f"bench_knn: ran past {LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_knn: ended with status {r.returncode}\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    f = lambda x: f"{x[0]:.3f} ms (min {x[1]:.3f}, max {x[2]:.3f})"
    lines = [f"# tools/bench_knn.py at config C's sizes; f32; device events around the whole call (Morton codes, sorts and searchsorted "
             f"included; no host read); median of {args.reps} (exhaustive mode: of {max(2, args.reps // 3)}; torch: of 2)"]
    ok = True
    for o in res:
        if o["name"] == "dist_cuda2":
            lines.append(f"dist_cuda2 of the {o['N']} Gaussian centres (search K = 3 without self + mean): {f(o['ms'])}; all finite: "
                         f"{o['finite']}; mean {o['mean']:.4e}")
            continue
        N, M, K = o["N"], o["M"], o["K"]
        sc, sf = o["stats_cull"], o["stats_full"]
        scale = N / o["torch_rows"]
        lines += [f"## {o['name']}: N = {N}, M = {M}, K = {K}",
                  f"culling:    {f(o['cull'])}; pairs {sc['pairs']} = {100.0 * sc['pairs'] / max(N * M, 1):.3f} % of N M, tiles skipped "
                  f"{sc['tiles_skipped']}",
                  f"exhaustive: {f(o['full'])}; pairs {sf['pairs']}, tiles skipped {sf['tiles_skipped']}; same bits as culling: "
                  f"{o['same_modes']}",
                  f"torch cdist + topk, chunks of {CHUNK} queries, on {o['torch_rows']} queries: {f(o['torch'])}"
                  + (f" -> x {scale:.0f} = {o['torch'][0] * scale:.0f} ms for all N (scaled, not run)" if scale > 1 else "")
                  + f"; rows with the same indices: {100.0 * o['torch_rows_equal']:.2f} %",
                  f"scipy cKDTree on the host, f64, build + query, 16 workers, once: {o['kdtree_ms']:.0f} ms; rows with the same "
                  f"indices: {100.0 * o['kdtree_rows_equal']:.2f} %"]
        ok = ok and o["same_modes"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert ok, "the culling and the exhaustive mode disagree"


if __name__ == "__main__":
    main()
