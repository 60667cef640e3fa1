"""The density field (gaustar_amd.density, gsr_density.hip) and SurfaceGaussians.postprocess_mesh at config C's sizes:
compute_density for 10^5 and 10^6 random surface samples against the 491 520 Gaussians of the bench scene at K = 16, the
search, the packing and the evaluation timed separately, and postprocess_mesh(5, 0.1) on the config-C mesh with one box cut
out of it (regions.cut_mesh_by_box), so that it has a rim.  Measurement only; it gates nothing.

    python tools/bench_density.py --out profiles/density_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  Timed
with device events after a warm-up; medians and the spread of --reps repeats.  The baseline is the f32 torch composition of
the same expressions on the same GPU (sugar_model.py:1024-1035 and refined_mesh.py:1163-1182 as written, with the package's
own search for knn_points: torch has none), in chunks of 2^17 queries so that its [Q,K,3,3] gather fits."""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

LIMIT_S = 540
CHUNK = 1 << 17
RECORD_BYTES = 48


def torch_density(x, idx, points, inv_sr, strengths):
    """:1024-1035 in f32, by chunks of queries."""
    import torch
    out = []
    for s in range(0, x.shape[0], CHUNK):
        i = idx[s:s + CHUNK]
        shift = x[s:s + CHUNK, None] - points[i]
        w = (inv_sr[i].transpose(-1, -2) @ shift[..., None])[..., 0]
        m = (w * w).sum(-1).clamp(min=0., max=1e8)
        out.append((strengths[i][..., 0] * torch.exp(-0.5 * m)).sum(-1))
    return torch.cat(out)


def torch_postprocess(model, iterations, threshold):
    """refined_mesh.py:1163-1182 with every face inside at the start: the peel by torch.unique counts, the restore by the f32
    composition at the removed centres -> the face mask."""
    import torch
    from gaustar_amd import density
    faces, verts = model._surface_mesh_faces, model._points.detach()
    e = torch.stack([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 1).sort(dim=-1)[0]
    key = e[..., 0] * int(verts.shape[0]) + e[..., 1]
    mask = torch.ones(faces.shape[0], dtype=torch.bool, device=faces.device)
    for _ in range(iterations):
        k = key[mask]
        _, inv, cnt = torch.unique(k.reshape(-1), return_inverse=True, return_counts=True)
        mask[mask.clone()] = (cnt[inv].view(-1, 3) >= 2).all(-1)
    centres = verts[faces].mean(-2)[~mask]
    pts = model.points.detach()
    idx = density.closest_gaussians(centres, pts, 16).long().clamp_(min=0)
    inv_sr = model.get_covariance(return_full_matrix=True, return_sqrt=True, inverse_scales=True)
    mask[~mask.clone()] = torch_density(centres, idx, pts, inv_sr, model.strengths.detach()) > threshold
    return mask


def step(reps: int) -> dict:
    import numpy as np
    import torch
    from bench_splice import timed
    from gaustar_amd import density, regions, scene
    from gaustar_amd.harness import SurfaceGaussians
    assert torch.cuda.is_available(), "bench_density needs a GPU"
    dev = torch.device("cuda:0")
    t = lambda a, d=np.float32: torch.from_numpy(np.ascontiguousarray(a, d)).to(dev)
    gs = scene.config_C()[0]
    pts, sc, qt, w = t(gs.means3D), t(gs.scales), t(gs.rotations), t(gs.opacities)
    v, f = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    rng = np.random.default_rng(0)
    out = dict(P=int(pts.shape[0]), cases=[])
    inv_sr = density.get_covariance(sc, qt, return_full_matrix=True, return_sqrt=True, inverse_scales=True)
    for Q in (100_000, 1_000_000):
        b = rng.dirichlet((1, 1, 1), Q)
        x = t(np.einsum("qvc,qv->qc", v[f[rng.integers(0, len(f), Q)]], b))
        o = dict(Q=Q, K=16)
        d, *o["whole"] = timed(lambda: density.compute_density(x, pts, sc, qt, w), reps)
        idx, *o["search"] = timed(lambda: density.closest_gaussians(x, pts, 16), reps)
        rec, *o["pack"] = timed(lambda: density.pack_records(pts, sc, qt, w), reps)
        err = torch.zeros(1, dtype=torch.int32, device=dev)
        (d2, _), *o["eval"] = timed(lambda: density.eval_records(x, idx, rec, 1.0, False, err), reps)
        (_, _), *o["eval_opac"] = timed(lambda: density.eval_records(x, idx, rec, 1.0, True, err), reps)
        o["same_bits"] = bool(torch.equal(d.view(torch.int32), d2.view(torch.int32)))
        il = idx.long().clamp_(min=0)
        ref, *o["torch"] = timed(lambda: torch_density(x, il, pts, inv_sr, w), max(2, reps // 3))
        o["max_abs_diff_to_torch"] = float((ref - d).abs().max())
        o["density_range"] = [float(d.min()), float(d.max())]
        o["gathered_bytes"] = Q * 16 * RECORD_BYTES
        out["cases"].append(o)
    # the config-C mesh with a box cut out of its front
    cut = regions.cut_mesh_by_box(t(v), t(f, np.int32), np.array([[-0.3, 0.9, 0.5], [0.3, 1.5, 1.5]]), True)
    model = SurfaceGaussians(cut.verts, cut.faces.long(), n_gaussians_per_surface_triangle=6)
    op = rng.uniform(0.001, 0.1, (model.n_points, 1))
    with torch.no_grad():
        model.all_densities.copy_(t(np.log(op / (1 - op))))
    res, *ms = timed(lambda: model.postprocess_mesh(5, 0.1), reps)
    mask, *ms_t = timed(lambda: torch_postprocess(model, 5, 0.1), max(2, reps // 3))
    out["post"] = dict(F=int(cut.faces.shape[0]), N=model.n_points, ms=ms, torch=ms_t, kept=res.kept_per_iteration, restored=res.restored,
                       left=int(res.face_mask.sum()), masks_differ=int((mask != res.face_mask).sum()))
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
        sys.exit(f"bench_density: ran past {LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_density: ended with status {r.returncode}\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    f = lambda x: f"{x[0]:.3f} ms (min {x[1]:.3f}, max {x[2]:.3f})"
    nt = max(2, args.reps // 3)
    lines = [f"# tools/bench_density.py at config C's sizes: {res['P']} Gaussians, K = 16, f32 in, f64 terms; device events; median of "
             f"{args.reps} (torch baseline: of {nt})"]
    for o in res["cases"]:
        gb = o["gathered_bytes"] / 1e9
        lines += [f"## compute_density, Q = {o['Q']} random surface samples",
                  f"whole call (pack + search + evaluation, no host read): {f(o['whole'])}",
                  f"search (Morton codes, sorts, gsr_knn_search):          {f(o['search'])}",
                  f"gsr_density_pack ({res['P']} records):                  {f(o['pack'])}",
                  f"gsr_density_eval, density only:                        {f(o['eval'])} = {gb / (o['eval'][0] * 1e-3):.0f} GB/s of the "
                  f"{gb:.3f} GB of records a query's lanes gather (most of them from cache: neighbouring samples share neighbours)",
                  f"gsr_density_eval with neighbor_opacities:              {f(o['eval_opac'])}",
                  f"separate calls give the whole call's bits: {o['same_bits']}",
                  f"torch f32 composition of :1024-1035 on the same indices, chunks of {CHUNK}: {f(o['torch'])} = "
                  f"{o['torch'][0] / o['eval'][0]:.1f} x the evaluation kernel; largest |difference| {o['max_abs_diff_to_torch']:.2e} on "
                  f"densities from {o['density_range'][0]:.2e} to {o['density_range'][1]:.3g}"]
    p = res["post"]
    lines += [f"## postprocess_mesh(5, 0.1) on the config-C mesh without the faces with a vertex in one box: {p['F']} faces, {p['N']} Gaussians",
              f"postprocess_mesh (5 edge counts, centres, pack + search + evaluation, one host read, the new model): {f(p['ms'])}",
              f"kept per iteration {p['kept']}, restored {p['restored']}, faces left {p['left']}",
              f"torch composition (unique counts, boolean indexing, f32 density; the same search): {f(p['torch'])}; faces whose mask "
              f"differs: {p['masks_differ']}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert all(o["same_bits"] for o in res["cases"]), "separate calls and the whole call disagree"


if __name__ == "__main__":
    main()
