"""tools/bench_mesh_reg.py [--iters N] [--out FILE] -- the surface-mesh regularisers of refine.py:676-706 at config-C size
(icosphere level 6: V = 40 962, F = 81 920, E = 122 880, Q = 122 880 face pairs) on one GPU:

  fused     losses.surface_mesh_loss forward + backward (gsr_mesh_reg_forward: element pass + finalise, gsr_mesh_reg_backward:
            one vertex-major pass): GPU time of the `loss_kernels` profiler stage and stream-event time per call;
  composed  the same three terms as torch operations the way pytorch3d computes them per iteration (edges_packed's sort +
            unique, mesh_normal_consistency's sort + bincount + face pairs -- built vectorised here, pytorch3d builds them in a
            Python loop -- then gathers, cross products, cosine_similarity and autograd's backward): stream-event time;
  window    tools/bench_window.py's loop at config-C size with and without --mesh-reg (autograd and --fused-step routes).

Prints one JSON line; --out also writes it, one key per line, to a text file (profiles/mesh_reg_config_c.txt)."""
import argparse, ctypes, json, os, sys
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
from gaustar_amd import _lib, losses, meshes, scene

FACTORS = dict(nc_factor=0.5, edge_factor=1000.0, area_factor=5000.0)   # train_seq.py:108-110


def composed_loss(verts, faces, ref_edge_len, ref_area, nc_factor, edge_factor, area_factor):
    """pytorch3d's per-call work restated in torch (one mesh, every edge of a closed manifold shared by two faces)."""
    V, F = verts.shape[0], faces.shape[0]
    v0, v1, v2 = faces.chunk(3, dim=1)
    e = torch.cat([torch.cat([v1, v2], 1), torch.cat([v2, v0], 1), torch.cat([v0, v1], 1)], 0).sort(dim=1)[0]
    u, inverse = torch.unique(V * e[:, 0] + e[:, 1], return_inverse=True)
    edges = torch.stack([u // V, u % V], 1)
    face_to_edge = inverse[torch.arange(3 * F, device=faces.device).view(3, F).t()]
    edge_idx, order = face_to_edge.reshape(-1).sort()
    vert_idx = faces.view(1, F, 3).expand(3, F, 3).transpose(0, 1).reshape(3 * F, 3)[order]
    num = edge_idx.bincount(minlength=edges.shape[0])
    pairs = torch.stack([torch.cumsum(num, 0) - num, torch.cumsum(num, 0) - num + 1], 1)   # (two faces per edge)
    a, b = verts[edges[edge_idx, 0]], verts[edges[edge_idx, 1]]
    n = sum(torch.linalg.cross(b - a, verts[vert_idx[:, k]] - a, dim=1) for k in range(3))
    nc = (1 - torch.nn.functional.cosine_similarity(n[pairs[:, 0]], -n[pairs[:, 1]], dim=1)).mean()
    ve = verts[edges]
    edge = (((ve[:, 0] - ve[:, 1]).norm(dim=1, p=2) - ref_edge_len) ** 2).mean()
    fv = verts[faces]
    area = (0.5 * torch.linalg.cross(fv[:, 1] - fv[:, 0], fv[:, 2] - fv[:, 0], dim=1).norm(dim=1) - ref_area).abs().mean()
    return nc_factor * nc + edge_factor * edge + area_factor * area


def timed(fn, iters, reps=5):
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(iters):
            fn()
        b.record(); torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / iters * 1e3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-window", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    lib = _lib.load()
    v, f = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    faces = torch.from_numpy(f).long().to(dev)
    v_ref = torch.from_numpy(v).float().to(dev)
    ref_mesh = meshes.Meshes(verts=[v_ref], faces=[faces])
    ve = v_ref[ref_mesh.edges_packed()]
    ref_edge_len, ref_area = (ve[:, 0] - ve[:, 1]).norm(dim=1), ref_mesh.faces_areas_packed()
    edge = float(ref_edge_len.mean())
    g = torch.Generator(device=dev).manual_seed(0)
    verts = (v_ref + 0.3 * edge * torch.randn(v_ref.shape, device=dev, generator=g)).requires_grad_(True)
    topo = meshes.MeshTopology.of(faces, verts.shape[0])
    one = torch.ones((), device=dev)

    def fused():
        verts.grad = None
        losses.surface_mesh_loss(verts, topo, ref_edge_len=ref_edge_len, ref_area=ref_area, **FACTORS).backward(one)

    def composed():
        verts.grad = None
        composed_loss(verts, faces, ref_edge_len, ref_area, **FACTORS).backward(one)

    for _ in range(20):
        fused(); composed()
    torch.cuda.synchronize()
    fused(); g_f = verts.grad.clone()
    composed(); g_c = verts.grad.clone()
    lf = float(losses.surface_mesh_loss(verts.detach(), topo, ref_edge_len=ref_edge_len, ref_area=ref_area, **FACTORS))
    lc = float(composed_loss(verts.detach(), faces, ref_edge_len, ref_area, **FACTORS))
    us_fused, us_comp = timed(fused, a.iters), timed(composed, a.iters)
    # GPU time of the two passes: the loss_kernels stage (HIP events around each launch group)
    nst = lib.gsr_num_stages()
    names = [lib.gsr_stage_name(i).decode() for i in range(nst)]
    ms, cnt = (ctypes.c_float * nst)(), (ctypes.c_int * nst)()
    lib.gsr_profile_read(ms, cnt, 1)
    lib.gsr_profile_enable(1)
    for _ in range(a.iters):
        fused()
    torch.cuda.synchronize()
    _lib.check(lib.gsr_profile_read(ms, cnt, 1), "gsr_profile_read")
    lib.gsr_profile_enable(0)
    k = names.index("loss_kernels")
    stage_us = ms[k] / a.iters * 1e3
    wsb = lib.gsr_mesh_reg_workspace_bytes(topo.V, topo.F, topo.E, topo.Q)
    # bytes of one pass (each array read once): verts, topology arrays, references, gradient out
    fwd_b = 12 * topo.V + 12 * topo.F + 8 * topo.E + 16 * topo.Q + 4 * (topo.E + topo.F)
    bwd_b = fwd_b + 4 * (topo.V + 1) + 4 * int(topo.csr_entries.numel()) + 12 * topo.V
    r = {"what": "surface-mesh regularisers (normal consistency + edge / area isometry) forward + backward, config C mesh",
         "V": topo.V, "F": topo.F, "E": topo.E, "Q": topo.Q, "incidences": int(topo.csr_entries.numel()),
         "factors": FACTORS, "iters": a.iters,
         "fused_gpu_us_loss_kernels_stage": round(stage_us, 2), "fused_launches_per_call": cnt[k] / a.iters,
         "fused_stream_us_per_call": [round(x, 2) for x in us_fused],
         "composed_stream_us_per_call": [round(x, 2) for x in us_comp],
         "speedup_stream_median": round(float(np.median(us_comp) / np.median(us_fused)), 2),
         "loss_fused": lf, "loss_composed": lc,
         "grad_normalised_max_diff": float((g_f - g_c).abs().max() / g_c.abs().max()),
         "bytes_fwd_pass": fwd_b, "bytes_bwd_pass": bwd_b, "workspace_bytes": int(wsb)}
    if not a.no_window:
        import bench_window
        w = {}
        for fused_step in (False, True):
            for reg in (False, True):
                res = bench_window.run(argparse.Namespace(frames=2, iters=50, level=6, width=1920, height=1080, cameras=160,
                                                          fused_step=fused_step, mesh_reg=reg))
                w[("fused_step" if fused_step else "autograd") + ("_mesh_reg" if reg else "")] = {
                    "median_ms_per_iteration": res["median_ms_per_iteration"], "ms_per_iteration": res["ms_per_iteration"],
                    "loss_last": [fr["loss_last"] for fr in res["frames"]]}
        r["window"] = w
        r["window_ratio_autograd"] = round(w["autograd_mesh_reg"]["median_ms_per_iteration"] / w["autograd"]["median_ms_per_iteration"], 3)
        r["window_ratio_fused_step"] = round(w["fused_step_mesh_reg"]["median_ms_per_iteration"] / w["fused_step"]["median_ms_per_iteration"], 3)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# tools/bench_mesh_reg.py on one MI355X (us = microseconds per forward + backward call)\n")
            for key, val in r.items():
                fh.write(f"{key}: {json.dumps(val)}\n")


if __name__ == "__main__":
    main()
