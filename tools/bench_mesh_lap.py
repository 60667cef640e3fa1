"""tools/bench_mesh_lap.py [--iters N] [--out FILE] -- the mesh Laplacian-smoothing loss (refine.py:681-683) and the small-area
regulariser (refine.py:713-718) at config-C size (icosphere level 6: V = 40 962, F = 81 920) on one GPU, forward + backward:

  fused     losses.mesh_smoothness_loss (gsr_mesh_lap_forward + gsr_mesh_lap_backward) per method and for the area regulariser
            alone: GPU time of the `loss_kernels` profiler stage (device events around each launch group) and stream-event
            time per call, medians over repetitions;
  composed  the same terms as the f32 torch composition on the same GPU (tests/mesh_lap_ref.py on the device: the weights
            rebuilt per call as pytorch3d does, index_add over directed edges, autograd's backward): stream-event time;
  window    tools/bench_window.py's loop at config-C size with --mesh-reg and with --mesh-reg --mesh-lap (autograd and
            --fused-step routes), alternated in this one session: the first is what the loop cost before this term existed.

Prints one JSON line; --out also writes it, one key per line, to a text file (profiles/mesh_lap_config_c.txt)."""
import argparse, ctypes, json, os, sys
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT); sys.path.insert(0, HERE); sys.path.insert(0, os.path.join(ROOT, "tests"))
from gaustar_amd import _lib, losses, meshes, scene
import mesh_lap_ref as ml

LAP_FACTOR, AREG_FACTOR = 5.0, 0.1   # refine.py:122, :143
CASES = {"uniform": (LAP_FACTOR, "uniform", 0.0), "cot": (LAP_FACTOR, "cot", 0.0), "cotcurv": (LAP_FACTOR, "cotcurv", 0.0),
         "area_reg": (0.0, "uniform", AREG_FACTOR)}


def composed_loss(verts, faces, lap, method, areg):
    loss = 0.0
    if lap:
        loss = loss + lap * ml.laplacian_loss(verts, faces, method)
    if areg:
        loss = loss + areg * ml.area_reg_loss(verts, faces)
    return loss


def timed(fn, iters, reps=7):
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
    if not torch.cuda.is_available():
        raise SystemExit("tools/bench_mesh_lap.py measures on a GPU: none found")
    dev = torch.device("cuda:0")
    lib = _lib.load()
    v, f = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    faces = torch.from_numpy(f).long().to(dev)
    v_ref = torch.from_numpy(v).float().to(dev)
    edge = float((v_ref[faces[:, 0]] - v_ref[faces[:, 1]]).norm(dim=1).mean())
    g = torch.Generator(device=dev).manual_seed(0)
    verts = (v_ref + 0.3 * edge * torch.randn(v_ref.shape, device=dev, generator=g)).requires_grad_(True)
    topo = meshes.MeshTopology.of(faces, verts.shape[0])
    one = torch.ones((), device=dev)
    nst = lib.gsr_num_stages()
    names = [lib.gsr_stage_name(i).decode() for i in range(nst)]
    k = names.index("loss_kernels")
    ms, cnt = (ctypes.c_float * nst)(), (ctypes.c_int * nst)()
    n_nbr, n_vf = int(topo.vertex_neighbours[1].numel()), int(topo.vertex_face_csr[1].numel())
    r = {"what": "mesh Laplacian-smoothing loss and small-area regulariser, forward + backward, config C mesh",
         "V": topo.V, "F": topo.F, "directed_edges": n_nbr, "face_incidences": n_vf, "iters": a.iters,
         "laplacian_factor": LAP_FACTOR, "area_reg_factor": AREG_FACTOR,
         "workspace_bytes": int(lib.gsr_mesh_lap_workspace_bytes(topo.V, topo.F))}
    for name, (lap, method, areg) in CASES.items():
        def fused():
            verts.grad = None
            losses.mesh_smoothness_loss(verts, topo, lap, method, areg).backward(one)

        def composed():
            verts.grad = None
            composed_loss(verts, faces, lap, method, areg).backward(one)

        for _ in range(20):
            fused(); composed()
        torch.cuda.synchronize()
        fused(); g_f = verts.grad.clone()
        composed(); g_c = verts.grad.clone()
        lf = float(losses.mesh_smoothness_loss(verts.detach(), topo, lap, method, areg))
        lc = float(composed_loss(verts.detach(), faces, lap, method, areg))
        us_f, us_c = [], []
        for _ in range(3):                      # the two alternated: other work shares the machine
            us_f += timed(fused, a.iters, 3); us_c += timed(composed, a.iters, 3)
        lib.gsr_profile_read(ms, cnt, 1)
        lib.gsr_profile_enable(1)
        for _ in range(a.iters):
            fused()
        torch.cuda.synchronize()
        _lib.check(lib.gsr_profile_read(ms, cnt, 1), "gsr_profile_read")
        lib.gsr_profile_enable(0)
        r[name] = {"fused_gpu_us_loss_kernels_stage": round(ms[k] / a.iters * 1e3, 2),
                   "fused_stream_us_per_call": [round(x, 2) for x in us_f],
                   "composed_f32_stream_us_per_call": [round(x, 2) for x in us_c],
                   "fused_stream_us_median": round(float(np.median(us_f)), 2),
                   "composed_f32_stream_us_median": round(float(np.median(us_c)), 2),
                   "speedup_stream_median": round(float(np.median(us_c) / np.median(us_f)), 2),
                   "loss_fused": lf, "loss_composed_f32": lc,
                   "grad_normalised_max_diff_vs_composed_f32": float((g_f - g_c).abs().max() / g_c.abs().max())}
        print(f"[mesh_lap] {name}: {r[name]['fused_stream_us_median']} us fused, {r[name]['composed_f32_stream_us_median']} us composed",
              file=sys.stderr, flush=True)
    if not a.no_window:
        import bench_window
        w = {}
        for rep in range(2):                    # alternated, twice: the spread is in the lists
            for fused_step in (False, True):
                for lap in (False, True):
                    res = bench_window.run(argparse.Namespace(frames=2, iters=50, level=6, width=1920, height=1080, cameras=160,
                                                              fused_step=fused_step, mesh_reg=True, mesh_lap=lap))
                    key = ("fused_step" if fused_step else "autograd") + ("_mesh_reg_mesh_lap" if lap else "_mesh_reg")
                    w.setdefault(key, {"median_ms_per_iteration": [], "loss_last": []})
                    w[key]["median_ms_per_iteration"].append(res["median_ms_per_iteration"])
                    w[key]["loss_last"].append([fr["loss_last"] for fr in res["frames"]])
                    print(f"[mesh_lap] window {key}: {res['median_ms_per_iteration']} ms", file=sys.stderr, flush=True)
        r["window"] = w
        med = lambda key: float(np.median(w[key]["median_ms_per_iteration"]))
        r["window_ratio_autograd"] = round(med("autograd_mesh_reg_mesh_lap") / med("autograd_mesh_reg"), 3)
        r["window_ratio_fused_step"] = round(med("fused_step_mesh_reg_mesh_lap") / med("fused_step_mesh_reg"), 3)
    line = json.dumps(r)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# tools/bench_mesh_lap.py on one MI355X (us = microseconds per forward + backward call)\n")
            for key, val in r.items():
                fh.write(f"{key}: {json.dumps(val)}\n")


if __name__ == "__main__":
    main()
