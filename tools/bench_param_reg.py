"""tools/bench_param_reg.py [--iters N] [--out FILE] [--no-window] -- the regularisers on the Gaussians' own parameters
(refine.py:739-740, :743-748, :663-669) at config-C size (N = 491 520 Gaussians, M = N) on one GPU:

  fused     losses.gaussian_param_loss forward + backward (gsr_param_reg_forward: element pass + finalise,
            gsr_param_reg_backward: one elementwise launch): GPU time of the `loss_kernels` profiler stage (device events around
            each launch group) and stream-event time per call;
  composed  the reference's four torch lines on the same tensors + autograd's backward: stream-event time.  The yardstick, not
            code under test.
  window    tools/bench_window.py's loop at config-C size, loose-bound: --fused-step with and without param_reg, and the
            autograd route with the torch composition.

The two routes are timed in interleaved regions; medians are reported.  Kernel times by name come from a run of its own:
    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -o preg -- python tools/bench_param_reg.py --fused-only
    python tools/bench_param_reg.py --kernel-stats DIR --out FILE        (appends to FILE)
Prints one JSON line; --out also writes it, one key per line, to a text file (profiles/param_reg_config_c.txt)."""
import argparse, csv, ctypes, glob, json, os, sys
import numpy as np
import torch
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE)); sys.path.insert(0, HERE)
from gaustar_amd import _lib, losses

FACTORS = dict(factor_t=100.0, factor_r=1.0, min_opacity=0.8, sh_factor=1.0)   # refine.py:29-33
N = 491_520


def composed_loss(dt, dr, w, dens, sh, pre, factor_t, factor_r, min_opacity, sh_factor):
    loss = factor_t * (w * dt.abs()).mean()
    loss = loss + factor_r * (w * dr[..., 1:].abs()).mean()
    loss = loss + torch.relu(min_opacity - torch.sigmoid(dens.view(-1, 1))).mean()
    return loss + sh_factor * ((pre - sh[:, 0, :]) ** 2).mean()


def region(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record(); torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3


def kernel_stats(a):
    files = glob.glob(os.path.join(a.kernel_stats, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {a.kernel_stats}")
    rows = []
    with open(files[0]) as fh:
        for r in csv.DictReader(fh):
            if "param_reg_" in r["Name"]:
                rows.append((r["Name"].split("(")[0].replace("gsr::", "").replace("(anonymous namespace)::", ""), int(r["Calls"]),
                             float(r["TotalDurationNs"]) / int(r["Calls"]) / 1e3))
    lines = ["", "# rocprofv3 --kernel-trace --stats of tools/bench_param_reg.py --fused-only: kernel, calls, mean us",
             *[f"  {n:<32} {c:>6} {us:>8.2f}" for n, c, us in sorted(rows)],
             f"fused_gpu_us_kernel_trace_sum: {sum(us for _, _, us in rows):.2f}"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if a.out:
        with open(a.out, "a") as fh:
            fh.write(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--no-window", action="store_true")
    ap.add_argument("--fused-only", action="store_true")
    ap.add_argument("--kernel-stats", default=None, metavar="DIR")
    a = ap.parse_args()
    if a.kernel_stats:
        return kernel_stats(a)
    dev = torch.device("cuda:0")
    lib = _lib.load()
    g = torch.Generator(device=dev).manual_seed(0)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    dt = (0.01 * r(N, 3)).requires_grad_(True)
    dr = torch.nn.functional.normalize(torch.tensor([1.0, 0.0, 0.0, 0.0], device=dev) + 0.05 * r(N, 4), dim=-1).requires_grad_(True)
    dens = (1.5 * r(N, 1) + 1.4).requires_grad_(True)
    sh = r(N, 1, 3).requires_grad_(True)
    pre = sh.detach()[:, 0].clone() + 0.1 * r(N, 3)
    w = (torch.rand(N // 6, device=dev, generator=g) > 0.3).float().repeat_interleave(6)[:, None].expand(-1, 3)   # refine.py:737
    leaves = (dt, dr, dens, sh)
    one = torch.ones((), device=dev)

    def fused():
        for p in leaves:
            p.grad = None
        losses.gaussian_param_loss(dt, dr, w, densities=dens, sh_dc=sh, pre_sh_dc=pre, **FACTORS).backward(one)

    def composed():
        for p in leaves:
            p.grad = None
        composed_loss(dt, dr, w, dens, sh, pre, **FACTORS).backward(one)

    for _ in range(20):
        fused()
        if not a.fused_only:
            composed()
    torch.cuda.synchronize()
    if a.fused_only:
        for _ in range(a.iters):
            fused()
        torch.cuda.synchronize()
        return
    fused(); g_f = [p.grad.clone() for p in leaves]
    composed(); g_c = [p.grad.clone() for p in leaves]
    lf = float(losses.gaussian_param_loss(dt.detach(), dr.detach(), w, densities=dens.detach(), sh_dc=sh.detach(), pre_sh_dc=pre, **FACTORS))
    lc = float(composed_loss(dt.detach(), dr.detach(), w, dens.detach(), sh.detach(), pre, **FACTORS))
    us_fused, us_comp = [], []
    for _ in range(5):                         # interleaved regions
        us_fused.append(region(fused, a.iters)); us_comp.append(region(composed, a.iters))
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
    fwd_b = 4 * N * (3 + 4 + 1 + 3 + 3 + 1)                 # delta_t, delta_r, densities, sh_dc, pre_sh_dc, one weight per Gaussian
    bwd_b = fwd_b + 4 * N * (3 + 4 + 1 + 3)
    r_ = {"what": "regularisers on the Gaussians' parameters (loose-bind t / r, opacity floor, SH dc) forward + backward, config C",
          "N": N, "M": N, "factors": FACTORS, "iters": a.iters,
          "fused_gpu_us_loss_kernels_stage": round(ms[k] / a.iters * 1e3, 2), "fused_launches_per_call": cnt[k] / a.iters,
          "fused_stream_us_per_call": [round(x, 2) for x in us_fused], "composed_stream_us_per_call": [round(x, 2) for x in us_comp],
          "fused_stream_us_median": round(float(np.median(us_fused)), 2), "composed_stream_us_median": round(float(np.median(us_comp)), 2),
          "speedup_stream_median": round(float(np.median(us_comp) / np.median(us_fused)), 2),
          "roofline_estimate_us": "10-15 (both directions, ~50 MB at several TB/s)",
          "loss_fused": lf, "loss_composed": lc,
          "grad_normalised_max_diff": max(float((x - y).abs().max() / y.abs().max()) for x, y in zip(g_f, g_c)),
          "bytes_fwd_pass": fwd_b, "bytes_bwd_pass": bwd_b, "workspace_bytes": int(lib.gsr_param_reg_workspace_bytes(N))}
    if not a.no_window:
        import bench_window
        ns = lambda **kw: argparse.Namespace(frames=2, iters=50, level=6, width=1920, height=1080, cameras=160, **kw)
        res = {"fused_step_loose_param_reg": bench_window.run(ns(fused_step=True, loose_bind=True)),
               "autograd_loose_torch_composition": bench_window.run(ns(fused_step=False, loose_bind=True)),
               "fused_step_loose_no_reg": bench_window.run(ns(fused_step=True, loose_bind=True, no_param_reg=True))}
        r_["window"] = {k_: {"median_ms_per_iteration": v["median_ms_per_iteration"], "ms_per_iteration": v["ms_per_iteration"],
                             "loss_last": [fr["loss_last"] for fr in v["frames"]]} for k_, v in res.items()}
        med = lambda k_: res[k_]["median_ms_per_iteration"]
        r_["window_ratio_fused_vs_torch_composition"] = round(med("fused_step_loose_param_reg") / med("autograd_loose_torch_composition"), 3)
        r_["window_ratio_param_reg_vs_none"] = round(med("fused_step_loose_param_reg") / med("fused_step_loose_no_reg"), 3)
    line = json.dumps(r_)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("# tools/bench_param_reg.py on one MI355X (us = microseconds per forward + backward call)\n")
            for key, val in r_.items():
                fh.write(f"{key}: {json.dumps(val)}\n")


if __name__ == "__main__":
    main()
