"""The editing kernels (gsr_edit.hip) at config C: the level-6 icosphere's 81 920 faces and 40 962 vertices, 491 520 Gaussians,
sh_levels 4, loose-bound.

    python tools/bench_edit.py --out profiles/edit_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  Every op
is timed through its C entry point on buffers made beforehand, with device events around --inner back-to-back calls and no host
read between them (medians and the spread of --reps repeats), and beside it the torch composition of the same rule on the same
GPU, timed the same way.  rotate_sh also stands beside a plain torch copy of the bytes it has to move.  The ops: the rigid
fit's sums for 303 anchors over 180 frames (merge_gstar's anchor file and frame range), the vertices' transform, the SH
rotation, cut_gstar's four groups of planes, the gather of a cut that keeps half the faces, and the two-triangle decal.  The
first 4 096 Gaussians of the rotated SH are checked against the numpy restatement tests/edit_ref.py."""
from __future__ import annotations

import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_LIMIT_S = 420
FIT_K, FIT_T = 303, 180


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
    import ctypes
    import numpy as np
    import torch
    import edit_ref as ref
    from gaustar_amd import _host, _lib, edit, scene
    assert torch.cuda.is_available(), "bench_edit needs a GPU"
    dev = torch.device("cuda:0")
    lib, p, st = _lib.load(), _lib.ptr, _host.raw_stream(dev.index)
    dptr = lambda a: a.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rng = np.random.default_rng(0)
    out = {}

    def ok(rc):
        assert rc == 0, lib.gsr_last_error()

    v, f = scene.icosphere(6, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    V, F, G, L = len(v), len(f), 6, 4
    N, M = F * G, L * L
    verts, faces = torch.from_numpy(v).to(dev), torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev)
    gen = torch.Generator(device=dev).manual_seed(0)
    rnd = lambda *s: torch.randn(*s, generator=gen, device=dev)
    params = [rnd(N, 2), rnd(N, 2), rnd(N, 1), rnd(N, 1, 3), rnd(N, M - 1, 3), rnd(N, 3), rnd(N, 4)]
    out["sizes"] = dict(V=V, F=F, N=N, M=M)
    R, t = ref.rotation(rng), rng.normal(size=3)
    Rt, tt = torch.from_numpy(R).to(dev), torch.from_numpy(t).to(dev)
    err = torch.zeros(1, dtype=torch.int32, device=dev)

    # 1. the rigid fit's sums
    src = rng.normal(size=(FIT_K, 3))
    dst = np.stack([src @ ref.rotation(rng).T + rng.normal(size=3) for _ in range(FIT_T)])
    a, b = torch.from_numpy(src).to(dev), torch.from_numpy(dst).to(dev)
    ws = torch.empty(int(lib.gsr_edit_fit_workspace_bytes(FIT_T, FIT_K)), dtype=torch.uint8, device=dev)
    sums = torch.empty(FIT_T, 16, dtype=torch.float64, device=dev)

    def fit_torch():
        okk = torch.isfinite(a).all(-1)[None] & torch.isfinite(b).all(-1)
        n = okk.sum(1, keepdim=True)
        abar = torch.where(okk[..., None], a[None], 0.0).sum(1) / n
        bbar = torch.where(okk[..., None], b, 0.0).sum(1) / n
        da = torch.where(okk[..., None], a[None] - abar[:, None], 0.0)
        return torch.einsum("tki,tkj->tij", da, b - bbar[:, None])
    out["fit_sums"] = dict(kernel=timed(lambda: ok(lib.gsr_edit_fit_sums(FIT_T, FIT_K, p(a), p(b), p(ws), p(sums), None, st)), reps, inner),
                           torch=timed(fit_torch, reps, inner))

    # 2. the vertices
    x = verts.clone()
    out["transform_points"] = dict(kernel=timed(lambda: ok(lib.gsr_edit_transform_points(V, 3, 0, p(x), dptr(R), dptr(t), None, st)), reps, inner),
                                   torch=timed(lambda: (verts.double() @ Rt.T + tt).float(), reps, inner))

    # 3. the SH rotation, beside a copy of the same bytes
    rest = params[4]
    D = torch.from_numpy(edit.sh_rotation_matrices(R, L)).to(dev)
    turned = torch.empty_like(rest)
    Dr = D[1:, 1:].contiguous()
    out["rotate_sh"] = dict(kernel=timed(lambda: ok(lib.gsr_edit_rotate_sh(N, M, p(D), p(rest), p(turned), None, st)), reps, inner),
                            torch=timed(lambda: torch.einsum("ik,nkc->nic", Dr, rest.double()).float(), reps, inner),
                            copy=timed(lambda: turned.copy_(rest), reps, inner), bytes=2 * rest.numel() * 4)
    ok(lib.gsr_edit_rotate_sh(N, M, p(D), p(rest), p(turned), None, st))
    out["same"] = bool(np.array_equal(turned[:4096].cpu().numpy(), ref.rotate_sh(rest[:4096].cpu().numpy(), D.cpu().numpy())))

    # 4. cut_gstar's planes (:84-100) as four groups
    groups = [np.array([[1.0, 0, -1.2, 0.37], [-1.0, 0, -0.8, 0.6], [1.0, 0, 0.8, -0.05], [0, -1.0, 0, 0.35]]),
              np.array([[1.0, 0, -1.2, 0.37], [0, -1.0, 0, 0.3]]), np.array([[-1.0, 0, 1.2, -0.37], [-1.0, 0, 0, 0.3]]),
              np.array([[-1.0, 0, 0, 0.3], [0, 1.0, 0, -0.95]])]
    sizes = (ctypes.c_int * len(groups))(*[len(g) for g in groups])
    planes = np.ascontiguousarray(np.concatenate(groups))
    mask = torch.empty(F, dtype=torch.uint8, device=dev)
    gt = [torch.from_numpy(g).to(dev) for g in groups]

    def halfspaces_torch():
        c = verts.double()[faces.long()]
        c = ((c[:, 0] + c[:, 1]) + c[:, 2]) / 3.0
        sel = torch.zeros(F, dtype=torch.bool, device=dev)
        for g in gt:
            sel |= ((c @ g[:, :3].T + g[:, 3]) > 0).all(-1)
        return sel
    out["faces_in_halfspaces"] = dict(
        kernel=timed(lambda: ok(lib.gsr_edit_faces_in_halfspaces(F, V, p(faces), p(verts), len(groups), sizes, dptr(planes), p(mask), p(err), st)),
                     reps, inner),
        torch=timed(halfspaces_torch, reps, inner))
    out["selected"] = int(mask.sum())

    # 5. the gather of a cut that keeps every other face
    kept = torch.arange(0, F, 2, dtype=torch.int32, device=dev)
    nk = int(kept.shape[0])
    dsts = [torch.empty((nk * G, *s.shape[1:]), device=dev) for s in params]
    k = len(params)
    sp, dp_ = (ctypes.c_void_p * k)(*[s.data_ptr() for s in params]), (ctypes.c_void_p * k)(*[d.data_ptr() for d in dsts])
    words = (ctypes.c_int * k)(*[s[0].numel() for s in params])
    rows = (kept.long()[:, None] * G + torch.arange(G, device=dev)).reshape(-1)
    out["gather_rows"] = dict(kernel=timed(lambda: ok(lib.gsr_edit_gather_rows(nk, F, p(kept), G, k, sp, dp_, words, p(err), st)), reps, inner),
                              torch=timed(lambda: [s[rows] for s in params], reps, inner),
                              bytes=2 * sum(d.numel() for d in dsts) * 4)

    # 6. the decal: a quad of half-width 0.45 R at 0.93 R above the centre, two triangles
    (cx, cy, cz), rad = scene.SUBJECT_CENTER, scene.SUBJECT_RADIUS
    hw, z = 0.45 * rad, cz + 0.93 * rad
    anchors = np.array([[cx - hw, cy - hw, z], [cx - hw, cy + hw, z], [cx + hw, cy - hw, z], [cx + hw, cy + hw, z]])
    uv = np.array([[0.1, 0.1], [0.1, 0.9], [0.9, 0.1], [0.9, 0.9]])
    tris = np.array([[0, 1, 2], [1, 2, 3]])
    table = torch.from_numpy(np.concatenate([anchors[tris].reshape(2, 9), uv[tris].reshape(2, 6)], 1)).to(dev)
    tex = torch.randint(0, 256, (512, 512, 1), dtype=torch.uint8, device=dev)
    bary = torch.tensor(ref.BARY[6], dtype=torch.float32, device=dev)
    scales, dc = params[0].clone(), params[3].clone()
    stats = torch.zeros(4, dtype=torch.int32, device=dev)
    at, ut, c0 = torch.from_numpy(anchors).to(dev), torch.from_numpy(uv).to(dev), 0.28209479177387814

    def paint_torch():
        fv = verts.double()[faces.long()]
        b = bary.double()
        pts = ((b[None, :, 0, None] * fv[:, None, 0] + b[None, :, 1, None] * fv[:, None, 1]) + b[None, :, 2, None] * fv[:, None, 2]).reshape(-1, 3)
        rgb = dc.view(-1, 3) * c0 + 0.5
        sc = scales.clone()
        for tri in tris.tolist():
            t0, t1, t2 = at[tri[0]], at[tri[1]], at[tri[2]]
            e0, e1, w = t1 - t0, t2 - t0, pts - t0
            d00, d01, d11, d02, d12 = e0 @ e0, e0 @ e1, e1 @ e1, w @ e0, w @ e1
            inv = 1.0 / (d00 * d11 - d01 * d01)
            b2, b1 = (d00 * d12 - d01 * d02) * inv, (d11 * d02 - d01 * d12) * inv
            nb = torch.stack([(1.0 - b1) - b2, b1, b2], -1)
            nrm = -torch.linalg.cross(t1 - t0, t2 - t1)
            dist = (t0 - pts) @ (nrm / nrm.norm())
            inside = (nb >= -0.03).all(-1) & (dist.abs() < 0.09)
            uvp = nb @ ut[tri]
            row, col = (uvp[:, 0] * 512).long().clamp(0, 511), (uvp[:, 1] * 512).long().clamp(0, 511)
            k_ = (tex[row, col, 0].double() / 255.0).float()
            rgb = torch.where(inside[:, None], rgb * k_[:, None], rgb)
            sc = torch.where(inside[:, None], torch.full_like(sc, -6.0), sc)
        return (rgb - 0.5) / c0, sc
    out["paint"] = dict(
        kernel=timed(lambda: ok(lib.gsr_edit_paint(N, G, F, V, p(faces), p(verts), p(bary), 2, p(table), 512, 512, 1, p(tex), 0, 0.03, 0.09, 1, -6.0,
                                                   50, p(scales), p(dc), p(stats), p(err), st)), reps, inner),
        torch=timed(paint_torch, reps, inner))
    out["painted"] = stats.cpu().tolist()
    assert int(err.cpu()) == 0
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
        sys.exit(f"bench_edit: the GPU step ran past {STEP_LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_edit: the GPU step ended with status {r.returncode}\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    s = res["sizes"]
    us = lambda k: f"{1e3 * k[0]:.1f} us (min {1e3 * k[1]:.1f}, max {1e3 * k[2]:.1f})"
    lines = [f"# tools/bench_edit.py: GPU time between device events, median of {args.reps} x {args.inner} back-to-back calls (min, max), no host "
             f"read; config C: {s['F']} faces, {s['V']} vertices, {s['N']} Gaussians, sh_levels 4"]
    what = {"fit_sums": f"gsr_edit_fit_sums, {FIT_K} anchors x {FIT_T} frames (three launches)",
            "transform_points": f"gsr_edit_transform_points, {s['V']} vertices",
            "rotate_sh": f"gsr_edit_rotate_sh, [{s['N']},{s['M'] - 1},3] f32",
            "faces_in_halfspaces": f"gsr_edit_faces_in_halfspaces, 4 groups, 10 planes ({res['selected']} faces selected)",
            "gather_rows": "gsr_edit_gather_rows, 7 arrays, every other face kept",
            "paint": f"gsr_edit_paint, 2 triangles, 512 x 512 texture, multiply ({res['painted'][2]} + {res['painted'][3]} inside, "
                     f"{res['painted'][0]} painted)"}
    for key, label in what.items():
        row = res[key]
        line = f"{label}: {us(row['kernel'])}; torch composition of the rule: {us(row['torch'])}"
        if "bytes" in row:
            line += f"; {row['bytes'] / 1e6:.1f} MB read + written, {row['bytes'] / row['kernel'][0] / 1e9:.2f} TB/s"
        if "copy" in row:
            line += (f"; torch copy of the same bytes: {us(row['copy'])}, {row['bytes'] / row['copy'][0] / 1e9:.2f} TB/s: the kernel reaches "
                     f"{100 * row['copy'][0] / row['kernel'][0]:.0f} % of the copy's bandwidth")
        lines.append(line)
    lines.append(f"rotate_sh's first 4096 Gaussians equal to the restatement bit for bit: {res['same']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert res["same"], "the kernel and the restatement disagree"


if __name__ == "__main__":
    main()
