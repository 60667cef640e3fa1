"""The five colour hand-over kernels (gsr_handover.hip) at config C's mesh sizes, the ones tools/bench_splice.py uses: base mesh a
level-6 icosphere (81 920 faces, 6 Gaussians each), fused surface a level-7 icosphere a little outside it, rotated, two regions
around the poles.

    python tools/bench_handover.py --out profiles/handover_config_c.txt

The GPU work runs in a child process under a time limit; if it fails, faults or runs out of time the run ends there.  Each
kernel is timed through its C entry point on buffers made beforehand, with device events around --inner back-to-back calls and
no host read between them; medians and the spread of --reps repeats, and the bytes each call has to move over that time.  Then
TopologyUpdate.with_colors as a whole (two host reads of an err word) and update_mesh_topology, which now also records
face_origin.  The results are checked against the numpy restatement tests/handover_ref.py."""
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

STEP_LIMIT_S = 420
G = 6


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
    import numpy as np
    import torch
    import handover_ref as ref
    from bench_splice import inputs
    from gaustar_amd import _host, _lib, handover, harness, regions
    assert torch.cuda.is_available(), "bench_handover needs a GPU"
    dev = torch.device("cuda:0")
    lib, p, st = _lib.load(), _lib.ptr, _host.raw_stream(dev.index)
    bv, bf, fv, ff, raw = inputs()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    rng = np.random.default_rng(0)
    F, V, Ff, Vf = len(bf), len(bv), len(ff), len(fv)
    dc = rng.normal(0, 1.2, size=(F * G, 3)).astype(np.float32)
    fcol = rng.random((Vf, 3)).astype(np.float32)
    bcol = rng.random((V, 3)).astype(np.float32)
    tbf, tff, tdc, tfcol, tbcol = t(bf), t(ff), t(dc), t(fcol), t(bcol)
    bary = torch.tensor(harness.BARY_COORDS[G], dtype=torch.float32, device=dev)
    none = torch.empty(0, dtype=torch.int32, device=dev)
    sel = regions.UpdateRegions(component=none, region=none, n_components=2, n_regions=2, labels=np.arange(2, dtype=np.int32),
                                counts=np.full(2, 100, np.int32), raw_boxes=raw.copy())

    class Mesh:
        verts, faces = t(fv), tff

    tv = t(bv)
    upd = regions.update_mesh_topology(tv, tbf, sel, Mesh)
    Nf, Nv = int(upd.faces.shape[0]), int(upd.verts.shape[0])
    err = torch.zeros(1, dtype=torch.int32, device=dev)
    rgba = torch.empty(F, 4, dtype=torch.uint8, device=dev)
    frgba = torch.empty(Ff, 4, dtype=torch.uint8, device=dev)
    urgba = torch.empty(Nf, 4, dtype=torch.uint8, device=dev)
    vrgba = torch.empty(Nv, 4, dtype=torch.uint8, device=dev)
    sums = torch.empty(Nv, 4, dtype=torch.int32, device=dev)
    sh = torch.empty(F * G, 3, dtype=torch.float32, device=dev)
    calls = {
        # name: (call, bytes a call has to move at the least)
        "face_colors": (lambda: lib.gsr_handover_face_colors(F, G, p(tdc), p(rgba), st), 12 * F * G + 4 * F),
        "vertex_to_face": (lambda: lib.gsr_handover_vertex_to_face(Ff, Vf, p(tff), p(tfcol), 3, p(frgba), p(err), st), 12 * Ff + 12 * Vf + 4 * Ff),
        "face_to_vertex": (lambda: lib.gsr_handover_face_to_vertex(Nf, Nv, p(upd.faces), p(urgba), p(sums), p(vrgba), p(err), st),
                           16 * Nf + 2 * 16 * Nv + 4 * Nv),
        "sh_dc": (lambda: lib.gsr_handover_sh_dc(F, G, V, p(tbf), p(tbcol), 3, p(bary), p(sh), p(err), st), 12 * F + 12 * V + 12 * F * G),
        "gather": (lambda: lib.gsr_handover_gather(Nf, p(upd.face_origin), F, p(rgba), Ff, Vf, p(tff), p(tfcol), 3, p(urgba), p(err), st),
                   4 * Nf + 4 * Nf + 4 * Nf),
    }
    out = dict(F=F, V=V, Ff=Ff, Vf=Vf, Nf=Nf, Nv=Nv, kernels={})
    for name in ("face_colors", "vertex_to_face", "gather", "face_to_vertex", "sh_dc"):      # (gather fills what face_to_vertex reads)
        fn, nbytes = calls[name]
        assert fn() == 0, name
        ms, lo, hi = timed(fn, reps, inner)
        out["kernels"][name] = dict(ms=ms, lo=lo, hi=hi, bytes=nbytes)
    assert int(err.cpu()) == 0
    ms, lo, hi = timed(lambda: upd.with_colors(rgba, tfcol), reps)
    out["with_colors"] = dict(ms=ms, lo=lo, hi=hi)
    ms, lo, hi = timed(lambda: regions.update_mesh_topology(tv, tbf, sel, Mesh), reps)
    out["update"] = dict(ms=ms, lo=lo, hi=hi)
    n = lambda x: x.cpu().numpy()
    same = {"face_colors": np.array_equal(n(rgba), ref.sh_face_colors(dc, G)),
            "vertex_to_face": np.array_equal(n(frgba), ref.vertex_to_face_colors(ff, fcol)),
            "sh_dc": n(sh).tobytes() == ref.sh_dc_from_vertex_colors(bf, bcol, G).tobytes()}
    want_fc = ref.gather_face_colors(n(upd.face_origin), n(rgba), ff, fcol)
    same["gather"] = np.array_equal(n(upd.face_colors), want_fc) and np.array_equal(n(urgba), want_fc)
    same["face_to_vertex"] = np.array_equal(n(upd.vertex_colors), ref.face_to_vertex_colors(n(upd.faces), want_fc, Nv))
    out["same"] = {k: bool(v) for k, v in same.items()}
    out["filled"] = int((upd.face_origin == handover.FILLED).sum())
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
        sys.exit(f"bench_handover: the GPU step ran past {STEP_LIMIT_S} s")
    if r.returncode != 0:
        sys.exit(f"bench_handover: the GPU step ended with status {r.returncode}\n{r.stderr[-2000:]}")
    res = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    what = {"face_colors": f"face colours from the SH dc ({res['F']} faces x {G} Gaussians)",
            "vertex_to_face": f"vertex -> face colours (the fused surface: {res['Ff']} faces / {res['Vf']} vertices)",
            "gather": f"face-origin gather (the updated mesh: {res['Nf']} faces)",
            "face_to_vertex": f"face -> vertex colours (the updated mesh: {res['Nf']} faces / {res['Nv']} vertices; clear + scatter + mean)",
            "sh_dc": f"SH dc from vertex colours ({res['F']} faces x {G} Gaussians / {res['V']} vertices)"}
    lines = [f"# tools/bench_handover.py at config C's mesh sizes (tools/bench_splice.py's inputs): base mesh {res['F']} faces, fused surface "
             f"{res['Ff']} faces, two regions around the poles; per call, median of {args.reps} x {args.inner} back-to-back calls, no host read"]
    for name, k in res["kernels"].items():
        lines.append(f"{what[name]}: {1e3 * k['ms']:.1f} us (min {1e3 * k['lo']:.1f}, max {1e3 * k['hi']:.1f}); {k['bytes'] / 1e6:.2f} MB at the "
                     f"least, {k['bytes'] / k['ms'] / 1e9:.3f} TB/s")
    w, u = res["with_colors"], res["update"]
    lines += [f"TopologyUpdate.with_colors (gather, then face -> vertex; two host reads of an err word), median of {args.reps}: {w['ms']:.3f} ms "
              f"(min {w['lo']:.3f}, max {w['hi']:.3f})",
              f"update_mesh_topology with face_origin, both boxes, median of {args.reps}: {u['ms']:.3f} ms (min {u['lo']:.3f}, max {u['hi']:.3f}); "
              f"{res['filled']} filled faces in the result",
              "results equal to the restatement: " + ", ".join(f"{k} {v}" for k, v in res["same"].items())]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert all(res["same"].values()), "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
