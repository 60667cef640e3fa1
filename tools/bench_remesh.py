"""Quadric decimation and smoothing at config C's size (fused surface: a level-7 icosphere = 327 680 faces, as tools/bench_splice.py
takes it; base mesh: 81 920 faces): gaustar_amd.remesh.simplify_mesh to the base mesh's face count and to half of it, the
rounds' breakdown, and 10 Laplacian sweeps.

    python tools/bench_remesh.py --out profiles/remesh_config_c.txt

Every GPU step runs in a child process of its own under a time limit; a step that fails, faults or runs out of time ends the
run there and nothing more is started.  Timed with device events around the calls (host reads included where the call has
them), after a warm-up; medians and the spread of --reps repeats.  The breakdown brackets every C entry point of one run with
events of its own; what is left of the round is torch's sorts and scans and the round's host read.  Next to them the wall time
of the numpy restatement (tests/remesh_ref.py) on the host, once, on a level-5 icosphere (20 480 -> 5 120 faces: plain Python
per edge, the full size would take many minutes), with the GPU's result on the same input compared bit for bit.  No time is
asserted."""
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

STEP_LIMIT_S = {"simplify": 420, "smooth": 120, "host": 420}
BASE_FACES = 81920


def fused_surface(level: int = 7):
    import numpy as np
    from gaustar_amd import scene
    v, f = scene.icosphere(level, float(scene.SUBJECT_RADIUS) * 1.004, scene.SUBJECT_CENTER)
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


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


class _Bracketed:
    """The library with every gsr_remesh_* call between two events."""

    def __init__(self, lib, log):
        self._lib, self._log = lib, log

    def __getattr__(self, name):
        import torch
        fn = getattr(self._lib, name)
        if not name.startswith("gsr_remesh_") or name == "gsr_remesh_cap":
            return fn

        def call(*args):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            rc = fn(*args)
            b.record()
            self._log.append((name, a, b))
            return rc
        return call


def breakdown(tv, tf, target):
    """One run of simplify_mesh's loop with every entry point bracketed -> (per entry point ms, total ms, rounds)."""
    import ctypes
    import torch
    from gaustar_amd import remesh
    log = []
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rd = remesh._Round(tv, tf, None, ())
    rd.lib = _Bracketed(rd.lib, log)
    n_live, rounds, n_apply = int(tf.shape[0]), [], ctypes.c_int(0)
    while n_live > target:
        state, ranked, n_sel = rd.select(n_live)
        rd.lib.gsr_remesh_cap(n_live, target, n_sel, ctypes.byref(n_apply))
        if n_apply.value == 0:
            break
        rd.apply(state, ranked, n_apply.value)
        rounds.append((n_live, n_sel, n_apply.value))
        n_live -= 2 * n_apply.value
    b.record()
    b.synchronize()
    per = {}
    for name, x, y in log:
        per[name] = per.get(name, 0.0) + x.elapsed_time(y)
    return per, a.elapsed_time(b), rounds


def step(name: str, reps: int) -> dict:
    """One GPU step, in this (child) process."""
    import numpy as np
    import torch
    from gaustar_amd import regions, remesh
    assert torch.cuda.is_available(), "bench_remesh needs a GPU"
    dev = torch.device("cuda:0")
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    if name == "host":
        import remesh_ref as ref
        v, f = fused_surface(5)
        target = len(f) // 4
        got, ms, lo, hi = timed(lambda: remesh.simplify_mesh(t(v), t(f), target), 3)
        t0 = time.perf_counter()
        want = ref.simplify(v, f, target)
        host = time.perf_counter() - t0
        same = bool(np.array_equal(got.faces.cpu().numpy(), want.faces) and got.verts.cpu().numpy().tobytes() == want.verts.tobytes()
                    and got.n_rounds == want.n_rounds)
        return dict(F=len(f), target=target, out=int(got.faces.shape[0]), rounds=got.n_rounds, ms=ms, host_ms=1e3 * host, same=same)
    v, f = fused_surface(7)
    tv, tf = t(v), t(f)
    if name == "smooth":
        _o, ms, lo, hi = timed(lambda: remesh.smooth_laplacian(tv, tf, iterations=10), reps)      # (the neighbour lists are cached on tf)
        return dict(F=len(f), V=len(v), ms=ms, lo=lo, hi=hi)
    res = dict(F=len(f), V=len(v), runs=[])
    for target in (BASE_FACES, BASE_FACES // 2):
        got, ms, lo, hi = timed(lambda: remesh.simplify_mesh(tv, tf, target), reps)
        per, total, rounds = breakdown(tv, tf, target)
        res["runs"].append(dict(target=target, out=int(got.faces.shape[0]), verts=int(got.verts.shape[0]), rounds=got.n_rounds,
                                stalled=got.stalled, watertight=regions.is_watertight(got.faces), ms=ms, lo=lo, hi=hi, per=per,
                                loop_ms=total, first=rounds[:3], last=rounds[-2:]))
    return res


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
    for name in ("simplify", "smooth", "host"):       # a child per step; the first that fails ends the run
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", name, "--reps", str(args.reps)],
                               capture_output=True, text=True, timeout=STEP_LIMIT_S[name])
        except subprocess.TimeoutExpired:
            sys.exit(f"bench_remesh: step {name} ran past {STEP_LIMIT_S[name]} s; nothing more is started")
        if r.returncode != 0:
            sys.exit(f"bench_remesh: step {name} ended with status {r.returncode}; nothing more is started\n{r.stderr[-2000:]}")
        res[name] = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
    s, m, h = res["simplify"], res["smooth"], res["host"]
    lines = [f"# tools/bench_remesh.py at config C's size: fused surface {s['F']} faces / {s['V']} vertices (a level-7 icosphere)"]
    for r in s["runs"]:
        kernels = sum(r["per"].values())
        lines.append(f"simplify_mesh to {r['target']} faces, median of {args.reps}: {r['ms']:.3f} ms (min {r['lo']:.3f}, max {r['hi']:.3f}), "
                     f"host reads and the final compaction included; result {r['out']} faces / {r['verts']} vertices in {r['rounds']} "
                     f"rounds, stalled {r['stalled']}, watertight {r['watertight']}")
        lines.append(f"  one bracketed run, setup and rounds {r['loop_ms']:.3f} ms: the rounds' entry points {kernels:.3f} ms; the setup, torch's sorts "
                     f"and scans and the rounds' host reads {r['loop_ms'] - kernels:.3f} ms; (live faces, selected, applied) of the first rounds "
                     f"{r['first']}, of the last {r['last']}")
        lines += [f"    {k[len('gsr_remesh_'):]:<16} {v:9.3f} ms" for k, v in sorted(r["per"].items(), key=lambda kv: -kv[1])]
    lines.append(f"smooth_laplacian, 10 sweeps, {m['V']} vertices, median of {args.reps}: {m['ms']:.3f} ms (min {m['lo']:.3f}, max {m['hi']:.3f})")
    lines.append(f"numpy restatement on the host, once, level-5 icosphere {h['F']} -> {h['target']} faces: {h['host_ms']:.0f} ms in {h['rounds']} "
                 f"rounds; simplify_mesh on the same input {h['ms']:.3f} ms; results equal bit for bit: {h['same']}")
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert h["same"], "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
