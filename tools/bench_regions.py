"""The re-mesh regions and their cuts at config C (level-6 icosphere = 81 920 faces, G = 6; the fused surface of the bench's
scene: 60 sampled + 160 rig cameras at 1080p): gaustar_amd.regions.

    python tools/bench_regions.py --out profiles/regions_config_c.txt
    python tools/bench_regions.py --fusion-level 7           # a level-7 icosphere stands in for the fused surface (no renders)

What a frame costs: the selection once (it does not depend on aabb_pad), then boxes + cuts for each of the reference's six
passes (five aabb_pad trials and the best one again, refined_mesh.py:1064-1100).  Timed with device events around calls that
end in their own host reads, after a warm-up of every shape; medians and the spread of --reps repeats.  Next to them, the
numpy restatement (tests/regions_ref.py) on the same inputs on the host, once -- it stands in for the reference's
trimesh / scipy path, which is not installed here.  The face colours are painted: three caps of the sphere at colour 255 and
forty specks below the face threshold."""
from __future__ import annotations

import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PADS = (0.01, 0.02, 0.03, 0.04, 0.05, 0.02)       # five trials and the best one again


def painted_colours(verts, faces, centre, radius):
    """[F] uint8: 255 on three caps (half-angles 25, 18 and 12 degrees around +y, -x and a tilted axis), 255 on forty specks of a
    few faces each, 100 elsewhere."""
    import numpy as np
    d = (verts[faces].mean(1) - centre) / radius
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    colour = np.full(len(faces), 100, np.uint8)
    for axis, deg in (((0, 1, 0), 25.0), ((-1, 0, 0), 18.0), ((0.5, -0.5, 0.7), 12.0)):
        a = np.asarray(axis, np.float64)
        colour[d @ (a / np.linalg.norm(a)) > np.cos(np.deg2rad(deg))] = 255
    rng = np.random.default_rng(0)
    for a in rng.normal(size=(40, 3)):
        colour[d @ (a / np.linalg.norm(a)) > np.cos(np.deg2rad(1.2))] = 255
    return colour


def timed(fn, reps):
    """Median, min and max in ms of `reps` calls between device events (each call ends in its own host read)."""
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


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--fusion-level", type=int, default=0, help="an icosphere of this level instead of fuse_mesh's surface")
    args = ap.parse_args()

    import numpy as np
    import torch
    import regions_ref as rr
    import test_gpu_topology as t
    from gaustar_amd import fusion, regions, scene

    assert torch.cuda.is_available(), "bench_regions needs a GPU"
    model = t._model(6)
    dev = model.device
    if args.fusion_level:
        fv, ff = scene.icosphere(args.fusion_level, scene.SUBJECT_RADIUS * 1.004, scene.SUBJECT_CENTER)
        g = torch.Generator().manual_seed(0)
        mesh = fusion.FusionMesh(verts=torch.from_numpy(fv).float().to(dev), faces=torch.from_numpy(ff).int().to(dev),
                                 colors=torch.rand(len(fv), 3, generator=g).to(dev), n_blocks=0, n_views=0)
        source = f"a level-{args.fusion_level} icosphere standing in for the fused surface"
    else:
        mesh = fusion.fuse_mesh(model, t._ring_cams())
        source = f"fuse_mesh over {mesh.n_views} views"
    verts = model._points.detach().float().cpu().numpy()
    faces = model._surface_mesh_faces.cpu().numpy().astype(np.int32)
    colour = painted_colours(verts, faces, np.asarray(scene.SUBJECT_CENTER), scene.SUBJECT_RADIUS)
    res = type("Res", (), {"face_colour": torch.from_numpy(colour).to(dev)})()
    with torch.no_grad():
        model.points
    torch.cuda.synchronize()

    found, sel_ms, sel_lo, sel_hi = timed(lambda: model.topology_update_regions(res), args.reps)

    def six_passes():
        return [model.cut_update_regions(found, mesh, aabb_pad=p) for p in PADS]

    cuts, cut_ms, cut_lo, cut_hi = timed(six_passes, args.reps)
    one, one_ms, one_lo, one_hi = timed(lambda: model.cut_update_regions(found, mesh, aabb_pad=0.02), args.reps)

    # the restatement on the host, on the same inputs, once
    pts = model.points.detach().cpu().numpy()
    fv, ff, fc = mesh.verts.cpu().numpy(), mesh.faces.cpu().numpy(), mesh.colors.cpu().numpy()
    t0 = time.perf_counter()
    want = rr.select_update_regions(verts, faces, pts, colour, 6)
    t1 = time.perf_counter()
    ref_cuts = []
    for p in PADS:
        ref_cuts.append([(rr.cut_mesh_by_box(fv, ff, b, False, attrs=(fc,)), rr.cut_mesh_by_box(verts, faces, b, True))
                         for b in rr.padded_boxes(want["raw_boxes"], p)])
    t2 = time.perf_counter()
    same = np.array_equal(found.region.cpu().numpy(), want["region"]) and found.raw_boxes.tobytes() == want["raw_boxes"].tobytes()
    for got, ref in zip(cuts, ref_cuts):
        same = same and len(got) == len(ref)
        for g, (patch, base) in zip(got, ref):
            same = same and np.array_equal(g.fusion_patch.faces.cpu().numpy(), patch["faces"]) and \
                np.array_equal(g.base_cut.face_mask.cpu().numpy(), base["face_mask"]) and \
                g.fusion_patch.verts.cpu().numpy().tobytes() == patch["verts"].tobytes()

    F, V, Ff, Vf = len(faces), len(verts), len(ff), len(fv)
    n_boxes = [len(c) for c in cuts]
    lines = [f"# tools/bench_regions.py at config C: base mesh {F} faces / {V} vertices, G = 6; fused surface {Ff} faces / {Vf} vertices ({source})",
             f"painted colours: {int((colour >= 153).sum())} faces above the cut-off in {found.n_components} components, "
             f"{found.n_regions} with more than 80 faces ({found.counts.tolist()} faces); merged boxes per pass {n_boxes}",
             f"selection, once per frame, median of {args.reps}: {sel_ms:.3f} ms (min {sel_lo:.3f}, max {sel_hi:.3f})",
             f"boxes + cuts, the six passes of a frame {PADS}, median of {args.reps}: {cut_ms:.3f} ms (min {cut_lo:.3f}, max {cut_hi:.3f})",
             f"boxes + cuts, one pass (aabb_pad 0.02, {n_boxes[1]} boxes: a fused-surface cut and a base-mesh cut each), median of "
             f"{args.reps}: {one_ms:.3f} ms (min {one_lo:.3f}, max {one_hi:.3f})",
             f"a frame (selection + six passes): {sel_ms + cut_ms:.3f} ms",
             f"numpy restatement on the host, once: selection {1e3 * (t1 - t0):.0f} ms, six passes of boxes + cuts {1e3 * (t2 - t1):.0f} ms",
             f"results equal to the restatement: {same}",
             "times are device events around the calls, host reads included (selection: one; a cut: one); launches per selection: "
             "9 kernels + sort + 2 cumsum; per cut: 5 kernels (+ 1 per attribute) + memset + 2 cumsum"]
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write(text)
    assert same, "the kernels and the restatement disagree"


if __name__ == "__main__":
    main()
