"""tools/planned_slot_time.py TAG [views...] -- config C under PLANNED binning: the forward blend's slot time (sum of its workgroups'
durations, from the trace stamps of the ordinary build), its number of workgroups and the share of tiles behind the non-empty
ones; the share of the backward's units past their list's end; and (TAG == parent: exact binning) how many of the backward's
dead (unit, block) waves lie in units at or behind every pixel's last contributor (profiles/planned_light_tiles.txt).
GSR_LIB_PATH chooses the build."""
import ctypes, os, sys
import numpy as np
sys.path.insert(0, os.getcwd())
import torch
from gaustar_amd import _lib, scene
from gaustar_amd import rasterizer as R

tag = sys.argv[1]
views = [int(a) for a in sys.argv[2:]] or [0, 90]
gs, cams, bg = scene.config_C()
dev = torch.device("cuda:0"); lib = _lib.load()
t = lambda x: torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
ps = (t(gs.means3D), t(gs.colors_precomp), t(gs.opacities), t(gs.scales), t(gs.rotations))
p_ = lambda x: x.data_ptr()
for view in views:
    cam = cams[view]
    W, H = cam.W, cam.H; gx, gy = (W + 15) // 16, (H + 15) // 16; T = gx * gy
    args = (t(bg), *ps, 1.0, torch.Tensor([]), t(cam.viewmatrix), t(cam.projmatrix), cam.tanfovx, cam.tanfovy, H, W, torch.Tensor([]), 0,
            t(cam.campos), False, False)
    R.drop_plans()
    R.rasterize_gaussians_native(*args, use_plan=False)
    for _ in range(4):
        before = R.PLAN_STATS["planned"]
        out = R.rasterize_gaussians_native(*args)
        torch.cuda.synchronize()
    assert R.PLAN_STATS["planned"] - before == 1
    trace = torch.zeros(2 * T + 2 * 65536 + 16 * T + 64, dtype=torch.int64, device=dev)
    lib.gsr_debug_set_trace(ctypes.c_void_p(trace.data_ptr()))
    out = R.rasterize_gaussians_native(*args)
    torch.cuda.synchronize(); lib.gsr_debug_set_trace(None)
    Rn, _c, _r, geom, binning, img, _m, U = out
    pi = next(iter(R._PLANS.values())).pi
    rg = torch.zeros(T, 2, dtype=torch.int32, device=dev)
    lib.gsr_debug_export(gs.P, Rn, U, W, H, p_(geom), None, p_(img), None, None, None, None, p_(rg), None, None, None, None)
    torch.cuda.synchronize()
    n = (rg[:, 1] - rg[:, 0]).cpu().numpy().astype(np.int64)
    se = trace.cpu().numpy()[:2 * T].astype(np.float64).reshape(T, 2) / 100.0
    ran = se[:, 1] > 0
    dur = np.where(ran, se[:, 1] - se[:, 0], 0.0)
    ne = int((n > 0).sum())
    t0 = se[ran, 0].min()
    n_light = int(pi.reserved1[1])
    print(f"[{tag}] view {view}: planned forward: {int(ran.sum())} workgroups stamped (+1 plan job), span {se[ran, 1].max() - t0:.1f} us, "
          f"slot time {dur.sum() / 1e3:.2f} ms.us; {ne} non-empty tiles {dur[:ne].sum() / 1e3:.2f} ms.us; behind them {int(ran[ne:].sum())} "
          f"workgroups {dur[ne:].sum() / 1e3:.2f} ms.us (mean {dur[ne:][ran[ne:]].mean():.2f} us); light tiles of the plan {n_light}")
    units_used = int(((n + 63) // 64).sum())
    print(f"[{tag}] view {view}: plan U_cap {pi.U_cap}, units that hold entries {units_used}: {100.0 * (pi.U_cap - units_used) / pi.U_cap:.1f} % "
          f"of the backward's waves leave at the s0 >= n test")
    if tag != "parent":
        continue
    # exact binning: dead (unit, block) waves, and those at or behind ceil(n_eff / 64), n_eff = the tile's deepest last contributor
    out = R.rasterize_gaussians_native(*args, need_backward=True, use_plan=False)
    Rn, _c, _r, geom, binning, img, _m, U = out
    nc = torch.zeros(H, W, dtype=torch.int32, device=dev); masks = torch.zeros(max(U, 1), 4, 64, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    lib.gsr_debug_export(gs.P, Rn, U, W, H, p_(geom), p_(binning), p_(img), None, None, None, None, p_(rg), None, None, p_(nc), None)
    lib.gsr_debug_export_masks(Rn, U, p_(binning), p_(masks), None)
    torch.cuda.synchronize()
    n = (rg[:, 1] - rg[:, 0]).cpu().numpy().astype(np.int64)
    units = (n + 63) // 64
    unit0 = np.concatenate([[0], np.cumsum(units)])
    assert int(unit0[-1]) == U
    words = masks.cpu().numpy().view(np.uint64)
    ncp = np.zeros((gy * 16, gx * 16), np.int64); ncp[:H, :W] = nc.cpu().numpy()
    nct = ncp.reshape(gy, 2, 8, gx, 2, 8).transpose(0, 3, 1, 4, 2, 5).reshape(T, 4, 64)
    tile_of = np.repeat(np.arange(T), units)
    u_local = np.arange(U) - unit0[tile_of]
    lim = np.clip(nct[tile_of] - 64 * u_local[:, None, None], 0, 64).astype(np.uint64)
    below = np.where(lim >= 64, np.uint64(0xffffffffffffffff), (np.uint64(1) << (lim & np.uint64(63))) - np.uint64(1))
    kept = np.bitwise_or.reduce(words & below, axis=2)         # [U, 4]
    dead = kept == 0
    n_eff = nct.reshape(T, -1).max(axis=1)
    behind = (u_local >= (n_eff[tile_of] + 63) // 64)[:, None] & dead
    print(f"[{tag}] view {view}: exact binning: {4 * U} backward waves, dead {int(dead.sum())} ({100.0 * dead.sum() / (4 * U):.1f} %), of those in "
          f"units at or behind ceil(n_eff / 64): {int(behind.sum())} ({100.0 * behind.sum() / max(int(dead.sum()), 1):.1f} % of the dead)")
