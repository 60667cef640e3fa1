"""GPU: scene-flow mesh warping (gaustar_amd.warp, gsr_warp.hip) against the numpy restatement of warp_mesh_using_flow
(tests/warp_ref.py), a known rigid motion at config C (tests/warp_scene.py), determinism and the drop-in adapter."""
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import warp_ref as wr
import warp_scene as ws
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _rig(cams):
    from gaustar_amd import harness, topology
    return topology.rig_from_cameras([harness.nerf_camera_from_scene(c) for c in cams])


def _small_rig(n_azim=8):
    from gaustar_amd import scene
    return _rig(scene.ring_cameras(n_rings=5, n_azim=n_azim, W=480, H=270, focal_px=300.0))


def _mesh(level, isolated=False):
    """(verts f64 numpy, faces int64 numpy); `isolated` appends a vertex no face uses (inside the sphere)."""
    from gaustar_amd import scene
    v, f = scene.icosphere(level, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    v = v.astype(np.float64)
    if isolated:
        v = np.concatenate([v, np.asarray(scene.SUBJECT_CENTER, np.float64)[None]])
    return v, f


def _frames(rig, device=DEV, flow_shape=None, pad=None):
    from gaustar_amd import scene
    return [ws.frames(rig["extrinsics"][i], rig["intrinsics"][i], rig["shape"][i], scene.SUBJECT_CENTER, scene.SUBJECT_RADIUS,
                      device, flow_shape, pad) for i in range(len(rig["shape"]))]


def _faces_t(f):
    return torch.from_numpy(f).long().to(DEV)


def _rows_against_restatement(v, f, rig, fr, res, cfg=wr.CFG, pad=None):
    normals = wr.vertex_normals(v, f)
    np.testing.assert_allclose(res.normals.cpu().numpy(), normals, rtol=0, atol=1e-12)
    n_vis = 0
    for i in range(len(rig["shape"])):
        ff, fb, dc, dn = (x.cpu().numpy() for x in fr[i])
        want, m = wr.camera_row(v, normals, ff, fb, pad, dc, dn, rig["intrinsics"][i], rig["extrinsics"][i], rig["shape"][i], cfg)
        got = res.table[i].cpu().numpy()
        vw, vg = ~np.isnan(want[:, 0]), ~np.isnan(got[:, 0])
        assert np.array_equal(np.isnan(got).any(1), np.isnan(got).all(1))
        close = m["quant"] < 1e-9
        for k, x in m.items():
            if k != "quant":
                close |= np.abs(x) < 1e-9
        bad = (vw != vg) & ~close
        assert not bad.any(), (i, int(bad.sum()), int((vw != vg).sum()))
        both = vw & vg
        np.testing.assert_allclose(got[both], want[both], rtol=0, atol=1e-9)
        n_vis += int(both.sum())
    return n_vis


def test_rows_match_the_restatement_small(hip_lib):
    from gaustar_amd import warp
    rig = _small_rig(2)                       # 10 cameras at 480x270
    v, f = _mesh(4)
    fr = _frames(rig)
    cfg = warp.WarpConfig(edge_scalar=100)
    res = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], cfg, return_stages=True)
    n = _rows_against_restatement(v, f, rig, fr, res, dict(wr.CFG, edge_scalar=100))
    assert n > 500, n
    # the default config too (almost nothing passes the edge test at this resolution; the rows must still agree)
    res = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], return_stages=True)
    _rows_against_restatement(v, f, rig, fr, res)


def test_rows_match_the_restatement_config_c_camera_padded_flow(hip_lib):
    """One config-C camera whose flows are stored at 432x768 with a pad (4, 4, 8, 8): ratios 1080 / 440 and 1920 / 784."""
    from gaustar_amd import scene, warp
    cams = scene.ring_cameras()
    rig = _rig(cams[70:72])
    v, f = _mesh(6)
    pad = (4, 4, 8, 8)
    fr = _frames(rig, flow_shape=(432, 768), pad=pad)
    assert tuple(fr[0][0].shape) == (432, 768, 2)
    res = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], pad=np.array(pad, np.float64), return_stages=True,
                         cfg=warp.WarpConfig(min_observe=1))
    n = _rows_against_restatement(v, f, rig, fr, res, pad=pad)
    assert n > 100, n


def test_rig_stages_match_the_restatement(hip_lib):
    """40 small cameras, edge_scalar 100, min_observe 2; the mesh carries one isolated vertex (NaN after smoothing)."""
    from gaustar_amd import warp
    rig = _small_rig()
    v, f = _mesh(4, isolated=True)
    fr = _frames(rig)
    cfg = warp.WarpConfig(edge_scalar=100, min_observe=2)
    res = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], cfg, return_stages=True)
    want = wr.rig_stages(res.table.cpu().numpy(), v, f, min_observe=2)
    assert torch.equal(res.observed.cpu(), torch.from_numpy(want["observed"]).int())
    assert torch.equal(res.count.cpu(), torch.from_numpy(want["count"]).int())
    assert (want["count"] >= 2).mean() > 0.3
    for k in ("move_raw", "move_propagated", "move_smoothed"):
        np.testing.assert_allclose(getattr(res, k).cpu().numpy(), want[k], rtol=1e-12, atol=0, equal_nan=True)
    sm = res.move_smoothed.cpu().numpy()
    assert np.isnan(sm[-1]).all() and not np.isnan(sm[:-1]).any()
    assert torch.equal(res.verts_smoothed.nan_to_num(7.0), (torch.from_numpy(v).to(DEV) + res.move_smoothed).nan_to_num(7.0))


def _aggregate_on_gpu(table, min_observe):
    """gsr_warp_aggregate on a [C,V,3] f64 table (NaN = not visible) -> (move, observed, count, valid) as numpy."""
    import ctypes
    from gaustar_amd import _lib
    lib = _lib.load()
    t = torch.from_numpy(np.ascontiguousarray(table, np.float64)).to(DEV)
    C, V = t.shape[0], t.shape[1]
    move = torch.full((V, 3), 123.0, dtype=torch.float64, device=DEV)
    observed, count = (torch.full((V,), -7, dtype=torch.int32, device=DEV) for _ in range(2))
    valid = torch.full((V,), 9, dtype=torch.uint8, device=DEV)
    p = lambda x: ctypes.c_void_p(x.data_ptr())
    _lib.check(lib.gsr_warp_aggregate(C, V, p(t), int(min_observe), p(move), p(observed), p(count), p(valid),
                                      ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "gsr_warp_aggregate")
    return move.cpu().numpy(), observed.cpu().numpy(), count.cpu().numpy(), valid.cpu().numpy()


def _outlier_table():
    """[10 cameras, V, 3]: hand-built columns first, then 300 random ones with heavy tails and random visibility."""
    C = 10
    cols = []
    spread = lambda n: np.stack([np.arange(n) * 1e-3, np.arange(n) * 2e-3 - 0.004, np.arange(n) * -1e-3], 1)
    a = spread(10); a[4, 0] = 100.0                        # 0: one far above in x: dropped (z = 3 > 2)
    cols.append(a)
    b = spread(10); b[4, 1] = -100.0                       # 1: one far below in y: kept (the test is one-sided)
    cols.append(b)
    cols.append(np.tile([[0.01, -0.02, 0.03]], (7, 1)))    # 2: seven identical rows: std 0, z = 0 / 0 = NaN, all dropped
    d = spread(6); d[5, 2] = 10.0                          # 3: six rows, one dropped (z = sqrt(5)): 5 kept, below min_observe 6
    cols.append(d)
    cols.append(spread(3))                                 # 4: three observations: below min_observe, no removal
    cols.append(np.zeros((0, 3)))                          # 5: never observed
    rng = np.random.default_rng(5)
    table = np.full((C, len(cols) + 300, 3), np.nan)
    for v, x in enumerate(cols):
        cams = np.sort(rng.choice(C, len(x), replace=False))          # observations spread over the cameras, NaN between
        table[cams, v] = x
    vis = rng.random((C, 300)) < 0.8
    vals = rng.standard_t(2, (C, 300, 3)) * 0.01
    table[:, len(cols):][vis] = vals[vis]
    return table


def test_aggregate_outlier_removal_matches_the_restatement(hip_lib):
    """gsr_warp_aggregate on a hand-built table against warp_ref.aggregate (remove_outlier, warp_mesh.py:174-181 and :351-358):
    a far-above outlier dropped, a far-below one kept, identical rows (std 0) all dropped, removal taking the count below
    min_observe (move 0), too few observations, none; then random heavy-tailed columns."""
    table = _outlier_table()
    for mo in (6, 4):
        move, observed, count, valid = _aggregate_on_gpu(table, mo)
        w_move, w_obs, w_cnt = wr.aggregate(table, mo)
        np.testing.assert_array_equal(observed, w_obs)
        np.testing.assert_array_equal(count, w_cnt)
        np.testing.assert_array_equal(valid, (w_cnt >= mo).astype(np.uint8))
        np.testing.assert_allclose(move, w_move, rtol=1e-14, atol=0)
        assert (count < observed).sum() >= 5, int((count < observed).sum())
        assert ((observed >= mo) & (count < mo)).any()
    move, observed, count, valid = _aggregate_on_gpu(table, 6)
    assert list(observed[:6]) == [10, 10, 7, 6, 3, 0] and list(count[:6]) == [9, 10, 0, 5, 3, 0]
    assert list(valid[:6]) == [1, 1, 0, 0, 0, 0]
    x = table[:, 0][~np.isnan(table[:, 0, 0])]
    np.testing.assert_allclose(move[0], np.delete(x, 4, 0).mean(0), rtol=1e-15, atol=0)
    assert move[1, 1] < -9.0                                # the far-below row is in the mean
    assert not move[2:6].any()


@pytest.fixture(scope="module")
def config_c(hip_lib):
    from gaustar_amd import scene
    rig = _rig(scene.ring_cameras())
    v, f = _mesh(6)
    fr = _frames(rig)
    torch.cuda.synchronize()
    return rig, v, _faces_t(f), fr


def _motion_errors(res, v):
    from gaustar_amd import scene
    want = ws.moved(v, scene.SUBJECT_CENTER)
    good = res.count.cpu().numpy() >= 4
    e = {k: np.linalg.norm(getattr(res, k).cpu().numpy() - want, axis=1) for k in ("verts_raw", "verts_propagated", "verts_smoothed")}
    return good, e


def test_known_motion_at_config_c(config_c):
    """The independent pin: warped vertices against R (v - c) + c + t (the motion is up to 99 mm).

    With the reference's edge scale (10 000) at most 3 of the 160 cameras pass a vertex here (observed when written: 27467 /
    11675 / 1783 / 37 vertices seen by 0 / 1 / 2 / 3 cameras), so nothing reaches min_observe = 4 and nothing moves.  The edge
    test keeps var below 1e-5 of the silhouette's (0.040 m^2 at camera 70), which admits only surfaces within about 7-10
    degrees of facing at 1200 px focal length (3.7 % of the subject's pixels in exact f64, 2.75 % in the reference's f32).  At
    edge_scalar = 1000, observed when written: 82.0 % with count >= 4; raw error median 0.055 mm, p99 0.187 mm, max 0.375 mm
    over them; smoothed median 0.062 mm, max 54.1 mm (vertices no camera passes, propagated from far away)."""
    from gaustar_amd import warp
    rig, v, ft, fr = config_c
    res = warp.warp_mesh(v, ft, rig, lambda i: fr[i])
    assert int(res.observed.max()) < 4 and int(res.count.max()) < 4 and not res.move_smoothed.any()
    res = warp.warp_mesh(v, ft, rig, lambda i: fr[i], warp.WarpConfig(edge_scalar=1000))
    good, e = _motion_errors(res, v)
    r = e["verts_raw"][good]
    print(f"\nedge_scalar 1000: count>=4 {good.mean():.4f}; raw median {1e3 * np.median(r):.3f} mm p99 "
          f"{1e3 * np.percentile(r, 99):.3f} max {1e3 * r.max():.3f}; smoothed median {1e3 * np.median(e['verts_smoothed']):.3f} "
          f"max {1e3 * e['verts_smoothed'].max():.3f}")
    assert good.mean() >= 0.75
    assert np.median(r) <= 2e-4 and np.percentile(r, 99) <= 5e-4 and r.max() <= 1e-3
    assert np.median(e["verts_smoothed"]) <= 2e-4 and e["verts_smoothed"].max() <= 0.07


def test_deterministic_across_calls_and_views_in_flight(config_c):
    from gaustar_amd import warp
    rig, v, ft, fr = config_c
    a = warp.warp_mesh(v, ft, rig, lambda i: fr[i], return_stages=True)
    b = warp.warp_mesh(v, ft, rig, lambda i: fr[i], return_stages=True)
    c = warp.warp_mesh(v, ft, rig, lambda i: fr[i], return_stages=True, views_in_flight=1)
    for x in (b, c):
        for k in ("table", "move_raw", "move_propagated", "move_smoothed", "observed", "count"):
            assert torch.equal(getattr(a, k).nan_to_num(7.0) if getattr(a, k).is_floating_point() else getattr(a, k),
                               getattr(x, k).nan_to_num(7.0) if getattr(x, k).is_floating_point() else getattr(x, k)), k


_TWO_RANK = r'''
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import torch, torch.distributed as dist
from gaustar_amd import dist as gd, warp
import test_gpu_warp as t
rank, world, _ = gd.init_from_env("gloo")
torch.cuda.set_device(0)
rig = t._small_rig()
v, f = t._mesh(4, isolated=True)
fr = t._frames(rig)
res = warp.warp_mesh(v, t._faces_t(f), rig, lambda i: fr[i], warp.WarpConfig(edge_scalar=100, min_observe=2), return_stages=True)
assert world == 2
if rank == 0:
    torch.save({k: getattr(res, k).cpu() for k in ("table", "move_raw", "move_propagated", "move_smoothed", "count")}, %r)
    print("WARP2_OK")
dist.barrier()
dist.destroy_process_group()
'''


def test_two_ranks_over_gloo_equal_one_rank(tmp_path, hip_lib):
    from gaustar_amd import warp
    out = str(tmp_path / "two.pt")
    script = tmp_path / "warp2.py"
    script.write_text(_TWO_RANK % (ROOT, ROOT, out))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "WARP2_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    two = torch.load(out)
    rig = _small_rig()
    v, f = _mesh(4, isolated=True)
    fr = _frames(rig)
    one = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], warp.WarpConfig(edge_scalar=100, min_observe=2), return_stages=True)
    for k, x in two.items():
        y = getattr(one, k).cpu()
        assert torch.equal(y.nan_to_num(7.0) if y.is_floating_point() else y, x.nan_to_num(7.0) if x.is_floating_point() else x), k


def test_drop_in_adapter_writes_the_reference_files(tmp_path, hip_lib):
    from gaustar_amd import formats, warp
    rig = _small_rig(2)
    C = len(rig["shape"])
    v, f = _mesh(4)
    fr = _frames(rig, device="cpu", flow_shape=(128, 240), pad=(3, 3, 0, 0))
    data = tmp_path / "data"
    for d in ("0005/flow_bi", "0005/depth", "0006/depth"):
        (data / d).mkdir(parents=True)
    np.savez(data / "rgb_cameras.npz", **rig)
    np.savetxt(data / "0005/flow_bi/pad.txt", [3.0, 3.0, 0.0, 0.0])
    for i in range(C):
        ff, fb, dc, dn = (x.numpy() for x in fr[i])
        np.savez_compressed(data / f"0005/flow_bi/{i:04d}_f.npz", flow=ff)
        np.savez_compressed(data / f"0005/flow_bi/{i:04d}_b.npz", flow=fb)
        np.savez_compressed(data / f"0005/depth/img_{i:04d}_depth.npz", depth=dc)
        np.savez_compressed(data / f"0006/depth/img_{i:04d}_depth.npz", depth=dn)
    col = np.random.default_rng(0).random((len(v), 3))
    formats.save_obj(str(tmp_path / "mesh.obj"), v, f, col)
    work = str(tmp_path / "work") + "/"
    res = warp.warp_mesh_using_flow(str(tmp_path / "mesh.obj"), str(data) + "/", work, 5)
    out = work + "0006/coarse_mesh/"
    assert os.path.exists(out + "config.json")
    for name, key, colours in (("warp_0005.obj", "verts_raw", None), ("warp_mesh_prop.obj", "verts_propagated", col),
                               ("warp_smooth.obj", "verts_smoothed", col)):
        v2, f2, c2 = formats.load_obj(out + name)
        assert np.array_equal(v2, getattr(res, key).cpu().numpy(), equal_nan=True), name
        assert np.array_equal(f2, f)
        assert (c2 is None) if colours is None else np.array_equal(c2, colours)
    direct = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], pad=(3, 3, 0, 0))
    assert torch.equal(direct.move_smoothed, res.move_smoothed)


def test_model_method_delegates(hip_lib):
    from gaustar_amd import harness, scene, warp
    rig_cams = [harness.nerf_camera_from_scene(c) for c in scene.ring_cameras(n_rings=5, n_azim=2, W=480, H=270, focal_px=300.0)]
    v, f = scene.icosphere(4, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    model = harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), sh_levels=1)
    from gaustar_amd import topology
    rig = topology.rig_from_cameras(rig_cams)
    fr = _frames(rig)
    a = model.warp_mesh(rig_cams, lambda i: fr[i], cfg=warp.WarpConfig(edge_scalar=100))
    b = warp.warp_mesh(model._points.detach(), model._surface_mesh_faces, rig, lambda i: fr[i], cfg=warp.WarpConfig(edge_scalar=100))
    assert torch.equal(a.move_smoothed, b.move_smoothed) and int((a.count > 0).sum()) > 0
