"""GPU: rig-wide topology-error detection (gaustar_amd.topology, gsr_topo.hip) against the numpy restatement of
detect_topo_err (tests/topo_ref.py), a planted depth error at config-C size, determinism and the entry points."""
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import topo_ref as tr
from conftest import ROOT

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CAP_DIR = np.array([0.8, 0.35, 0.5]) / np.linalg.norm([0.8, 0.35, 0.5])   # a cap on the side, away from the floor
CAP_ANGLE = 0.4          # rad: 36 cm of arc at radius 0.9
CAP_DEPTH, CAP_RAMP = 0.05, 0.01


def _opaque(m):
    """Opacity 0.9997 (alpha is clamped at 0.99) and twice the initial in-plane scale: a surface that hides what is behind it,
    as a trained one does.  Otherwise the depth of the surface behind leaks into the render by a millimetre or so, and a
    dent on the far side of the sphere shows in front of it."""
    with torch.no_grad():
        m.all_densities.fill_(8.0)
        m._scales.add_(math.log(2.0))    # every surface pixel under at least two Gaussians: transmittance 1e-4 behind them
    return m


def _model(level):
    from gaustar_amd import harness, scene
    v, f = scene.icosphere(level, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    return _opaque(harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), sh_levels=1))


def _small_cams():
    from gaustar_amd import harness, scene
    eyes = [(3.0 * np.cos(a), 1.2 + 0.8 * np.sin(3 * a), 3.0 * np.sin(a)) for a in np.linspace(0, 2 * np.pi, 8, endpoint=False)]
    return [harness.nerf_camera_from_scene(scene.look_at_camera(e, scene.SUBJECT_CENTER, 480, 270, focal_px=300.0)) for e in eyes]


def _ring_cams():
    from gaustar_amd import harness, scene
    return [harness.nerf_camera_from_scene(c) for c in scene.ring_cameras()]


def _inside(verts):
    """Arc distance inside the cap's boundary (negative outside)."""
    from gaustar_amd import scene
    d = verts.astype(np.float64) - np.asarray(scene.SUBJECT_CENTER)
    theta = np.arccos(np.clip(d @ CAP_DIR / np.linalg.norm(d, axis=1), -1, 1))
    return scene.SUBJECT_RADIUS * (CAP_ANGLE - theta)


def _gt_depth(model, cams, planted):
    """GT depth = the depth render of the same model, optionally with the cap pushed inward by 5 cm (1 cm smooth ramp)."""
    from gaustar_amd import harness, topology, scene
    m = model
    if planted:
        v = model._points.detach().cpu().numpy()
        t = np.clip(_inside(v) / CAP_RAMP, 0, 1)
        push = CAP_DEPTH * t * t * (3 - 2 * t)
        d = v - np.asarray(scene.SUBJECT_CENTER)
        v2 = v - push[:, None] * d / np.linalg.norm(d, axis=1, keepdims=True)
        m = _opaque(harness.SurfaceGaussians(torch.from_numpy(v2).float().to(DEV), model._surface_mesh_faces, sh_levels=1))
    r = topology.DepthRenders(m)
    return torch.stack([r(c)[0] for c in cams])


@pytest.fixture(scope="module")
def small(hip_lib):
    model, cams = _model(4), _small_cams()
    return model, cams, _gt_depth(model, cams, True)


def test_depth_renders_are_the_reference_calls(small):
    from gaustar_amd import topology
    model, cams, _ = small
    r = topology.DepthRenders(model)
    for cam in cams[:3]:
        render, surface = r(cam)
        z = model.view_depth_colors(cam)
        with torch.no_grad():
            a = model.render_image_gaussian_rasterizer(cam, bg_color=[10.0] * 3, point_colors=z)[..., 0]
            b = model.render_image_gaussian_rasterizer(cam, bg_color=[10.0] * 3, point_colors=z, use_solid_surface=True)[..., 0]
        assert torch.equal(render, a) and torch.equal(surface, b)
        assert not torch.equal(render, surface)


def _rows_against_restatement(model, cams, gt, res, idx):
    from gaustar_amd import topology
    rig = topology.rig_from_cameras(cams)
    r = topology.DepthRenders(model)
    verts = model._points.detach().cpu().numpy()
    n_vis = 0
    for j, i in enumerate(idx):
        render, surface = (x.cpu().numpy() for x in r(cams[i]))
        want, pix = tr.camera_row(verts, gt[i].cpu().numpy(), render, surface, rig["intrinsics"][i], rig["extrinsics"][i],
                                  rig["shape"][i])
        got = res.table[j].cpu().numpy()
        vis_w, vis_g = want != -1, got != -1
        frac = (pix + 0.5) - np.floor(pix + 0.5)
        boundary = (np.minimum(frac, 1 - frac) < 1e-9).any(1)
        bad = (vis_w != vis_g) & ~boundary
        assert bad.sum() <= max(0, int(1e-4 * len(verts))), (i, int(bad.sum()))
        both = vis_w & vis_g
        np.testing.assert_allclose(got[both], want[both], rtol=0, atol=1e-6)
        n_vis += int(both.sum())
    assert n_vis > 0


def test_rows_match_the_restatement_small(small):
    from gaustar_amd import topology
    model, cams, gt = small
    res = topology.detect_topology_errors(model, cams, gt, return_stages=True)
    _rows_against_restatement(model, cams, gt, res, range(len(cams)))
    assert (res.table > 0).any()


def test_rows_match_the_restatement_one_config_c_camera(hip_lib):
    from gaustar_amd import topology
    model, cams = _model(6), _ring_cams()[70:71]
    gt = _gt_depth(model, cams, True)
    res = topology.detect_topology_errors(model, cams, gt, return_stages=True, min_observe=1)
    _rows_against_restatement(model, cams, gt, res, [0])


def test_aggregation_and_faces_match_the_restatement(small):
    from gaustar_amd import topology
    model, cams, gt = small
    res = topology.detect_topology_errors(model, cams, gt, return_stages=True, min_observe=2)
    verts = model._points.detach().cpu().numpy()
    faces = model._surface_mesh_faces.cpu().numpy()
    want = tr.rig_stages(res.table.cpu().numpy(), verts, faces, min_observe=2)
    assert torch.equal(res.count.cpu(), torch.from_numpy(want["count"]).int())
    for k in ("value", "propagated"):
        np.testing.assert_allclose(getattr(res, k).cpu().numpy(), want[k], rtol=1e-12, atol=0)
    assert res.n_voxels == len(want["voxel_keys"])
    # a vertex whose K-th and (K+1)-th nearest voxels are (nearly) tied may pick the other one: the only mismatch allowed,
    # on at most 0.1 % of the vertices
    idx, dist = tr.knn(verts, want["voxel_centre"].astype(np.float32), 9)
    tie = np.abs(dist[:, 8] - dist[:, 7]) <= 1e-6 * np.maximum(dist[:, 7], 1e-30)
    got = res.interpolated.cpu().numpy()
    off = ~np.isclose(got, want["interpolated"], rtol=1e-9, atol=1e-12)
    assert not (off & ~tie).any() and off.sum() <= 1e-3 * len(verts), (int((off & ~tie).sum()), int(off.sum()))
    fc = res.face_colour.cpu().numpy().astype(int)
    diff = np.abs(fc - want["face_colour"].astype(int))
    assert diff.max() <= 1 and (diff > 0).sum() <= 1e-3 * len(fc)
    assert (want["value"] > 0).any()
    np.testing.assert_array_equal(res.face_loss.cpu().numpy(), (fc / 255).astype(np.float32))


@pytest.fixture(scope="module")
def config_c(hip_lib):
    model, cams = _model(6), _ring_cams()
    return model, cams, _gt_depth(model, cams, True)


def test_planted_error_at_config_c(config_c):
    from gaustar_amd import topology
    model, cams, gt = config_c
    res = topology.detect_topology_errors(model, cams, gt)
    verts = model._points.detach().cpu().numpy()
    faces = model._surface_mesh_faces.cpu().numpy()
    inside = _inside(verts)[faces]
    fl = res.face_loss.cpu().numpy()
    core = (inside >= 0.02).all(1)
    far = (inside < -0.10).all(1)
    assert core.sum() > 100 and far.sum() > 10000
    assert (fl[core] == 1).mean() >= 0.9, (fl[core] == 1).mean()
    assert (fl[far] > 0).mean() <= 0.005, (fl[far] > 0).mean()
    assert res.topo_change_num >= 100 and res.decision
    assert res.topo_change_num == int((res.unbind_weight[:, 0] == 0).sum()) == 6 * int((fl == 1).sum())
    clean_gt = _gt_depth(model, cams, False)
    clean = topology.detect_topology_errors(model, cams, lambda i: clean_gt[i])
    assert int(clean.face_loss.count_nonzero()) == 0 and clean.topo_change_num == 0 and not clean.decision


def test_deterministic_across_calls_and_views_in_flight(config_c):
    from gaustar_amd import topology
    model, cams, gt = config_c
    a = topology.detect_topology_errors(model, cams, gt, return_stages=True)
    b = topology.detect_topology_errors(model, cams, gt, return_stages=True)
    c = topology.detect_topology_errors(model, cams, gt, return_stages=True, views_in_flight=1)
    for x in (b, c):
        for k in ("table", "value", "propagated", "interpolated", "face_loss", "face_colour"):
            assert torch.equal(getattr(a, k), getattr(x, k)), k


_TWO_RANK = r'''
import os, sys
sys.path.insert(0, %r)
sys.path.insert(0, os.path.join(%r, "tests"))
import torch, torch.distributed as dist
from gaustar_amd import dist as gd, topology
import test_gpu_topology as t
rank, world, _ = gd.init_from_env("gloo")
torch.cuda.set_device(0)
model, cams = t._model(4), t._small_cams()
gt = t._gt_depth(model, cams, True)
res = topology.detect_topology_errors(model, cams, gt, return_stages=True, min_observe=2)
assert world == 2
if rank == 0:
    torch.save({k: getattr(res, k).cpu() for k in ("table", "value", "propagated", "interpolated", "face_loss")}, %r)
    print("TOPO2_OK")
dist.barrier()
dist.destroy_process_group()
'''


def test_two_ranks_over_gloo_equal_one_rank(tmp_path, small):
    from gaustar_amd import topology
    model, cams, gt = small
    out = str(tmp_path / "two.pt")
    script = tmp_path / "topo2.py"
    script.write_text(_TWO_RANK % (ROOT, ROOT, out))
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(script)]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "TOPO2_OK" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
    two = torch.load(out)
    one = topology.detect_topology_errors(model, cams, gt, return_stages=True, min_observe=2)
    for k, v in two.items():
        assert torch.equal(getattr(one, k).cpu(), v), k


def test_entry_points_return_the_native_result(small):
    from gaustar_amd import topology
    model, cams, gt = small
    res = topology.detect_topology_errors(model, cams, gt, mesh_prop=5)
    via_model = model.detect_topology_errors(cams, gt, mesh_prop=5)
    assert torch.equal(res.face_loss, via_model.face_loss) and res.topo_change_num == via_model.topo_change_num

    class Nerf:
        cameras = cams

        @staticmethod
        def get_gt_depth(camera_indices):
            return gt[camera_indices][..., None]

    fl = topology.detect_topo_err(model, Nerf, "unused/", topology.rig_from_cameras(cams), 0, use_depth_loss=True, depth_scalar=3,
                                  use_color_loss=False, use_densifier_grad=False, mesh_prop=5, save_inter=False,
                                  save_render=False, save_mesh=True)
    assert isinstance(fl, np.ndarray) and fl.dtype == np.float64 and fl.shape == (model._surface_mesh_faces.shape[0],)
    np.testing.assert_array_equal(fl, res.face_colour.cpu().numpy() / 255)
    assert np.array_equal(fl.astype(np.float32), res.face_loss.cpu().numpy())
