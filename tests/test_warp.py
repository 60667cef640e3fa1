"""CPU: the numpy restatement of warp_mesh_using_flow (tests/warp_ref.py) on closed-form cases, the OBJ reader / writer, the
config file and the drop-in adapter's input errors (raised before any launch)."""
import json
import os

import numpy as np
import pytest

import warp_ref as wr
import warp_scene as ws


def _small_rig():
    from gaustar_amd import harness, scene, topology
    cams = [harness.nerf_camera_from_scene(c) for c in scene.ring_cameras(n_rings=5, n_azim=8, W=480, H=270, focal_px=300.0)]
    return topology.rig_from_cameras(cams)


def test_restatement_recovers_a_rigid_motion():
    """40 cameras at 480x270 around a level-3 icosphere.  At a quarter of config C's resolution a pixel spans four times the
    depth, so the default edge scale (10 000) passes almost nothing; edge_scalar = 100 and min_observe = 2 leave 47 % of
    the vertices observed.  Observed when written: raw error median 0.44 mm, p99 1.15 mm, max 1.64 mm over them; the motion
    itself is up to 99 mm."""
    from gaustar_amd import scene
    rig = _small_rig()
    cfg = dict(wr.CFG, edge_scalar=100)
    v, f = scene.icosphere(3, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    v = v.astype(np.float64)
    n = wr.vertex_normals(v, f)
    rows = []
    for i in range(len(rig["shape"])):
        fr = [x.numpy() for x in ws.frames(rig["extrinsics"][i], rig["intrinsics"][i], rig["shape"][i], scene.SUBJECT_CENTER,
                                           scene.SUBJECT_RADIUS)]
        rows.append(wr.camera_row(v, n, fr[0], fr[1], None, fr[2], fr[3], rig["intrinsics"][i], rig["extrinsics"][i],
                                  rig["shape"][i], cfg)[0])
    st = wr.rig_stages(np.stack(rows), v, f, min_observe=2)
    want = ws.moved(v, scene.SUBJECT_CENTER)
    good = st["count"] >= 2
    err = np.linalg.norm(v + st["move_raw"] - want, axis=1)[good]
    assert good.mean() >= 0.4, good.mean()
    assert np.median(err) <= 1e-3 and err.max() <= 3e-3, (np.median(err), err.max())
    assert np.linalg.norm(want - v, axis=1).max() > 0.09
    assert (st["observed"] >= st["count"]).all()


def test_flow_pad_and_resize_closed_form():
    rng = np.random.default_rng(0)
    raw = rng.standard_normal((4, 5, 2)).astype(np.float32)
    # 2x upscale: every source pixel becomes a 2x2 block, values x2 (f32), (x, y) swapped to (row, col)
    out = wr.pad_and_resize_flow(raw, None, (8, 10))
    want = np.repeat(np.repeat(raw * np.float32(2.0), 2, 0), 2, 1)[..., ::-1]
    assert out.dtype == np.float32 and np.array_equal(out, want)
    # a non-integer ratio: source index min(floor(x * (1 / (W / w))), w - 1)
    out = wr.pad_and_resize_flow(raw, None, (7, 12))
    s = np.float32(7 / 4)
    sy = [min(int(np.floor(y * (1.0 / (7 / 4)))), 3) for y in range(7)]
    sx = [min(int(np.floor(x * (1.0 / (12 / 5)))), 4) for x in range(12)]
    assert sy == [0, 0, 1, 1, 2, 2, 3] and sx == [0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4]
    for y in range(7):
        for x in range(12):
            assert np.array_equal(out[y, x], (raw[sy[y], sx[x]] * s)[::-1])
    # a pad (top, bottom, left, right), truncated to int32: zeros outside the raw flow, the scale uses the padded height
    out = wr.pad_and_resize_flow(raw, [1.9, 1, 2, 0], (6, 7))
    assert out.shape == (6, 7, 2)
    assert np.array_equal(out[0], np.zeros((7, 2), np.float32)) and np.array_equal(out[:, :2], np.zeros((6, 2, 2), np.float32))
    assert np.array_equal(out[1, 2], raw[0, 0, ::-1] * np.float32(1.0)) and np.array_equal(out[4, 6], raw[3, 4, ::-1])


def test_box7_and_edge_map():
    rng = np.random.default_rng(1)
    d = (2.0 + rng.random((9, 11))).astype(np.float32)
    b = wr.box7(d)
    p = np.pad(d.astype(np.float64), 3, mode="reflect")
    ref = np.array([[p[y:y + 7, x:x + 7].sum() / 49 for x in range(11)] for y in range(9)])
    assert np.allclose(b, ref, rtol=1e-7, atol=0)
    assert wr.depth_edge7(np.full((5, 5), 10.0, np.float32)) is None          # nothing below 10
    assert wr.edge_vis(np.full((8, 8), 3.0, np.float32)) is None              # flat: max(var) = 0


def test_remove_outlier_edge_cases():
    same = np.tile([[0.1, 0.2, 0.3]], (5, 1))
    assert wr.remove_outlier(same).shape[0] == 0             # std 0: z = 0 / 0 = NaN drops every row
    x = np.zeros((10, 3))
    x[:, 1] = np.arange(10)
    x[:, 2] = np.arange(10) * 0.5
    x[0] = [-100.0, 0.0, 0.0]                                 # far below: one-sided, so it stays
    x[9, 0] = 100.0                                           # far above: dropped
    kept = wr.remove_outlier(x)
    assert kept.shape[0] == 9 and (kept[:, 0] == -100).any() and not (kept[:, 0] == 100).any()
    move, observed, count = wr.aggregate(x[:, None, :], 4)          # ten cameras, one vertex
    assert observed[0] == 10 and count[0] == 9
    assert np.array_equal(move[0], np.mean(kept, axis=0))


def test_smoothing_isolated_vertex_is_nan():
    nb = [[1], [0], []]
    out = wr.smooth(nb, np.array([[1.0, 2, 3], [3.0, 4, 5], [0.0, 0, 0]]), 1)
    assert np.array_equal(out[0], [3, 4, 5]) and np.array_equal(out[1], [1, 2, 3]) and np.isnan(out[2]).all()


def test_obj_round_trip_is_exact(tmp_path):
    from gaustar_amd import formats
    rng = np.random.default_rng(2)
    v = rng.standard_normal((50, 3)) * 10.0 ** rng.integers(-8, 8, (50, 1))
    v[3, 1] = np.nan
    f = rng.integers(0, 50, (80, 3))
    col = rng.random((50, 3))
    p = str(tmp_path / "m.obj")
    formats.save_obj(p, v, f, col)
    v2, f2, c2 = formats.load_obj(p)
    assert np.array_equal(v, v2, equal_nan=True) and np.array_equal(f, f2) and np.array_equal(col, c2)
    formats.save_obj(p, v, f)
    assert formats.load_obj(p)[2] is None
    # vt / vn / slashed corners / negative indices accepted, order kept; quads rejected
    (tmp_path / "t.obj").write_text("# c\nv 0 0 0\nv 1 0 0\nvt 0 0\nvn 0 0 1\nv 0 1 0\nf 1/1/1 2//1 -1/1\n")
    v3, f3, _ = formats.load_obj(str(tmp_path / "t.obj"))
    assert np.array_equal(v3, [[0, 0, 0], [1, 0, 0], [0, 1, 0]]) and np.array_equal(f3, [[0, 1, 2]])
    (tmp_path / "q.obj").write_text("v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 4 3\n")
    with pytest.raises(ValueError):
        formats.load_obj(str(tmp_path / "q.obj"))


def test_save_cfg_writes_the_reference_keys(tmp_path):
    from gaustar_amd import warp
    warp.WarpConfig().save_cfg(str(tmp_path))
    text = (tmp_path / "config.json").read_text()
    d = json.loads(text)
    assert d == {"min_observe": 4, "depth_edge_ker_size": 7, "knn_K": 8, "cmr_view_max_cos": -0.5, "max_move_dist": 0.2,
                 "voxel_size": 0.04, "bi_direct_pix_threshold": 4, "bi_direct_depth_threshold": 0.004, "edge_scalar": 10000,
                 "edge_threshold": 0.1, "post_processing": "mesh"}
    assert text == json.dumps(d, sort_keys=True, indent=4, separators=(",", ": "))
    assert list(d) == sorted(d)


def _tree(tmp_path, C=2):
    """A data root with rgb_cameras.npz, frame 0's flows and depths and frame 1's depths; a mesh."""
    root = tmp_path / "data"
    (root / "0000" / "flow_bi").mkdir(parents=True)
    for fr in ("0000", "0001"):
        (root / fr / "depth").mkdir(parents=True)
        for c in range(C):
            np.savez(root / fr / "depth" / f"img_{c:04d}_depth.npz", depth=np.full((4, 4), 3.0, np.float32))
    for c in range(C):
        for d in ("f", "b"):
            np.savez(root / "0000" / "flow_bi" / f"{c:04d}_{d}.npz", flow=np.zeros((4, 4, 2), np.float32))
    np.savez(root / "rgb_cameras.npz", intrinsics=np.tile(np.eye(3), (C, 1, 1)), extrinsics=np.tile(np.eye(4), (C, 1, 1)),
             shape=np.tile([4, 4], (C, 1)))
    from gaustar_amd import formats
    formats.save_obj(str(tmp_path / "mesh.obj"), np.eye(3), np.array([[0, 1, 2]]))
    return str(root) + "/", str(tmp_path / "work") + "/", str(tmp_path / "mesh.obj")


def test_adapter_raises_before_any_launch(tmp_path):
    from gaustar_amd import warp
    data, work, mesh = _tree(tmp_path)
    with pytest.raises(RuntimeError, match="Interval Error!"):
        warp.warp_mesh_using_flow(mesh, data, work, 0, interval=3)
    assert os.path.exists(work + "0003/coarse_mesh/config.json")          # written first, as the reference does
    with pytest.raises(ValueError):
        warp.warp_mesh_using_flow(mesh, data, work, 0, save_inter=True)
    os.remove(data + "0000/flow_bi/0001_f.npz")
    with pytest.raises(RuntimeError, match="Flow not found!"):
        warp.warp_mesh_using_flow(mesh, data, work, 0)
    data, work, mesh = _tree(tmp_path / "b")
    os.remove(data + "0000/depth/img_0001_depth.npz")
    with pytest.raises(RuntimeError, match="Depth not found!"):
        warp.warp_mesh_using_flow(mesh, data, work, 0)
    with pytest.raises(RuntimeError, match="Flow not found!"):
        warp.warp_mesh_using_flow(mesh, data, work, 0, interval=2)             # flow_bi_2f does not exist
