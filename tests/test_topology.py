"""CPU: the numpy restatement of detect_topo_err (tests/topo_ref.py) against independent statements of its library pieces,
and the host side of gaustar_amd.topology (rig layout, result bookkeeping, the adapter's option checks)."""
import math

import numpy as np
import pytest
import torch

import topo_ref as tr
from gaustar_amd import harness, scene, topology


def test_box_filter_is_reflect101_uniform_filter():
    from scipy import ndimage
    rng = np.random.default_rng(0)
    for shape in ((7, 5), (2, 9), (31, 17)):
        a = rng.random(shape) * 5
        np.testing.assert_allclose(tr.box3(a), ndimage.uniform_filter(a, size=3, mode="mirror"), rtol=0, atol=1e-12)


def test_depth_edge_clips_at_1p1_of_the_max_below_10():
    g = np.full((6, 6), 2.0, np.float32)
    g[:, 3:] = 50.0                                   # background: clipped to 1.1 * 2
    var = tr.depth_edge(g)
    assert var[:, 0].max() == 0 and var[:, 2].max() > 0
    d = np.minimum(g, np.float32(2.2))
    col = np.array([2.0, 2.0, 2.2], np.float64)       # the 3x3 window around column 2: columns 1, 2, 3
    want = np.float32(np.float32((col ** 2).sum() * 3 / 9) - np.float32(col.sum() * 3 / 9) ** 2)
    assert abs(var[2, 2] - want) <= 1e-6 and d.max() == np.float32(2.2)
    assert tr.depth_edge(np.full((4, 4), 12.0, np.float32)) is None


def test_lookup_semantics_on_closed_form_pixels():
    img = np.arange(12, dtype=np.float32).reshape(3, 4)   # H = 3, W = 4
    # int32(p + 0.5) truncates toward zero: valid iff p + 0.5 lies in (-1, size)
    pix = np.array([[-0.9, 0.0], [-1.2, 0.0], [3 - 0.6, 0.0], [np.nan, 0.0], [-1.6, 0.0], [3 - 0.4, 0.0], [0.0, 4 - 0.6],
                    [0.0, 4 - 0.4], [1.49, 2.51]])
    val, ok = tr.query(img, pix)
    assert ok.tolist() == [True, True, True, False, False, False, True, False, True]
    assert val[0] == 0 and val[1] == 0 and val[2] == img[2, 0] and val[6] == img[0, 3] and val[8] == img[1, 3]


def test_voxel_grid_matches_a_dict():
    rng = np.random.default_rng(1)
    p = rng.random((400, 3)) * 0.1
    val = rng.random(400)
    keys, centre, mean = tr.voxel_grid(p, val, 0.02)
    origin = p.min(0) - 0.01
    d = {}
    for x, v in zip(p, val):
        d.setdefault(tuple(int(math.floor(c)) for c in (x - origin) / 0.02), []).append(v)
    assert len(d) == len(keys)
    for k, c, m in zip(keys, centre, mean):
        vs = d[tuple(k)]
        assert m == sum(vs) / len(vs)
        np.testing.assert_allclose(c, origin + (k + 0.5) * 0.02, rtol=0, atol=1e-15)


def test_knn_matches_ckdtree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(2)
    c = rng.random((300, 3)).astype(np.float32)
    q = rng.random((200, 3)).astype(np.float32)
    idx, dist = tr.knn(q, c, 8)
    d_t, i_t = cKDTree(c.astype(np.float64)).query(q.astype(np.float64), k=8)
    assert (idx == i_t).all()
    np.testing.assert_allclose(dist, d_t ** 2, rtol=1e-5)


def _holey_mesh(seed):
    rng = np.random.default_rng(seed)
    v, f = scene.icosphere(2)
    valid = rng.random(len(v)) < 0.5
    valid[rng.choice(len(v), 10, replace=False)] = False
    return v, f, valid, rng.random(len(v)) * valid


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_sequential_propagation_equals_jacobi(seed):
    v, f, valid, value = _holey_mesh(seed)
    nb = tr.neighbours(f, len(v))
    for ite in (1, 3, 20):
        np.testing.assert_array_equal(tr.propagate_sequential(nb, valid, value, ite), tr.propagate_jacobi(nb, valid, value, ite))


def test_vertex_neighbours_csr_equals_trimesh_lists():
    from gaustar_amd import meshes
    v, f = scene.icosphere(2)
    topo = meshes.MeshTopology(torch.from_numpy(f).long(), len(v))
    off, nbr = topology.vertex_neighbours(topo)
    lists = tr.neighbours(f, len(v))
    assert off.tolist() == [0] + list(np.cumsum([len(x) for x in lists]))
    assert nbr.tolist() == [u for x in lists for u in x]


def test_face_colours_truncate():
    faces = np.array([[0, 1, 2]])
    assert tr.face_colours(faces, np.array([1.0, 1.0, 0.999]))[0] == 254     # (255 + 255 + 254) / 3 = 254.67 -> 254
    assert tr.face_colours(faces, np.array([2.0, 5.0, 1.0]))[0] == 255


def _rig_cams():
    cams = [scene.look_at_camera(e, scene.SUBJECT_CENTER, 480, 270, focal_px=300.0) for e in ((0.5, 1.6, 3.0), (-2.5, 0.4, 1.5))]
    return cams, [harness.nerf_camera_from_scene(c) for c in cams]


def test_rig_from_cameras_projects_like_the_rasterizer():
    """The reference's projection (warp_mesh.py:57-74) with rig_from_cameras' matrices lands where the rasterizer's own
    matrices put a point (ndc2Pix of full_proj), up to the reference's half-pixel offset: it adds W/2, ndc2Pix W/2 - 1/2."""
    _cams, ncams = _rig_cams()
    rig = topology.rig_from_cameras(ncams)
    v, _ = scene.icosphere(2, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    assert rig["extrinsics"].dtype == np.float64 and rig["shape"].tolist() == [[270, 480]] * 2
    for i, nc in enumerate(ncams):
        rc = nc.rasterizer_camera()
        pix, _loc = tr.project(v, rig["intrinsics"][i], rig["extrinsics"][i], rig["shape"][i])
        ph = np.c_[v, np.ones(len(v))] @ rc.projmatrix.astype(np.float64)
        ndc = ph[:, :2] / ph[:, 3:4]
        px = ((ndc[:, 0] + 1.0) * rc.W - 1.0) * 0.5
        py = ((ndc[:, 1] + 1.0) * rc.H - 1.0) * 0.5
        np.testing.assert_allclose(pix[:, 1], px + 0.5, rtol=0, atol=1e-3)   # (full_proj is stored in f32)
        np.testing.assert_allclose(pix[:, 0], py + 0.5, rtol=0, atol=1e-3)
        # in double, from the same camera: the view matrix in f64 and the pinhole model give the pixel to 1e-6 px
        w2c = np.linalg.inv(np.r_[np.asarray(nc.c2w, np.float64)[:3], [[0, 0, 0, 1]]] @ np.diag([1.0, -1.0, -1.0, 1.0]))
        loc = v @ w2c[:3, :3].T + w2c[:3, 3]
        np.testing.assert_allclose(pix[:, 1], nc.fx * loc[:, 0] / loc[:, 2] + rc.W / 2, rtol=0, atol=1e-6)
        np.testing.assert_allclose(pix[:, 0], nc.fy * loc[:, 1] / loc[:, 2] + rc.H / 2, rtol=0, atol=1e-6)


def test_topo_change_num_counts_gaussians_not_faces():
    """refine.py:729-730 on a face_loss with 20 faces at 1: repeat(1 - face_loss, G) has 20 G zeros."""
    G = 6
    fc = np.zeros(50, np.uint8)
    fc[:20] = 255
    fc[20:25] = 254
    face_loss = fc / 255
    ref_unbind = torch.tensor(1 - face_loss.repeat(G))
    unbind, n = topology.unbind_weights(torch.from_numpy(face_loss).float(), torch.from_numpy(fc), G)
    assert int(n) == int((ref_unbind == 0).sum()) == 20 * G
    assert unbind.shape == (50 * G, 3) and torch.equal(unbind[:, 0] == 0, ref_unbind == 0)
    assert torch.equal(unbind[:, 1], unbind[:, 2]) and torch.allclose(unbind[:, 0].double(), ref_unbind, rtol=0, atol=1e-7)


@pytest.mark.parametrize("opt", ["use_color_loss", "use_densifier_grad", "use_opacity_loss", "save_inter", "save_render"])
def test_adapter_rejects_unimplemented_options(opt):
    kw = dict(use_depth_loss=True, depth_scalar=3, use_color_loss=False, use_densifier_grad=False, mesh_prop=20)
    kw[opt] = True
    with pytest.raises(ValueError, match=opt):
        topology.detect_topo_err(None, None, "", None, 0, **kw)
    with pytest.raises(ValueError, match="use_depth_loss"):
        topology.detect_topo_err(None, None, "", None, 0, use_depth_loss=False, use_color_loss=False)
