"""gaustar_amd.handover, TopologyUpdate.face_origin / with_colors and the model side of the frame hand-over on the GPU against
the numpy restatement tests/handover_ref.py (itself pinned by tests/test_handover.py).  Every output is compared bit for bit:
the colours are integers, and the two float results (the SH dc, and the face colours' f32 steps before the truncation) are
defined operation by operation."""
import functools

import numpy as np
import pytest
import torch

import handover_ref as ref
import regions_ref as rr
import splice_ref
from test_gpu_splice import _Mesh, _check_update, _n, _regions_of, _t
from test_handover import GS, edge_dc, fan_case, origin_want
from test_splice import GAP_FACE, chain_case, chain_want, grid_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FS = (1, 63, 64, 65, 1000)


def _bary(G):
    return torch.tensor(ref.BARY_COORDS[G], dtype=torch.float32, device=DEV)


# ---------------------------------------------------------------------------------------------------- 1a
@pytest.mark.parametrize("G", GS)
def test_face_colors(G):
    from gaustar_amd import handover
    flipped = 0
    for F in FS:
        dc = edge_dc(G, F)
        want = ref.sh_face_colors(dc, G)
        got = handover.sh_face_colors(_t(dc), G)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (F, 4)
        assert np.array_equal(_n(got), want), np.nonzero((_n(got) != want).any(axis=1))[0][:10]
        if F >= 254:                                  # the restatement's answers differ between the neighbours of an edge
            trip = want[:, :3].reshape(-1)[:762].reshape(254, 3)
            flipped = int((trip[:, 0] != trip[:, 2]).sum())
    assert flipped > 100
    # the parameter's own layout [N,1,3], and the same bytes twice
    dc = edge_dc(G, 1000)
    a = handover.sh_face_colors(_t(dc).view(-1, 1, 3), G)
    assert np.array_equal(_n(a), ref.sh_face_colors(dc, G)) and torch.equal(a, handover.sh_face_colors(_t(dc), G))
    if G > 1:                                         # rows that are no whole number of faces
        with pytest.raises(ValueError):
            handover.sh_face_colors(_t(dc)[:7 * G + 1], G)


def test_face_colors_reject_another_G():
    from gaustar_amd import _lib, handover
    with pytest.raises((_lib.GsrError, ValueError)):
        handover.sh_face_colors(torch.zeros(10, 3, device=DEV), 2)


# ---------------------------------------------------------------------------------------------------- 1b, 1c
def _grid_colours(seed=3):
    faces, V = grid_case()
    rng = np.random.default_rng(seed)
    rgba = rng.integers(0, 256, size=(len(faces), 4)).astype(np.uint8)
    rgba[:, 3] = 255
    return np.asarray(faces), V, rgba, rng


def test_vertex_to_face_colors():
    from gaustar_amd import handover
    faces, V, _rgba, rng = _grid_colours()
    col = rng.random((V, 3)).astype(np.float32)
    col[:300] = (rng.integers(0, 256, size=(300, 3)).astype(np.float32) + np.float32(0.5)) / np.float32(255.0)     # near the ties
    col[300:310] = [[-0.25, 0.0, 1.0]] * 5 + [[1.5, 0.5, 2.5 / 255]] * 5
    for c in (col, np.concatenate([col, np.ones((V, 1), np.float32)], axis=1)):        # [V,3] and [V,4] rows
        got = handover.vertex_to_face_colors(_t(faces), _t(c))
        assert got.dtype == torch.uint8 and np.array_equal(_n(got), ref.vertex_to_face_colors(faces, c))
    got64 = handover.vertex_to_face_colors(_t(faces, torch.long), _t(col.astype(np.float64)))       # load_obj's widths
    assert np.array_equal(_n(got64), ref.vertex_to_face_colors(faces, col))
    for F in FS[:4]:
        assert np.array_equal(_n(handover.vertex_to_face_colors(_t(faces[:F]), _t(col))), ref.vertex_to_face_colors(faces[:F], col))


def test_face_to_vertex_colors():
    from gaustar_amd import handover
    faces, V, rgba, rng = _grid_colours()
    mixed = rgba.copy()
    mixed[rng.random(len(faces)) < 0.2, 3] = 0                       # faces of alpha 0 mixed in
    cases = [(faces, rgba, V), (faces, mixed, V), fan_case(),         # the fan: 300 x 255 does not fit 16 bits
             (faces, rgba, V + 7),                                     # unreferenced vertices
             (np.array([[0, 1, 2], [2, 1, 4]], np.int32), np.array([[9, 8, 7, 255], [1, 2, 4, 0]], np.uint8), 6)]
    for f, c, nv in cases:
        want = ref.face_to_vertex_colors(f, c, nv)
        got = handover.face_to_vertex_colors(_t(f), _t(c), nv)
        assert got.dtype == torch.uint8 and tuple(got.shape) == (nv, 4) and np.array_equal(_n(got), want)
        again = handover.face_to_vertex_colors(_t(f), _t(c), nv)
        assert _n(again).tobytes() == _n(got).tobytes()               # integer sums: the same bytes every call
    fan = _n(handover.face_to_vertex_colors(*[_t(a) if isinstance(a, np.ndarray) else a for a in fan_case()]))
    assert fan[0].tolist() == [255, 255, 255, 255]
    unref = _n(handover.face_to_vertex_colors(_t(faces), _t(rgba), V + 7))
    assert (unref[V:] == 0).all()


def test_out_of_range_indices_raise():
    from gaustar_amd import handover
    faces, V, rgba, rng = _grid_colours()
    col = rng.random((V, 3)).astype(np.float32)
    bad = faces.copy()
    bad[5, 1] = V
    neg = faces.copy()
    neg[70, 2] = -1
    for b in (bad, neg):
        with pytest.raises(ValueError):
            handover.vertex_to_face_colors(_t(b), _t(col))
        with pytest.raises(ValueError):
            handover.face_to_vertex_colors(_t(b), _t(rgba), V)
        with pytest.raises(ValueError):
            handover.sh_dc_from_vertex_colors(_t(b), _t(col), _bary(3))
    ff = _t(faces)
    for o in ([0, len(faces)], [-1 - len(faces)], [3, -2 ** 31 + 1]):
        with pytest.raises(ValueError):
            handover.gather_face_colors(_t(np.array(o, np.int32)), _t(rgba), ff, _t(col))
    with pytest.raises(ValueError):                                    # a fusion face that names a vertex outside the colours
        handover.gather_face_colors(_t(np.array([-1 - 5], np.int32)), _t(rgba), _t(bad), _t(col))
    ok = handover.gather_face_colors(_t(np.array([2, -1 - 4, -2 ** 31], np.int32)), _t(rgba), ff, _t(col))
    assert np.array_equal(_n(ok), ref.gather_face_colors([2, -5, -2 ** 31], rgba, faces, col)) and _n(ok)[2].tolist() == [0] * 4


# ---------------------------------------------------------------------------------------------------- 1d
@pytest.mark.parametrize("G", GS)
def test_sh_dc(G):
    from gaustar_amd import handover
    _bv, bf, _fv, _ff, _raw = chain_case()
    V = int(bf.max()) + 1
    rng = np.random.default_rng(30 + G)
    cols = (rng.random((V, 3)).astype(np.float32), np.zeros((V, 3), np.float32), np.ones((V, 3), np.float32))
    for F in FS:
        for col in cols if F == 1000 else cols[:1]:
            want = ref.sh_dc_from_vertex_colors(bf[:F], col, G)
            got = handover.sh_dc_from_vertex_colors(_t(bf[:F]), _t(col), _bary(G))
            assert got.dtype == torch.float32 and tuple(got.shape) == (F * G, 3)
            assert _n(got).tobytes() == want.tobytes(), float(np.abs(_n(got) - want).max())
    wide = np.concatenate([cols[0], np.ones((V, 1), np.float32)], axis=1).astype(np.float64)      # [V,4] float64 rows
    got = handover.sh_dc_from_vertex_colors(_t(bf, torch.long), _t(wide), _bary(G))
    assert _n(got).tobytes() == ref.sh_dc_from_vertex_colors(bf, cols[0], G).tobytes()


# ---------------------------------------------------------------------------------------------------- the update with colours
@functools.lru_cache(maxsize=None)
def _colours(gap):
    bv, bf, fv, _ff, _raw = chain_case()
    rng = np.random.default_rng(40 + int(gap))
    base = rng.integers(0, 256, size=(len(bf), 4)).astype(np.uint8)
    base[:, 3] = 255
    fcol = rng.random((len(fv), 3)).astype(np.float32)
    for a in (base, fcol):
        a.setflags(write=False)
    return base, fcol


@pytest.mark.parametrize("gap", [False, True])
def test_update_with_colours(gap):
    from gaustar_amd import regions
    bv, bf, fv, ff0, raw = chain_case()
    want, ff = origin_want(gap)
    base, fcol = _colours(gap)
    got = regions.update_mesh_topology(_t(bv), _t(bf), _regions_of(raw), _Mesh(fv, ff))
    plain = chain_want() if not gap else splice_ref.update_mesh_topology(bv, bf, 2, rr.padded_boxes(raw, 0.02), fv, ff)
    _check_update(got, plain, len(bf))                                  # what the call returns today
    assert got.face_origin.dtype == torch.int32 and np.array_equal(_n(got.face_origin), want["face_origin"])
    assert int((got.face_origin == -2 ** 31).sum()) == want["n_fills_made"] and (want["n_fills_made"] > 0) == gap
    assert np.array_equal(_n(got.face_origin[:got.track_face_num]), np.nonzero(_n(got.track_face_mask))[0])
    assert got.face_colors is None and got.vertex_colors is None
    faces_before, verts_before = got.faces.clone(), got.verts.clone()
    assert got.with_colors(_t(base), _t(fcol)) is got
    fc, vc = ref.with_colors(want, base, ff, fcol)
    assert got.face_colors.dtype == torch.uint8 and got.vertex_colors.dtype == torch.uint8
    assert np.array_equal(_n(got.face_colors), fc) and np.array_equal(_n(got.vertex_colors), vc)
    assert tuple(got.vertex_colors.shape) == (int(got.verts.shape[0]), 4) and bool((got.vertex_colors[:, 3] == 255).all())
    assert torch.equal(got.faces, faces_before) and torch.equal(got.verts, verts_before)
    with pytest.raises(ValueError):
        got.with_colors(_t(base[:-1]), _t(fcol))
    with pytest.raises(ValueError):
        got.with_colors(_t(base), _t(fcol[:-1]))


def test_nothing_to_update_and_failed_boxes_with_colours():
    from gaustar_amd import regions
    bv, bf, fv, ff, _raw = chain_case()
    base, fcol = _colours(False)
    want_vc = ref.face_to_vertex_colors(bf, base, len(bv))
    none = regions.update_mesh_topology(_t(bv), _t(bf), _regions_of(np.zeros((0, 2, 3))), _Mesh(fv, ff))
    far = regions.update_mesh_topology(_t(bv), _t(bf), _regions_of(np.array([[[5, 5, 5], [6, 6, 6]]], np.float64)), _Mesh(fv, ff))
    assert none.nothing_to_update and none.cc_update_num == -1 and none.new_ref_area is None
    assert far.cc_update_num == 0 and far.n_spliced == 0 and torch.equal(far.faces, _t(bf))
    for out in (none, far):
        assert np.array_equal(_n(out.face_origin), np.arange(len(bf))) and bool(out.track_face_mask.all())
        out.with_colors(_t(base), _t(fcol))
        assert np.array_equal(_n(out.face_colors), base) and np.array_equal(_n(out.vertex_colors), want_vc)


# ---------------------------------------------------------------------------------------------------- one hand-over, end to end
def test_hand_over_end_to_end(tmp_path):
    from gaustar_amd import formats, harness, regions, scene
    bv, bf, fv, ff, raw = chain_case()
    ff = np.delete(ff, GAP_FACE, axis=0)
    G, levels = 3, 2
    old = harness.SurfaceGaussians(_t(bv), _t(bf, torch.long), n_gaussians_per_surface_triangle=G, sh_levels=levels).to(DEV)
    gen = torch.Generator().manual_seed(6)
    with torch.no_grad():
        old._sh_coordinates_dc.copy_((torch.rand(old.n_points, 1, 3, generator=gen) * 4 - 2).to(DEV))
        old._sh_coordinates_rest.copy_((torch.randn(old.n_points, levels ** 2 - 1, 3, generator=gen) * 0.1).to(DEV))
    # 1. the colour mesh of the old model
    v, f, rgba = old.color_mesh()
    want_rgba = ref.sh_face_colors(_n(old._sh_coordinates_dc.detach()).reshape(-1, 3), G)
    assert np.array_equal(_n(rgba), want_rgba) and torch.equal(v, old._points.detach()) and torch.equal(f, old._surface_mesh_faces)
    # 2. the update, with hand-made regions, carrying colour
    sel = _regions_of(raw)
    old.topology_update_regions = lambda res, **kw: sel
    fusion = _Mesh(fv, ff)
    fusion.colors = _t(_colours(True)[1])
    assert old.update_mesh_topology(None, fusion, aabb_pad=0.02).vertex_colors is None             # the default: as today
    upd = old.update_mesh_topology(None, fusion, aabb_pad=0.02, colors=True)
    want, _ff = origin_want(True)
    fc, vc = ref.with_colors(want, want_rgba, ff, _colours(True)[1])
    assert np.array_equal(_n(upd.face_colors), fc) and np.array_equal(_n(upd.vertex_colors), vc)
    # 3. the files, and the next model from them
    obj, npz = upd.save(str(tmp_path))
    fv2, ff2, fc2 = formats.load_obj(obj)
    assert fc2.shape == (len(fv2), 3) and np.array_equal(ref.unit_to_u8(fc2), vc[:, :3])
    new = harness.SurfaceGaussians.from_mesh(fv2, ff2, fc2, n_gaussians_per_surface_triangle=G, sh_levels=levels)
    # 4. its SH dc is the restatement's on the file's contents, its densities inverse_sigmoid(0.1)
    made = ref.from_mesh(ff2, fc2, G)
    assert new.n_points == len(ff2) * G and new._sh_coordinates_dc.requires_grad
    assert _n(new._sh_coordinates_dc.detach()).reshape(-1, 3).tobytes() == made["sh_dc"].tobytes()
    x = torch.full((1,), 0.1, dtype=torch.float32)
    dens = _n(new.all_densities.detach())
    assert dens.shape == (new.n_points, 1) and (dens == torch.log(x / (1 - x)).numpy()).all() and (dens == made["density"]).all()
    assert not _n(new._sh_coordinates_rest.detach()).any()
    assert _n(new._points.detach()).tobytes() == fv2.astype(np.float32).tobytes() and np.array_equal(_n(new._surface_mesh_faces), ff2)
    with pytest.raises(ValueError):
        harness.SurfaceGaussians.from_mesh(fv2, ff2, None)
    with pytest.raises(ValueError):
        harness.SurfaceGaussians.from_mesh(fv2, ff2, fc2[:-1])
    # 5. the new model's own colour mesh reloads with V colours
    path = str(tmp_path / "color_mesh.obj")
    new.save_color_mesh(path)
    cv, cf, cc = formats.load_obj(path)
    assert np.array_equal(cf, ff2) and cv.astype(np.float32).tobytes() == fv2.astype(np.float32).tobytes()
    want_cc = ref.face_to_vertex_colors(ff2, ref.sh_face_colors(made["sh_dc"], G), len(fv2))
    assert cc.shape == (len(fv2), 3) and np.array_equal(cc, want_cc[:, :3].astype(np.float64) / 255.0)
    # 6. the tracked prefix of the old model's SH
    mask, ref_area = regions.load_tracking(npz)
    assert np.array_equal(mask, _n(upd.track_face_mask)) and np.array_equal(ref_area, _n(upd.new_ref_area))
    pre_dc, pre_sh = harness.tracked_pre_sh(old.state_dict(), upd.track_face_mask, G)
    gm = upd.gaussian_mask(G)
    assert tuple(pre_dc.shape) == (upd.track_face_num * G, 3) and tuple(pre_sh.shape) == (upd.track_face_num * G, levels ** 2, 3)
    assert torch.equal(pre_dc, old._sh_coordinates_dc.detach()[gm][:, 0])
    assert torch.equal(pre_sh, torch.cat([old._sh_coordinates_dc, old._sh_coordinates_rest], dim=1).detach()[gm])
    pre_np = harness.tracked_pre_sh({"state_dict": old.state_dict()}, mask, G)[0]
    assert torch.equal(pre_np, pre_dc)
    # 7. one refinement step of the new model, held to the old colours
    W, H = 64, 48
    cam = harness.nerf_camera_from_scene(scene.look_at_camera((0.0, 0.12, 0.45), (0.0, 0.0, 0.0), W, H, focal_px=150.0))
    bg4 = torch.tensor([0.0, 1.0, 0.0, 10.0], device=DEV)
    gdev = torch.Generator(device=DEV).manual_seed(7)
    gt_rgb = torch.rand(3, H, W, device=DEV, generator=gdev)
    # (depths on both sides of max_depth, as in tests/test_gpu_iteration.py: the depth loss takes a mean over {gt < max_depth}
    # and one over {gt > max_depth}, and the mean over an empty set is NaN here as in the reference)
    gt_d = torch.rand(H, W, device=DEV, generator=gdev) * 12.0
    loss_plain, _img, _radii = new.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0)
    for p in new.parameters():
        p.grad = None
    loss, img, radii = new.rgbd_step(cam, bg4, gt_rgb, gt_d, 10.0, param_reg=dict(pre_sh_dc=pre_dc, min_opacity=None, sh_factor=1.0))
    assert tuple(img.shape) == (4, H, W) and bool(torch.isfinite(loss)) and int((radii > 0).sum()) > 0
    M = int(pre_dc.shape[0])
    sh_term = float(((pre_dc - new._sh_coordinates_dc.detach()[:M, 0]) ** 2).mean())
    assert sh_term > 0 and abs(float(loss) - float(loss_plain) - sh_term) <= 1e-4 * (abs(float(loss)) + sh_term)
    assert new._sh_coordinates_dc.grad is not None and bool(new._sh_coordinates_dc.grad[:M].abs().sum() > 0)
