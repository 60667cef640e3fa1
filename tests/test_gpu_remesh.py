"""gaustar_amd.remesh on the GPU against the numpy restatement tests/remesh_ref.py (itself pinned by tests/test_remesh.py).
Every output is an integer or an exactly defined float, so every comparison is exact: integers by value, floats by their bits.
No tolerances.  The shapes are the smallest that reach every branch: Cramer's rule and the three-candidate fallback, the cap
round, fixed boundaries, locked vertices, a stall, a fin, zero-area faces, attributes."""
import functools
import os

import numpy as np
import pytest
import torch

import remesh_ref as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _grid_locked():
    locked = np.zeros(81, bool)
    for j in (3, 4, 5):
        locked[j * 9 + 3:j * 9 + 6] = True
    return locked


def _colours(n):
    return np.random.default_rng(7).random((n, 3)).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _case(name):
    """(verts, faces, target, locked, attrs, closed)"""
    if name == "ico2_to_80":
        return (*R.icosphere(2), 80, None, (), True)
    if name == "bumpy3_to_320":
        return (*R.bumpy(3), 320, None, (), True)
    if name == "grid_to_32":
        return (*R.flat_grid(9, 0.5), 32, None, (), False)
    if name == "grid_locked_block":
        return (*R.flat_grid(9, 0.5), 32, _grid_locked(), (), False)
    if name == "tetrahedron_stall":
        return (*R.tetrahedron(), 2, None, (), True)
    if name == "fin":
        v, f, _fin = R.fin_mesh()
        return v, f, 40, None, (), False
    if name == "zero_area_and_sliver":
        return (*R.degenerate_mesh(), 100, None, (), True)
    if name == "target_at_least_F":
        return (*R.icosphere(1), 80, None, (), True)
    if name == "target_0_to_the_stall":
        return (*R.icosphere(1), 0, None, (), True)
    if name == "colour_attribute":
        v, f = R.icosphere(2)
        return v, f, 101, None, (_colours(len(v)),), True
    raise KeyError(name)


CASES = ["ico2_to_80", "bumpy3_to_320", "grid_to_32", "grid_locked_block", "tetrahedron_stall", "fin", "zero_area_and_sliver",
         "target_at_least_F", "target_0_to_the_stall", "colour_attribute"]


@functools.lru_cache(maxsize=None)
def _want(name):
    v, f, target, locked, attrs, _closed = _case(name)
    return R.simplify(v, f, target, locked, attrs)


@pytest.mark.parametrize("name", CASES)
def test_simplify_is_bit_equal_to_the_restatement(hip_lib, name):
    from gaustar_amd import regions, remesh
    v, f, target, locked, attrs, closed = _case(name)
    tv, tf = _t(v), _t(f)
    tl = None if locked is None else _t(locked)
    ta = tuple(_t(a) for a in attrs)
    got = remesh.simplify_mesh(tv, tf, target, tl, ta)
    want = _want(name)
    assert got.verts.dtype == torch.float32 and got.faces.dtype == torch.int32 and got.face_origin.dtype == torch.int32
    assert (got.n_rounds, got.stalled) == (want.n_rounds, want.stalled)
    assert np.array_equal(got.faces.cpu().numpy(), want.faces)
    assert np.array_equal(got.face_origin.cpu().numpy(), want.face_origin)
    assert _same_bits(got.verts.cpu().numpy(), want.verts)
    assert len(got.attrs) == len(want.attrs)
    for a, b in zip(got.attrs, want.attrs):
        assert _same_bits(a.cpu().numpy(), b)
    # the inputs are not modified, and a second call gives the same bits
    assert _same_bits(tv.cpu().numpy(), v) and np.array_equal(tf.cpu().numpy(), f)
    for a, b in zip(ta, attrs):
        assert _same_bits(a.cpu().numpy(), b)
    again = remesh.simplify_mesh(tv, tf, target, tl, ta)
    assert torch.equal(again.verts, got.verts) and torch.equal(again.faces, got.faces) and torch.equal(again.face_origin, got.face_origin)
    assert (again.n_rounds, again.stalled) == (got.n_rounds, got.stalled)
    for a, b in zip(again.attrs, got.attrs):
        assert torch.equal(a, b)
    if closed:
        assert regions.is_watertight(tf) and regions.is_watertight(got.faces)


def test_what_the_cases_reach(hip_lib):
    """The cases take the paths they are there for (read off the restatement, which the GPU equals bit for bit)."""
    assert _want("tetrahedron_stall").stalled and _want("tetrahedron_stall").n_rounds == 0
    assert _want("target_0_to_the_stall").stalled and _want("target_0_to_the_stall").n_rounds > 0
    assert _want("target_at_least_F").n_rounds == 0 and not _want("target_at_least_F").stalled
    assert _want("bumpy3_to_320").n_rounds > 10 and len(_want("bumpy3_to_320").faces) == 320
    assert len(_want("colour_attribute").faces) == 100                  # an odd distance to the target: target - 1
    grid = _want("grid_locked_block")
    v, _f, _t_, locked, _a, _c = _case("grid_locked_block")
    out = {tuple(p) for p in grid.verts.view(np.uint32).tolist()}
    assert all(tuple(p.view(np.uint32).tolist()) in out for p in v[locked])
    assert not _same_bits(grid.faces, _want("grid_to_32").faces)


def test_errors(hip_lib):
    from gaustar_amd import remesh
    v, f = R.icosphere(1)
    tv, tf = _t(v), _t(f)
    with pytest.raises(ValueError):
        remesh.simplify_mesh(tv, tf, -1)
    bad = f.copy()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError):
        remesh.simplify_mesh(tv, _t(bad), 10)
    with pytest.raises(ValueError):
        remesh.simplify_mesh(tv, tf, 10, attrs=(torch.zeros(len(v), 3, dtype=torch.int32, device=DEV),))
    with pytest.raises(ValueError):
        remesh.simplify_mesh(tv, tf, 10, locked=torch.zeros(3, dtype=torch.bool, device=DEV))
    with pytest.raises(ValueError):
        remesh.smooth_laplacian(tv, tf, weights="cotangent")
    with pytest.raises(ValueError):
        remesh.smooth_laplacian(tv, _t(bad))


# ------------------------------------------------------------------------------------------------ smoothing
def _noisy_with_extras():
    v, f = R.noisy_sphere(2, seed=3)
    v = np.concatenate([v, np.asarray([[2.0, 2.0, 2.0]], np.float32)])       # an isolated vertex
    locked = np.zeros(len(v), bool)
    locked[5] = True
    return v, f, locked


@pytest.mark.parametrize("weights", ["inverse_distance", "uniform"])
@pytest.mark.parametrize("kind", ["laplacian", "taubin"])
def test_smoothing_is_bit_equal_to_the_restatement(hip_lib, kind, weights):
    from gaustar_amd import remesh
    v, f, locked = _noisy_with_extras()
    tv, tf, tl = _t(v), _t(f), _t(locked)
    if kind == "laplacian":
        got = remesh.smooth_laplacian(tv, tf, iterations=10, lambda_filter=0.5, weights=weights, locked=tl)
        want = R.smooth(v, f, 10, (0.5, 0.5), weights, locked)
    else:
        got = remesh.smooth_taubin(tv, tf, iterations=10, lambda_filter=0.5, mu=-0.53, weights=weights, locked=tl)
        want = R.smooth(v, f, 20, (0.5, -0.53), weights, locked)
    assert got.dtype == torch.float32 and _same_bits(got.cpu().numpy(), want)
    assert _same_bits(got[-1].cpu().numpy(), v[-1]) and _same_bits(got[5].cpu().numpy(), v[5])
    assert _same_bits(tv.cpu().numpy(), v)
    if kind == "laplacian":
        assert torch.equal(remesh.smooth_laplacian(tv, tf, iterations=0), tv)
        assert torch.equal(remesh.smooth_laplacian(tv, tf, 10, 0.5, weights, tl), got)


# ------------------------------------------------------------------------------------------------ the fusion route
@pytest.fixture(scope="module")
def fused(hip_lib):
    from test_gpu_fusion import _cams, _model
    model, cams = _model(5), _cams()
    kw = dict(voxel_size=0.03, sdf_trunc=0.075)
    return model, cams, kw, model.extract_mesh_fusion(cams, **kw)


def test_fusion_route_defaults_and_simplify(fused):
    from gaustar_amd import fusion, remesh
    model, cams, kw, base = fused
    N = int(base.faces.shape[0])
    assert N > 1000
    same = fusion.fuse_mesh(model, cams, smooth_iterations=0, simplify_face_num=0, **kw)
    assert torch.equal(same.verts, base.verts) and torch.equal(same.faces, base.faces) and torch.equal(same.colors, base.colors)
    got = model.extract_mesh_fusion(cams, simplify_face_num=N // 2, **kw)
    want = remesh.simplify_mesh(base.verts, base.faces, N // 2, attrs=(base.colors,))
    assert int(got.faces.shape[0]) <= N // 2 and not want.stalled
    assert torch.equal(got.verts, want.verts) and torch.equal(got.faces, want.faces) and torch.equal(got.colors, want.attrs[0])
    assert got.colors.shape == (got.verts.shape[0], 3)


def test_fusion_route_smooth(fused):
    from gaustar_amd import remesh
    model, cams, kw, base = fused
    got = model.extract_mesh_fusion(cams, smooth_iterations=3, **kw)
    want = remesh.smooth_laplacian(base.verts, base.faces, iterations=3)
    assert torch.equal(got.verts, want) and torch.equal(got.faces, base.faces) and torch.equal(got.colors, base.colors)
    assert not torch.equal(got.verts, base.verts)
    with pytest.raises(ValueError):
        model.extract_mesh_fusion(cams, simplify_face_num=-1, **kw)


# ------------------------------------------------------------------------------------------------ the command line
def test_cli_round_trip(hip_lib, tmp_path, capsys):
    from gaustar_amd import formats, remesh
    v, f = R.bumpy(2)
    col = _colours(len(v))
    src, dst = os.path.join(tmp_path, "in.obj"), os.path.join(tmp_path, "out.obj")
    formats.save_obj(src, v, f, col)
    assert remesh.main([src, dst, "--faces", "120"]) == 0
    assert "120 faces" in capsys.readouterr().out
    want = remesh.simplify_mesh(_t(v), _t(f), 120, attrs=(_t(col),))
    ov, of, oc = formats.load_obj(dst)
    assert _same_bits(ov.astype(np.float32), want.verts.cpu().numpy())
    assert np.array_equal(of, want.faces.cpu().numpy())
    assert _same_bits(oc.astype(np.float32), want.attrs[0].cpu().numpy())
    # with smoothing in front, and without colours
    formats.save_obj(src, v, f)
    assert remesh.main([src, dst, "--faces", "120", "--smooth", "2", "--taubin", "1"]) == 0
    sv = remesh.smooth_taubin(remesh.smooth_laplacian(_t(v), _t(f), iterations=2), _t(f), iterations=1)
    want = remesh.simplify_mesh(sv, _t(f), 120)
    ov, of, oc = formats.load_obj(dst)
    assert oc is None or oc.shape[1] == 0
    assert _same_bits(ov.astype(np.float32), want.verts.cpu().numpy()) and np.array_equal(of, want.faces.cpu().numpy())
