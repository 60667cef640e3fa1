"""gaustar_amd.edit without a GPU: the C entry points' argument checks, the Python layer's ValueErrors before any launch, the SH
rotation matrices' group properties, and the numpy restatement tests/edit_ref.py against closed forms.
tests/test_gpu_edit.py compares the kernels with the same restatement bit for bit."""
import ctypes

import numpy as np
import pytest
import torch

import edit_ref as ref
from gaustar_amd import _lib, edit, formats, harness, scene

EPS = 2.0 ** -52
BAND_COND = (1.0, 1.02, 1.05, 1.14)          # Y_l at the 32 directions: measured once, recorded in edit.sh_rotation_matrices


# ------------------------------------------------------------------------------------------------ the C ABI
def test_entry_points_reject_bad_arguments_before_any_device_work(hip_lib):
    lib, null = hip_lib, None
    msg = lambda: lib.gsr_last_error() or b""
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    dp = ctypes.cast(buf, ctypes.POINTER(ctypes.c_double))
    assert lib.gsr_abi_version() == 16 and _lib.ABI_VERSION == 16
    # fit_sums
    assert lib.gsr_edit_fit_workspace_bytes(3, 1025) >= 3 * 5 * 5 * 4 * 8 and lib.gsr_edit_fit_workspace_bytes(0, 0) > 0
    assert lib.gsr_edit_fit_sums(-1, 4, p, p, p, p, null, null) != 0 and b"negative" in msg()
    assert lib.gsr_edit_fit_sums(1, 0, p, p, p, p, null, null) != 0 and b"no anchors" in msg()
    assert lib.gsr_edit_fit_sums(70000, 4, p, p, p, p, null, null) != 0 and b"65535" in msg()
    for i in range(4):
        args = [p] * 4
        args[i] = null
        assert lib.gsr_edit_fit_sums(1, 4, *args, null, null) != 0 and b"null" in msg(), i
    assert lib.gsr_edit_fit_sums(0, 4, null, null, null, null, null, null) == 0
    # transform_points
    assert lib.gsr_edit_transform_points(-1, 3, 0, p, dp, dp, null, null) != 0 and b"negative" in msg()
    assert lib.gsr_edit_transform_points(4, 2, 0, p, dp, dp, null, null) != 0 and b"columns" in msg()
    assert lib.gsr_edit_transform_points(4, 4, 2, p, dp, dp, null, null) != 0 and b"columns" in msg()
    assert lib.gsr_edit_transform_points(4, 3, 0, null, dp, dp, null, null) != 0 and b"null" in msg()
    assert lib.gsr_edit_transform_points(4, 3, 0, p, None, dp, null, null) != 0 and b"null" in msg()
    assert lib.gsr_edit_transform_points(0, 3, 0, null, dp, None, null, null) == 0
    # rotate_sh
    assert lib.gsr_edit_rotate_sh(-1, 16, p, p, p, null, null) != 0 and b"negative" in msg()
    assert lib.gsr_edit_rotate_sh(4, 1, p, p, p, null, null) != 0 and b"M must be" in msg()
    assert lib.gsr_edit_rotate_sh(4, 25, p, p, p, null, null) != 0 and b"M must be" in msg()
    for i in range(3):
        args = [p] * 3
        args[i] = null
        assert lib.gsr_edit_rotate_sh(4, 16, *args, null, null) != 0 and b"null" in msg(), i
    off = ctypes.c_void_p(p.value + 4)
    assert lib.gsr_edit_rotate_sh(4, 16, p, off, p, null, null) != 0 and b"aligned" in msg()
    assert lib.gsr_edit_rotate_sh(0, 16, null, null, null, null, null) == 0
    # faces_in_halfspaces
    sizes = lambda *s: (ctypes.c_int * len(s))(*s)
    hs = lambda F=4, V=4, faces=p, verts=p, n=1, gs=sizes(2), planes=dp, mask=p, err=p: \
        lib.gsr_edit_faces_in_halfspaces(F, V, faces, verts, n, gs, planes, mask, err, null)
    assert hs(F=-1) != 0 and b"negative" in msg()
    assert hs(n=0) != 0 and b"groups" in msg()
    assert hs(n=17, gs=sizes(*[1] * 17)) != 0 and b"groups" in msg()
    assert hs(gs=sizes(0)) != 0 and b"plane" in msg()
    assert hs(n=2, gs=sizes(40, 25)) != 0 and b"64 planes" in msg()
    for missing in ("faces", "mask", "err", "verts", "planes", "gs"):
        assert hs(**{missing: None}) != 0 and b"null" in msg(), missing
    assert hs(F=0, faces=None, mask=None, err=None) == 0
    # gather_rows
    ptrs = lambda *v: (ctypes.c_void_p * len(v))(*v)
    gr = lambda n=4, F=8, kept=p, G=6, k=1, src=ptrs(p.value), dst=ptrs(p.value), words=sizes(3), err=p: \
        lib.gsr_edit_gather_rows(n, F, kept, G, k, src, dst, words, err, null)
    assert gr(n=-1) != 0 and b"negative" in msg()
    assert gr(G=0) != 0 and b"G must be" in msg()
    assert gr(k=0) != 0 and b"tables" in msg()
    assert gr(k=9) != 0 and b"tables" in msg()
    assert gr(words=sizes(0)) != 0 and b"row width" in msg()
    for missing in ("kept", "err", "src", "dst", "words"):
        assert gr(**{missing: None}) != 0 and b"null" in msg(), missing
    assert gr(src=ptrs(None)) != 0 and b"null" in msg()
    assert gr(n=0, kept=None, err=None) == 0
    # paint
    def paint(N=12, G=6, F=2, V=4, faces=p, verts=p, bary=p, n_tri=2, tri=p, h=5, w=7, C=1, tex=p, mode=0, shrink=1, scales=p, dc=p,
              stats=p, err=p):
        return lib.gsr_edit_paint(N, G, F, V, faces, verts, bary, n_tri, tri, h, w, C, tex, mode, 0.03, 0.05, shrink, -6.0, 50, scales, dc,
                                  stats, err, null)
    assert paint(N=-1) != 0 and b"negative" in msg()
    assert paint(G=0) != 0 and b"G must be" in msg()
    assert paint(n_tri=0) != 0 and b"triangles" in msg()
    assert paint(n_tri=65) != 0 and b"triangles" in msg()
    assert paint(h=0) != 0 and b"size" in msg()
    assert paint(C=2) != 0 and b"channels" in msg()
    assert paint(mode=2) != 0 and b"mode" in msg()
    assert paint(mode=1, C=1) != 0 and b"replace" in msg()
    for missing in ("faces", "verts", "bary", "tri", "tex", "scales", "dc", "stats", "err"):
        assert paint(**{missing: None}) != 0 and b"null" in msg(), missing


# ------------------------------------------------------------------------------------------------ the Python layer
def _cpu_model(level=1, G=6, sh_levels=2, **kw):
    v, f = scene.icosphere(level)
    return harness.SurfaceGaussians(torch.from_numpy(v), torch.from_numpy(f), n_gaussians_per_surface_triangle=G, sh_levels=sh_levels, **kw)


def test_value_errors_come_before_any_launch():
    m = _cpu_model()
    F = int(m._surface_mesh_faces.shape[0])
    quad = np.array([[0, 0, 1], [1, 0, 1], [0, 1, 1], [1, 1, 1]], np.float64)
    uv = np.array([[0.1, 0.1], [0.1, 0.9], [0.9, 0.1], [0.9, 0.9]])
    tris = [[0, 1, 2], [1, 2, 3]]
    tex = np.zeros((5, 7), np.uint8)
    # fit_rigid
    with pytest.raises(ValueError, match="float64"):
        edit.fit_rigid(quad.astype(np.float32), quad)
    with pytest.raises(ValueError, match=r"\[K,3\]"):
        edit.fit_rigid(quad[:, :2], quad)
    with pytest.raises(ValueError, match="dst must be"):
        edit.fit_rigid(quad, quad[None, :3])
    with pytest.raises(ValueError, match="anchors"):
        edit.fit_rigid(quad[:0], quad[:0])
    with pytest.raises(ValueError, match="GPU"):
        edit.fit_rigid(quad, quad, device="cpu")
    # transform_model / sh_rotation_matrices
    with pytest.raises(ValueError, match="SurfaceGaussians"):
        edit.transform_model(object(), np.eye(3), np.zeros(3))
    with pytest.raises(ValueError, match="GPU"):
        edit.transform_model(m, np.eye(3), np.zeros(3))
    with pytest.raises(ValueError, match=r"R must be \[3,3\]"):
        edit.sh_rotation_matrices(np.eye(4), 4)
    with pytest.raises(ValueError, match="rotation"):
        edit.sh_rotation_matrices(np.diag([1.0, 1.0, -1.0]), 4)
    with pytest.raises(ValueError, match="rotation"):
        edit.sh_rotation_matrices(2.0 * np.eye(3), 4)
    with pytest.raises(ValueError, match="sh_levels"):
        edit.sh_rotation_matrices(np.eye(3), 5)
    with pytest.raises(ValueError, match="GPU"):
        edit.rotate_sh_rest(torch.zeros(4, 15, 3), np.eye(16))
    # faces_in_halfspaces
    one = np.array([[1.0, 0.0, 0.0, 0.0]])
    verts, faces = m._points.detach(), m._surface_mesh_faces
    with pytest.raises(ValueError, match="64 planes"):
        edit.faces_in_halfspaces(verts, faces, [np.tile(one, (33, 1)), np.tile(one, (32, 1))])
    with pytest.raises(ValueError, match="16 groups"):
        edit.faces_in_halfspaces(verts, faces, [one] * 17)
    with pytest.raises(ValueError, match="16 groups"):
        edit.faces_in_halfspaces(verts, faces, [])
    with pytest.raises(ValueError, match="at least one plane"):
        edit.faces_in_halfspaces(verts, faces, [one[:0]])
    with pytest.raises(ValueError, match=r"\[n,4\]"):
        edit.faces_in_halfspaces(verts, faces, [one[:, :3]])
    with pytest.raises(ValueError, match="float64"):
        edit.faces_in_halfspaces(verts, faces, [one.astype(np.float32)])
    with pytest.raises(ValueError, match="one GPU"):
        edit.faces_in_halfspaces(verts, faces, [one])
    # cut_model
    with pytest.raises(ValueError, match="keep_faces"):
        edit.cut_model(m, torch.ones(F + 1, dtype=torch.bool))
    with pytest.raises(ValueError, match="keep_faces"):
        edit.cut_model(m, torch.ones(F, dtype=torch.float32))
    with pytest.raises(ValueError, match="GPU"):
        edit.cut_model(m, torch.ones(F, dtype=torch.bool))
    # merge_models
    for other, what in ((_cpu_model(G=1), "n_gaussians_per_surface_triangle"), (_cpu_model(sh_levels=3), "sh_levels"),
                        (_cpu_model(surface_mesh_thickness=1e-3), "thickness"), (_cpu_model(loose_bind=True), "loose")):
        with pytest.raises(ValueError, match=what):
            edit.merge_models(m, other)
    with pytest.raises(ValueError, match="GPU"):
        edit.merge_models(m, _cpu_model())
    # paint_decal
    with pytest.raises(ValueError, match="64 triangles"):
        edit.paint_decal(m, quad, uv, [[0, 1, 2]] * 65, tex)
    with pytest.raises(ValueError, match="64 triangles"):
        edit.paint_decal(m, quad, uv, np.zeros((0, 3), np.int64), tex)
    with pytest.raises(ValueError, match="outside"):
        edit.paint_decal(m, quad, uv, [[0, 1, 4]], tex)
    with pytest.raises(ValueError, match="integers"):
        edit.paint_decal(m, quad, uv, np.array(tris, np.float64), tex)
    with pytest.raises(ValueError, match="uv"):
        edit.paint_decal(m, quad, uv[:3], tris, tex)
    with pytest.raises(ValueError, match="anchors"):
        edit.paint_decal(m, quad.astype(np.float32), uv, tris, tex)
    with pytest.raises(ValueError, match="uint8"):
        edit.paint_decal(m, quad, uv, tris, tex.astype(np.float32))
    with pytest.raises(ValueError, match="C = 1, 3 or 4"):
        edit.paint_decal(m, quad, uv, tris, np.zeros((5, 7, 2), np.uint8))
    with pytest.raises(ValueError, match="mode"):
        edit.paint_decal(m, quad, uv, tris, tex, mode="add")
    with pytest.raises(ValueError, match="replace needs"):
        edit.paint_decal(m, quad, uv, tris, tex, mode="replace")
    with pytest.raises(ValueError, match="GPU"):
        edit.paint_decal(m, quad, uv, tris, tex)
    # the ops check what they are built from
    with pytest.raises(ValueError, match="64 planes"):
        edit.CutOp([np.tile(one, (65, 1))])
    with pytest.raises(ValueError, match="GPU"):
        edit.AttachOp(m, quad)
    with pytest.raises(ValueError, match="not among the tracked"):
        edit._frame_anchors({"face_trajectory": np.zeros((3, 4, 3)), "frames": np.array([10, 16, 2])}, [10, 13])
    got = edit._frame_anchors({"face_trajectory": np.arange(36.0).reshape(3, 4, 3), "frames": np.array([10, 16, 2])}, [14, 10])
    assert np.array_equal(got, np.arange(36.0).reshape(3, 4, 3)[[2, 0]])


def test_the_model_has_the_thin_methods():
    for name in ("cut", "merged_with", "transform", "paint_decal"):
        assert callable(getattr(harness.SurfaceGaussians, name))
    for name in edit.__all__:
        assert hasattr(edit, name)


# ------------------------------------------------------------------------------------------------ SH rotation matrices
@pytest.mark.parametrize("levels", [1, 2, 3, 4])
def test_sh_rotation_matrices_form_a_representation(levels):
    """D(R) D(R)^T = I and D(R1 R2) = D(R1) D(R2) to 1e-12: eps times the bands' condition numbers (at most 1.14) with three
    orders of slack.  The identity gives the identity to 1e-14."""
    assert EPS * max(BAND_COND) * 1e3 < 1e-12
    rng = np.random.default_rng(5)
    M = levels * levels
    for _ in range(4):
        R1, R2 = ref.rotation(rng), ref.rotation(rng)
        D1, D2, D12 = (edit.sh_rotation_matrices(R, levels) for R in (R1, R2, R1 @ R2))
        assert D1.shape == (M, M) and D1.dtype == np.float64
        assert np.array_equal(D1, ref.sh_rotation_matrices(R1, levels))
        block = np.zeros((M, M), bool)
        for l in range(levels):
            block[l * l:(l + 1) ** 2, l * l:(l + 1) ** 2] = True
        assert (D1[~block] == 0).all()
        print(levels, np.abs(D1 @ D1.T - np.eye(M)).max(), np.abs(D12 - D1 @ D2).max())
        assert np.abs(D1 @ D1.T - np.eye(M)).max() < 1e-12
        assert np.abs(D12 - D1 @ D2).max() < 1e-12
    assert np.abs(edit.sh_rotation_matrices(np.eye(3), levels) - np.eye(M)).max() < 1e-14


def test_sh_basis_is_the_one_the_renderer_evaluates():
    """scene.eval_sh_rgb (spherical_harmonics.py:134-160) of coefficients c is basis @ c + 0.5, and the rotated coefficients
    give at d what the originals give at R^T d."""
    rng = np.random.default_rng(6)
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    c = rng.normal(size=(64, 16, 3)) * 0.2
    Y = edit.sh_basis(d, 4)
    assert np.array_equal(Y, ref.sh_basis(d, 4))
    got = np.einsum("nm,nmc->nc", Y, c) + 0.5
    want = scene.eval_sh_rgb(3, c, d)
    live = want > 0
    assert np.abs(got - want)[live].max() < 1e-6
    cond = [np.linalg.cond(edit.sh_basis(edit.fibonacci_sphere(32), 4)[:, l * l:(l + 1) ** 2]) for l in range(4)]
    assert np.allclose(cond, BAND_COND, atol=0.006)
    R = ref.rotation(rng)
    D = edit.sh_rotation_matrices(R, 4)
    c1 = c[0, :, 0]
    assert np.abs(edit.sh_basis(d, 4) @ (D @ c1) - edit.sh_basis(d @ R, 4) @ c1).max() < 1e-13


def test_rotate_sh_restatement_is_the_matrix_product():
    rng = np.random.default_rng(7)
    rest = rng.normal(size=(9, 15, 3)).astype(np.float32)
    D = ref.sh_rotation_matrices(ref.rotation(rng), 4)
    got = ref.rotate_sh(rest, D)
    want = np.einsum("ik,nkc->nic", D[1:, 1:], rest.astype(np.float64))
    assert got.dtype == np.float32 and np.abs(got - want).max() < 1e-6
    assert np.array_equal(ref.rotate_sh(rest, np.eye(16)), rest)


# ------------------------------------------------------------------------------------------------ the restatement, closed forms
QUAD = np.array([[-0.4, -0.3, 0.0], [0.5, -0.35, 0.0], [-0.45, 0.4, 0.0], [0.55, 0.5, 0.0]])      # coplanar


def test_fit_recovers_a_known_motion_and_takes_both_reflection_branches():
    """A coplanar quad leaves H of rank 2: the SVD's third pair of vectors is free in sign, and det(Vt^T U^T) < 0 happens for
    about a quarter of the seeds.  Either way the fit is the motion."""
    flips = []
    for seed in range(16):
        rng = np.random.default_rng(seed)
        R0, t0 = ref.rotation(rng), rng.normal(size=3)
        dst = QUAD @ R0.T + t0
        R, t, n, ok, flipped = ref.fit_rigid(QUAD, dst)
        assert ok[0] and n[0] == 4
        assert np.abs(R[0] - R0).max() < 1e-14 and np.abs(t[0] - t0).max() < 1e-14
        assert abs(np.linalg.det(R[0]) - 1) < 1e-14
        mine = edit.rigid_from_sums(_sums(QUAD, dst))
        assert np.array_equal(mine.R[0], R[0]) and np.array_equal(mine.t[0], t[0]) and mine.ok[0] and mine.n[0] == 4
        flips.append(bool(flipped[0]))
    print("reflection branch:", flips)
    assert any(flips) and not all(flips)


def _sums(src, dst):
    n, abar, bbar, _, _ = ref.fit_centroids(src, dst)
    H = ref.fit_cross(src, dst, abar, bbar)[0]
    return np.concatenate([[n], abar, bbar, H.reshape(-1)])[None]


def test_fit_skips_lost_points_and_refuses_collinear_ones():
    rng = np.random.default_rng(3)
    R0, t0 = ref.rotation(rng), rng.normal(size=3)
    src = rng.normal(size=(7, 3))
    dst = np.stack([src @ R0.T + t0] * 3)
    dst[1, 2] = np.nan                                         # one lost point: the fit goes on without it
    dst[2, :5, 0] = np.nan                                     # five lost: two are left
    R, t, n, ok, _ = ref.fit_rigid(src, dst)
    assert n.tolist() == [7, 6, 2] and ok.tolist() == [True, True, False]
    assert np.abs(R[:2] - R0).max() < 1e-14 and np.isnan(R[2]).all() and np.isnan(t[2]).all()
    line = np.outer(np.linspace(-1, 1, 5), [0.3, -0.2, 0.9]) + 0.1
    R, t, n, ok, _ = ref.fit_rigid(line, line @ R0.T + t0)
    assert n[0] == 5 and not ok[0] and np.isnan(R[0]).all()
    mine = edit.rigid_from_sums(_sums(line, line @ R0.T + t0))
    assert not mine.ok[0] and np.isnan(mine.R[0]).all()


def test_transform_and_selection_restatements():
    rng = np.random.default_rng(4)
    x = rng.normal(size=(11, 3)).astype(np.float32)
    R, t = ref.rotation(rng), rng.normal(size=3)
    assert np.abs(ref.transform_points(x, R, t) - (x.astype(np.float64) @ R.T + t)).max() < 1e-6
    assert np.array_equal(ref.transform_points(x, np.eye(3)), x)
    q = rng.normal(size=(5, 4)).astype(np.float32)
    assert np.array_equal(ref.transform_delta_r(q, R)[:, 0], q[:, 0])
    v, f = scene.icosphere(1)
    c = ref.face_centres(v, f)
    sel = ref.faces_in_halfspaces(v, f, [np.array([[1.0, 0, 0, -0.1], [0, -1.0, 0, 0]]), np.array([[0, 0, 1.0, -0.5]])])
    assert np.array_equal(sel, ((c[:, 0] > 0.1) & (c[:, 1] < 0)) | (c[:, 2] > 0.5))
    p = ref.plane_through(c[17], [0.3, -0.5, 0.8])
    assert not ref.faces_in_halfspaces(v, f, [p[None]])[17]


def test_cut_and_merge_restatements():
    v, f = scene.icosphere(1)
    G = 6
    params = {"a": np.arange(len(f) * G * 2, dtype=np.float32).reshape(-1, 2)}
    keep = np.zeros(len(f), bool)
    keep[[3, 4, 50]] = True
    cv, cf, cp = ref.cut(v, f, params, keep, G)
    assert np.array_equal(cv[cf], v[f[keep]]) and len(cv) == len(np.unique(f[keep]))
    assert np.array_equal(cp["a"][:G], params["a"][3 * G:4 * G]) and len(cp["a"]) == 3 * G
    mv, mf, mp = ref.merge(cv, cf, cp, v, f, params)
    assert np.array_equal(mv[mf[3:]], v[f]) and np.array_equal(mp["a"][3 * G:], params["a"])


def test_png_rgba_reader(tmp_path):
    a = np.random.default_rng(1).integers(0, 256, (6, 4, 4), dtype=np.uint8)
    path = str(tmp_path / "decal.png")
    formats._save_png8(path, a, 6)
    assert np.array_equal(formats.load_png_rgba8(path), a)
    formats.save_png_rgb8(path, a[:, :, :3])
    with pytest.raises(ValueError, match="RGBA"):
        formats.load_png_rgba8(path)
