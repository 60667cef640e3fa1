"""The editing kernels on the device (gsr_edit.hip behind gaustar_amd.edit) against their numpy restatement tests/edit_ref.py:
bit for bit, except the rigid fit's tree sums, which are held to the bound of a sum of m terms.  Meshes: scene.icosphere(1)
(80 faces) and (2) (320 faces) of radius 0.9 about (0.1, 1.2, -0.2), G in {1, 6}."""
import os

import numpy as np
import pytest
import torch

import edit_ref as ref
from gaustar_amd import edit, formats, harness, scene

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
CENTRE, RADIUS = (0.1, 1.2, -0.2), 0.9
PARAMS = ("_scales", "_quaternions", "all_densities", "_sh_coordinates_dc", "_sh_coordinates_rest")
DELTAS = ("_delta_t", "_delta_r")


def _model(level=1, G=6, sh_levels=2, loose=False, seed=0, centre=CENTRE):
    """A model with random parameters of O(1), so that every array is told apart from every other."""
    v, f = scene.icosphere(level, RADIUS, centre)
    m = harness.SurfaceGaussians(torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV), n_gaussians_per_surface_triangle=G,
                                 sh_levels=sh_levels, loose_bind=loose)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for k in (*PARAMS, *(DELTAS if loose else ())):
            p = getattr(m, k)
            p.copy_(torch.randn(p.shape, generator=gen).to(DEV))
    return m


def _np(m):
    """The model's arrays on the host: verts, faces, {name: array}."""
    names = (*PARAMS, *(DELTAS if getattr(m, "_delta_t", None) is not None else ()))
    return m._points.detach().cpu().numpy(), m._surface_mesh_faces.cpu().numpy(), {k: getattr(m, k).detach().cpu().numpy() for k in names}


def _same(a, b):
    """Bit equality of two float arrays (NaN patterns and signed zeros included)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ------------------------------------------------------------------------------------------------ 1. rigid fit
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("K", [3, 4, 255, 256, 257, 1025])         # one wave, a workgroup less one, one, one more, past four
def test_fit_sums(K, T):
    rng = np.random.default_rng(100 * K + T)
    src = rng.normal(size=(K, 3))
    Rs, ts = [ref.rotation(rng) for _ in range(T)], rng.normal(size=(T, 3))
    dst = np.stack([src @ R.T + t for R, t in zip(Rs, ts)])
    if K > 3:                                                      # lost points: a NaN row in a frame; beyond four anchors also
        dst[T - 1, K // 2] = np.nan                                # a single NaN coordinate, in a frame and in src
    if K > 4:
        dst[0, K - 1, 1] = np.nan
        src[1, 2] = np.nan
    sums = edit.fit_sums(src, dst if T > 1 else dst[0])
    assert sums.is_cuda and tuple(sums.shape) == (T, 16) and sums.dtype == torch.float64
    again = edit.fit_sums(torch.from_numpy(src).to(DEV), torch.from_numpy(dst).to(DEV))
    assert _same(sums.cpu().numpy(), again.cpu().numpy())          # a fixed-order reduction: the same bits
    got = sums.cpu().numpy()
    for t in range(T):
        n, abar, bbar, tol_a, tol_b = ref.fit_centroids(src, dst[t])
        assert got[t, 0] == n and n >= 3
        err_a, err_b = np.abs(got[t, 1:4] - abar), np.abs(got[t, 4:7] - bbar)
        H, tol_h = ref.fit_cross(src, dst[t], got[t, 1:4], got[t, 4:7])
        err_h = np.abs(got[t, 7:].reshape(3, 3) - H)
        print(f"K={K} t={t}: n={n} centroid err/tol {np.max(err_a / tol_a):.3f} {np.max(err_b / tol_b):.3f}  H err/tol {np.max(err_h / tol_h):.3f}")
        assert (err_a <= tol_a).all() and (err_b <= tol_b).all() and (err_h <= tol_h).all()
    fit = edit.fit_rigid(src, dst)
    R, t, n, ok, _ = ref.rigid_from_sums(got)
    assert _same(fit.R, R) and _same(fit.t, t) and np.array_equal(fit.n, n) and np.array_equal(fit.ok, ok) and ok.all()
    for i in range(T):                                             # (sums of <= 1025 terms of O(1) err by 1e-13: this catches wrong logic)
        assert np.abs(fit.R[i] - Rs[i]).max() < 1e-9 and np.abs(fit.t[i] - ts[i]).max() < 1e-9


def test_fit_of_collinear_and_of_too_few_anchors_is_not_ok():
    line = np.outer(np.linspace(-1, 1, 6), [0.3, -0.2, 0.9]) + 0.1
    few = np.array(line)
    few[:4] = np.nan
    fit = edit.fit_rigid(line, np.stack([line + 1.0, few]))
    assert fit.n.tolist() == [6, 2] and not fit.ok.any() and np.isnan(fit.R).all() and np.isnan(fit.t).all()


# ------------------------------------------------------------------------------------------------ 2. moving a model
@pytest.mark.parametrize("G,loose", [(1, False), (6, True)])
def test_transform_points_and_deltas(G, loose):
    m = _model(1, G, 1, loose)
    v0, f0, p0 = _np(m)
    rng = np.random.default_rng(11)
    R, t = ref.rotation(rng), rng.normal(size=3)
    assert m.transform(R, t, rotate_sh=False) is m
    v1, f1, p1 = _np(m)
    assert _same(v1, ref.transform_points(v0, R, t)) and np.array_equal(f0, f1)
    for k in PARAMS:
        assert _same(p1[k], p0[k]), k
    if loose:
        assert _same(p1["_delta_t"], ref.transform_points(p0["_delta_t"], R))
        assert _same(p1["_delta_r"], ref.transform_delta_r(p0["_delta_r"], R)) and _same(p1["_delta_r"][:, 0], p0["_delta_r"][:, 0])
    # the Gaussians ride along: the producer's centres of the moved model are the moved centres
    want = ref.gaussian_centres(v1, f1, G)
    if not loose:
        assert np.abs(m.points.detach().cpu().numpy() - want).max() < 1e-5


@pytest.mark.parametrize("levels", [2, 3, 4])
@pytest.mark.parametrize("N", [1, 63, 64, 65, 480])                # a workgroup takes 64 Gaussians
def test_rotate_sh(N, levels):
    rng = np.random.default_rng(1000 * levels + N)
    M = levels * levels
    rest = rng.normal(size=(N, M - 1, 3)).astype(np.float32)
    R = ref.rotation(rng)
    D = edit.sh_rotation_matrices(R, levels)
    want = ref.rotate_sh(rest, D)
    dev = torch.from_numpy(rest).to(DEV)
    got = edit.rotate_sh_rest(dev, D)
    assert _same(got.cpu().numpy(), want) and _same(dev.cpu().numpy(), rest)
    assert edit.rotate_sh_rest(dev, D, out=dev) is dev and _same(dev.cpu().numpy(), want)      # in place
    # the turned coefficients at d give what the originals give at R^T d: one f32 rounding per coefficient + the matrix's defect
    d = rng.normal(size=(64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    Y, Yr = ref.sh_basis(d, levels)[:, 1:], ref.sh_basis(d @ R, levels)[:, 1:]
    new = np.einsum("dm,nmc->ndc", Y, want.astype(np.float64))
    old = np.einsum("dm,nmc->ndc", Yr, rest.astype(np.float64))
    tol = 2.0 ** -23 * np.einsum("dm,nmc->ndc", np.abs(Y), np.abs(want).astype(np.float64)) + 1e-12
    print(f"N={N} levels={levels}: err/tol {np.max(np.abs(new - old) / tol):.3f}")
    assert (np.abs(new - old) <= tol).all()


@pytest.mark.parametrize("levels", [1, 4])
def test_transform_model_turns_the_sh(levels):
    m = _model(1, 6, levels)
    _, _, p0 = _np(m)
    R, t = ref.rotation(np.random.default_rng(12)), np.array([0.5, -0.25, 0.125])
    edit.transform_model(m, np.eye(3), t)                          # the identity: nothing launched for the SH, the bits stay
    assert _same(_np(m)[2]["_sh_coordinates_rest"], p0["_sh_coordinates_rest"])
    edit.transform_model(m, R, t)
    p1 = _np(m)[2]
    if levels == 1:
        assert p1["_sh_coordinates_rest"].shape[1] == 0
    else:
        assert _same(p1["_sh_coordinates_rest"], ref.rotate_sh(p0["_sh_coordinates_rest"], ref.sh_rotation_matrices(R, levels)))
        assert not _same(p1["_sh_coordinates_rest"], p0["_sh_coordinates_rest"])
    assert _same(p1["_sh_coordinates_dc"], p0["_sh_coordinates_dc"])


# ------------------------------------------------------------------------------------------------ 3. selecting and cutting
def _groups():
    cx, cy, cz = CENTRE
    return [np.array([[1.0, 0.0, 0.0, -(cx + 0.1 * RADIUS)], [0.0, -1.0, 0.0, cy]]),       # x > cx + 0.1 R and y < cy
            np.array([[0.0, 0.0, 1.0, -(cz + 0.5 * RADIUS)]])]                              # or z > cz + 0.5 R


@pytest.mark.parametrize("level,n_sel,n_both", [(1, 34, 4), (2, 133, 15)])     # (counted with the restatement, for this centre)
def test_faces_in_halfspaces(level, n_sel, n_both):
    v, f = scene.icosphere(level, RADIUS, CENTRE)
    verts, faces = torch.from_numpy(v).to(DEV), torch.from_numpy(f).to(DEV)
    groups = _groups()
    want = ref.faces_in_halfspaces(v, f, groups)
    both = ref.faces_in_halfspaces(v, f, groups[:1]) & ref.faces_in_halfspaces(v, f, groups[1:])
    assert want.sum() == n_sel and both.sum() == n_both
    got = edit.faces_in_halfspaces(verts, faces, groups)
    assert got.dtype == torch.bool and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    assert np.array_equal(edit.faces_in_halfspaces(verts, faces.int(), groups).cpu().numpy(), want)
    # strictly: a plane through a face's centre, its offset formed the kernel's way, leaves that face out
    c = ref.face_centres(v, f)
    for face, normal in ((17, [0.3, -0.5, 0.8]), (len(f) - 1, [-1.0, 0.25, 0.0])):
        plane = ref.plane_through(c[face], normal)
        sel = edit.faces_in_halfspaces(verts, faces, [plane[None]]).cpu().numpy()
        assert not sel[face] and np.array_equal(sel, ref.faces_in_halfspaces(v, f, [plane[None]])) and sel.any()
    bad = faces.clone()
    bad[5, 1] = len(v)
    with pytest.raises(ValueError, match="outside"):
        edit.faces_in_halfspaces(verts, bad, groups)


@pytest.mark.parametrize("level,G,loose", [(1, 1, False), (1, 6, True), (2, 6, False)])
def test_cut_model(level, G, loose):
    m = _model(level, G, 4, loose, seed=3)
    v, f, p = _np(m)
    keep = ref.faces_in_halfspaces(v, f, _groups())
    mask = torch.from_numpy(keep).to(DEV)
    part = m.cut(mask)
    cv, cf, cp = ref.cut(v, f, p, keep, G)
    gv, gf, gp = _np(part)
    assert _same(gv, cv) and np.array_equal(gf, cf) and set(gp) == set(cp)
    for k in cp:
        assert _same(gp[k], cp[k]), k
    assert part.is_loose_bind() == loose and part.sh_levels == 4 and part.n_gaussians_per_surface_triangle == G
    assert _same(_np(m)[0], v) and all(_same(_np(m)[2][k], p[k]) for k in p)                   # the source is left alone
    whole = edit.cut_model(m, torch.ones(len(f), dtype=torch.bool, device=DEV))                # keep-all: the model again
    wv, wf, wp = _np(whole)
    assert _same(wv, v) and np.array_equal(wf, f) and all(_same(wp[k], p[k]) for k in p)
    # a mask and its complement, merged: the same Gaussians, face by face
    rest = edit.cut_model(m, ~mask)
    joined = edit.merge_models(part, rest)
    jv, jf, jp = _np(joined)
    row = lambda vv, ff, pp: np.concatenate([vv[ff].reshape(len(ff), -1).repeat(G, 0)] + [pp[k].reshape(len(ff) * G, -1) for k in sorted(pp)], 1)
    a, b = row(v, f, p), row(jv, jf, jp)
    order = lambda x: x[np.lexsort(x.T[::-1])]
    assert _same(order(a), order(b))
    with pytest.raises(ValueError, match="no face"):
        edit.cut_model(m, torch.zeros(len(f), dtype=torch.bool, device=DEV))


def test_merge_models():
    a, b = _model(1, 6, 3, True, seed=1), _model(2, 6, 3, True, seed=2, centre=(2.0, 0.0, 0.0))
    va, fa, pa = _np(a)
    vb, fb, pb = _np(b)
    got = a.merged_with(b)
    mv, mf, mp = ref.merge(va, fa, pa, vb, fb, pb)
    gv, gf, gp = _np(got)
    assert _same(gv, mv) and np.array_equal(gf, mf) and all(_same(gp[k], mp[k]) for k in mp) and set(gp) == set(mp)
    assert got.is_loose_bind() and got.n_points == a.n_points + b.n_points
    with pytest.raises(ValueError, match="n_gaussians_per_surface_triangle"):
        edit.merge_models(a, _model(1, 1, 3, True))
    # attach = merge with a moved copy; b itself stays
    R, t = ref.rotation(np.random.default_rng(13)), np.array([0.1, 0.2, 0.3])
    att = edit.attach(a, b, R, t)
    assert _same(_np(b)[0], vb) and _same(_np(b)[2]["_sh_coordinates_rest"], pb["_sh_coordinates_rest"])
    moved = edit.transform_model(_model(2, 6, 3, True, seed=2, centre=(2.0, 0.0, 0.0)), R, t)
    hv, hf, hp = _np(edit.merge_models(a, moved))
    av, af, ap = _np(att)
    assert _same(av, hv) and np.array_equal(af, hf) and all(_same(ap[k], hp[k]) for k in hp)
    assert _same(av[len(va):], ref.transform_points(vb, R, t))
    assert _same(ap["_sh_coordinates_rest"][a.n_points:], ref.rotate_sh(pb["_sh_coordinates_rest"], ref.sh_rotation_matrices(R, 3)))


# ------------------------------------------------------------------------------------------------ 5. painting
def _quad():
    (cx, cy, cz), hw = CENTRE, 0.45 * RADIUS
    z = cz + 0.93 * RADIUS
    anchors = np.array([[cx - hw, cy - hw, z], [cx - hw, cy + hw, z], [cx + hw, cy - hw, z], [cx + hw, cy + hw, z]])
    return anchors, [[0, 1, 2], [1, 2, 3]]


UV_IN = np.array([[0.1, 0.1], [0.1, 0.9], [0.9, 0.1], [0.9, 0.9]])
UV_OUT = np.array([[-0.2, -0.2], [-0.2, 1.2], [1.2, -0.2], [1.2, 1.2]])


def _texture(mode):
    rng = np.random.default_rng(21)
    if mode == "multiply":
        return rng.integers(0, 256, (5, 7), dtype=np.uint8)
    tex = rng.integers(0, 256, (6, 4, 4), dtype=np.uint8)
    tex[::2, :, 3] = 50                                            # not above alpha_min: these texels paint nothing
    tex[1::2, :, 3] = 51
    return tex


@pytest.mark.parametrize("uv,outside", [(UV_IN, False), (UV_OUT, True)], ids=["uv_inside", "uv_outside"])
@pytest.mark.parametrize("mode", ["multiply", "replace"])
def test_paint_decal(mode, uv, outside):
    m = _model(2, 6, 2, seed=4)
    v, f, p = _np(m)
    anchors, tris = _quad()
    tex = _texture(mode)
    kw = dict(mode=mode, bary_slack=0.03, max_dist=0.09)
    scales, dc, n_inside, n_painted, n_outside, touched = ref.paint(v, f, 6, p["_scales"], p["_sh_coordinates_dc"], anchors, uv, tris, tex, **kw)
    res = m.paint_decal(anchors, uv, tris, tex, **kw)
    print(mode, res)
    assert res.n_inside == n_inside == [75, 75] and touched.sum() == 140                       # 10 lie in both triangles
    assert res.n_painted == n_painted and res.n_outside == n_outside and (n_outside > 0) == outside
    assert 0 < n_painted <= 140
    _, _, q = _np(m)
    assert _same(q["_scales"], scales) and _same(q["_sh_coordinates_dc"].reshape(-1, 3), dc)
    assert (q["_scales"][touched] == np.float32(-6.0)).all()
    assert _same(q["_scales"][~touched], p["_scales"][~touched])
    assert _same(q["_sh_coordinates_dc"][~touched], p["_sh_coordinates_dc"][~touched])        # untouched rows keep their bits
    changed = (q["_sh_coordinates_dc"].reshape(-1, 3) != p["_sh_coordinates_dc"].reshape(-1, 3)).any(-1)
    assert changed.sum() <= n_painted and changed.any()
    for k in ("_quaternions", "all_densities", "_sh_coordinates_rest"):
        assert _same(q[k], p[k])


def test_paint_without_shrink_on_rgb_and_a_lost_anchor():
    m = _model(2, 6, 1, seed=5)
    v, f, p = _np(m)
    anchors, tris = _quad()
    tex = np.random.default_rng(22).integers(0, 256, (3, 3, 3), dtype=np.uint8)
    kw = dict(mode="replace", max_dist=0.09, shrink_scale=None)
    scales, dc, n_inside, n_painted, n_outside, _ = ref.paint(v, f, 6, p["_scales"], p["_sh_coordinates_dc"], anchors, UV_IN, tris, tex, **kw)
    res = edit.paint_decal(m, anchors, UV_IN, tris, torch.from_numpy(tex).to(DEV), **kw)
    assert res == edit.PaintResult(n_inside, n_painted, n_outside) and n_painted == 140
    q = _np(m)[2]
    assert _same(q["_scales"], p["_scales"]) and _same(q["_sh_coordinates_dc"].reshape(-1, 3), dc)
    anchors[3] = np.nan                                            # the second triangle loses a corner and holds nothing
    res = edit.paint_decal(m, anchors, UV_IN, tris, tex, **kw)
    assert res.n_inside == [75, 0]


# ------------------------------------------------------------------------------------------------ 6. a sequence
def test_edit_sequence(tmp_path):
    work, out = str(tmp_path / "work"), str(tmp_path / "out")
    frames, iteration = [4, 6], 30
    sources = []
    for i, fr in enumerate(frames):
        m = _model(1, 6, 2, seed=30 + i)
        os.makedirs(os.path.join(work, f"{fr:04d}"))
        formats.save_sugar_checkpoint(os.path.join(work, f"{fr:04d}", f"{iteration}.pt"), m._points.detach(), m._surface_mesh_faces,
                                      m._scales.detach(), m._quaternions.detach(), m.all_densities.detach(), m.sh_coordinates.detach(),
                                      m._thickness(), optimizer_state_dict={"state": {}}, iteration=iteration)
        sources.append(m)
    hat = _model(1, 6, 2, seed=40, centre=(0.0, 0.0, 0.0))
    rng = np.random.default_rng(41)
    anchors0, tris = _quad()
    spin = lambda a: np.array([[np.cos(a), -np.sin(a), 0.0], [np.sin(a), np.cos(a), 0.0], [0.0, 0.0, 1.0]])
    traj = np.stack([(anchors0 - CENTRE) @ spin(0.1 * (i + 1)).T + CENTRE + rng.normal(size=3) * 0.01 for i in range(len(frames))])
    hat_anchors = anchors0 - np.array(CENTRE)
    tex = _texture("multiply")
    groups = _groups()[1:]
    ops = [edit.CutOp(groups), edit.AttachOp(hat, hat_anchors), edit.PaintOp(tex, UV_IN, tris, max_dist=0.09)]
    written = edit.edit_sequence(work, out, frames, iteration, ops, trajectory={"face_trajectory": traj, "frames": np.array([4, 8, 2])})
    assert written == [os.path.join(out, f"{fr:04d}", f"{iteration}.pt") for fr in frames]
    fit = edit.fit_rigid(hat_anchors, traj)
    assert fit.ok.all()
    for i, fr in enumerate(frames):
        m = sources[i]
        sel = edit.faces_in_halfspaces(m._points.detach(), m._surface_mesh_faces, groups)
        assert 0 < int(sel.sum()) < 80
        by_hand = edit.attach(edit.cut_model(m, ~sel), hat, fit.R[i], fit.t[i])
        res = edit.paint_decal(by_hand, traj[i], UV_IN, tris, tex, max_dist=0.09)
        assert res == ops[2].results[i] and res.n_painted > 0
        ck = formats.load_sugar_checkpoint(written[i])
        assert "optimizer_state_dict" not in ck["extra"] and ck["extra"]["iteration"] == iteration
        v, f, p = _np(by_hand)
        assert _same(ck["verts"].numpy(), v) and np.array_equal(ck["faces"].numpy(), f)
        assert _same(ck["raw_scales"].numpy(), p["_scales"]) and _same(ck["raw_complex"].numpy(), p["_quaternions"])
        assert _same(ck["densities"].numpy(), p["all_densities"])
        assert _same(ck["sh"].numpy(), np.concatenate([p["_sh_coordinates_dc"], p["_sh_coordinates_rest"]], 1))
        ov, of, _ = formats.load_obj(os.path.join(out, f"{fr:04d}", "color_mesh.obj"))
        assert np.array_equal(of, f) and np.array_equal(ov.astype(np.float32), v)
