"""The rules of gaustar_amd.remesh as tests/remesh_ref.py restates them (no GPU): hand cases, the selection rule, the flat grid,
closed-mesh invariants, quality against the sequential greedy decimator, smoothing; and the C entry points' argument checks."""
import ctypes
import functools
import itertools

import numpy as np
import pytest

import remesh_ref as R


def _edges(faces):
    f = np.asarray(faces, np.int64)
    return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])


def assert_closed_manifold(verts, faces, chi=2):
    f = np.asarray(faces, np.int64)
    assert (f[:, 0] != f[:, 1]).all() and (f[:, 1] != f[:, 2]).all() and (f[:, 2] != f[:, 0]).all()
    d = _edges(f)
    directed = set(map(tuple, d.tolist()))
    assert len(directed) == len(d)                                  # every directed edge once
    assert all((b, a) in directed for a, b in directed)             # with its reverse
    assert len(verts) - len(directed) // 2 + len(f) == chi
    assert set(f.reshape(-1).tolist()) == set(range(len(verts)))    # no unreferenced vertex


@functools.lru_cache(maxsize=None)
def _simplified(name, target):
    v, f = {"ico2": lambda: R.icosphere(2), "ico3": lambda: R.icosphere(3), "bumpy3": lambda: R.bumpy(3)}[name]()
    return v, f, R.simplify(v, f, target)


# ------------------------------------------------------------------------------------------------ hand cases
def test_tetrahedron_stalls_unchanged():
    v, f = R.tetrahedron()
    r = R.simplify(v, f, 2)
    assert r.stalled and r.n_rounds == 0
    assert np.array_equal(r.verts.view(np.uint32), v.view(np.uint32)) and np.array_equal(r.faces, f)
    assert np.array_equal(r.face_origin, np.arange(4))


def test_octahedron_low_target_ends_at_a_tetrahedron():
    v, f = R.octahedron()
    r = R.simplify(v, f, 2)
    assert r.stalled and len(r.faces) == 4 and len(r.verts) == 4
    assert_closed_manifold(r.verts, r.faces)
    r6 = R.simplify(v, f, 6)
    assert not r6.stalled and len(r6.faces) == 6 and r6.n_rounds == 1
    assert_closed_manifold(r6.verts, r6.faces)
    assert (np.diff(r6.face_origin) > 0).all() and len(r6.face_origin) == 6


def test_fin_edge_vertices_stay():
    v, f, fin = R.fin_mesh()
    r = R.simplify(v, f, 40)
    assert len(r.faces) < len(f)
    out = {tuple(p) for p in r.verts.view(np.uint32).tolist()}
    for w in fin:
        assert tuple(v[w].view(np.uint32).tolist()) in out
    assert len(f) - 1 in r.face_origin.tolist()                     # the fin's own face is never on a collapsed edge


def test_identity_and_argument_checks():
    v, f = R.icosphere(1)
    r = R.simplify(v, f, len(f))
    assert r.n_rounds == 0 and not r.stalled and np.array_equal(r.faces, f) and np.array_equal(r.face_origin, np.arange(len(f)))
    with pytest.raises(ValueError):
        R.simplify(v, f, -1)
    bad = f.copy()
    bad[3, 1] = len(v)
    with pytest.raises(ValueError):
        R.simplify(v, bad, 10)


def test_locked_vertices_keep_their_bits_and_attributes_are_averaged():
    v, f = R.icosphere(2)
    locked = np.zeros(len(v), bool)
    locked[:12] = True
    col = np.random.default_rng(1).random((len(v), 3)).astype(np.float32)
    r = R.simplify(v, f, 100, locked=locked, attrs=(col,))
    out = {tuple(p): i for i, p in enumerate(r.verts.view(np.uint32).tolist())}
    for w in range(12):
        i = out[tuple(v[w].view(np.uint32).tolist())]
        assert np.array_equal(r.attrs[0][i], col[w])
    assert r.attrs[0].dtype == np.float32 and r.attrs[0].shape == (len(r.verts), 3)
    assert r.attrs[0].min() >= col.min() and r.attrs[0].max() <= col.max()


# ------------------------------------------------------------------------------------------------ the selection rule
@pytest.mark.parametrize("mesh", ["ico2", "bumpy3", "grid"])
def test_no_face_touches_two_selected_edges(mesh):
    v, f = {"ico2": lambda: R.icosphere(2), "bumpy3": lambda: R.bumpy(3), "grid": R.flat_grid}[mesh]()
    st = R._State(v, f, None, ())
    for _round in range(3):
        edges, selected, where, vf = R.select_round(st)
        assert selected
        ends = [set(edges[e]) for _k, e in selected]
        touching = [{g for w in s for g in vf[w]} for s in ends]
        for i, j in itertools.combinations(range(len(ends)), 2):
            assert not (touching[i] & touching[j])
        ring = [{w for g in t for w in st.faces[g]} for t in touching]      # the vertices a collapse's tests read
        for i, j in itertools.permutations(range(len(ends)), 2):
            assert not (ring[i] & ends[j])
        for _k, e in selected:
            st.collapse(edges[e][0], edges[e][1], where[e], vf)


# ------------------------------------------------------------------------------------------------ the flat grid
def test_flat_grid_stays_flat_and_keeps_its_boundary():
    v, f = R.flat_grid(9, 0.5)
    r = R.simplify(v, f, 32)
    assert not r.stalled and len(r.faces) in (32, 31)
    assert (r.verts[:, 2].view(np.uint32) == np.float32(0.5).view(np.uint32)).all()
    out = {tuple(p) for p in r.verts.view(np.uint32).tolist()}
    boundary = (v[:, 0] == 0) | (v[:, 0] == 8) | (v[:, 1] == 0) | (v[:, 1] == 8)
    assert boundary.sum() == 32
    for p in v[boundary]:
        assert tuple(p.view(np.uint32).tolist()) in out
    P = r.verts.astype(np.float64)[r.faces]
    n = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
    assert (n[:, 2] > 0).all()
    area = 0.5 * np.linalg.norm(n, axis=1).sum()
    assert abs(area - 64.0) <= 1e-6 * 64.0


# ------------------------------------------------------------------------------------------------ closed meshes
@pytest.mark.parametrize("name,target", [("ico2", 80), ("ico2", 161), ("ico3", 320), ("ico3", 500), ("bumpy3", 640), ("bumpy3", 320)])
def test_closed_mesh_invariants(name, target):
    v, f, r = _simplified(name, target)
    assert not r.stalled
    assert len(r.faces) in (target, target - 1)
    assert_closed_manifold(r.verts, r.faces, chi=2)
    assert (np.diff(r.face_origin) > 0).all() and r.face_origin.min() >= 0 and r.face_origin.max() < len(f)


def test_degenerate_faces_do_not_block():
    v, f = R.degenerate_mesh()
    assert_closed_manifold(v, f)
    r = R.simplify(v, f, 100)
    assert not r.stalled and len(r.faces) in (100, 99)
    assert_closed_manifold(r.verts, r.faces)
    assert np.isfinite(r.verts).all()


# ------------------------------------------------------------------------------------------------ quality
def radial_error(verts, faces):
    """(RMS, max) of | |p| - g(p / |p|) | over the vertices and the face centroids."""
    P = np.asarray(verts, np.float64)
    pts = np.concatenate([P, P[np.asarray(faces, np.int64)].mean(axis=1)])
    rad = np.linalg.norm(pts, axis=1)
    err = np.abs(rad - R.bump(pts / rad[:, None]))
    return float(np.sqrt((err ** 2).mean())), float(err.max())


@pytest.mark.parametrize("target", [640, 320])
def test_quality_against_the_greedy_decimator(target):
    """The parallel rounds against the sequential greedy decimator on the bumpy level-3 icosphere, whose true surface is known in
    closed form: RMS radial error at most 1.25 x the greedy one's.  Measured: to 640 faces 1.015 x, to 320 faces 1.009 x; the
    maxima 1.253 x and 1.020 x, printed and not asserted (NOTEBOOK.md)."""
    v, f, par = _simplified("bumpy3", target)
    seq = R.greedy_simplify(v, f, target)
    assert len(seq.faces) == target and not seq.stalled
    assert_closed_manifold(seq.verts, seq.faces)
    (prms, pmax), (srms, smax) = radial_error(par.verts, par.faces), radial_error(seq.verts, seq.faces)
    print(f"\nbumpy level 3 -> {target}: parallel RMS {prms:.6f} max {pmax:.6f} ({len(par.faces)} faces, {par.n_rounds} rounds); "
          f"greedy RMS {srms:.6f} max {smax:.6f}; ratio RMS {prms / srms:.3f} max {pmax / smax:.3f}")
    assert prms <= 1.25 * srms


# ------------------------------------------------------------------------------------------------ smoothing
def _noisy_with_extras():
    """The noisy level-2 icosphere with one isolated vertex appended and one locked vertex."""
    v, f = R.noisy_sphere(2, seed=3)
    v = np.concatenate([v, np.asarray([[2.0, 2.0, 2.0]], np.float32)])
    locked = np.zeros(len(v), bool)
    locked[5] = True
    return v, f, locked


@pytest.mark.parametrize("weights", ["inverse_distance", "uniform"])
def test_smoothing_keeps_isolated_and_locked_vertices(weights):
    v, f, locked = _noisy_with_extras()
    for lambdas, steps in (((0.5, 0.5), 10), ((0.5, -0.53), 20)):
        out = R.smooth(v, f, steps, lambdas, weights, locked)
        assert out.dtype == np.float32 and np.isfinite(out).all()
        assert np.array_equal(out[-1].view(np.uint32), v[-1].view(np.uint32))
        assert np.array_equal(out[5].view(np.uint32), v[5].view(np.uint32))
        assert not np.array_equal(out[6], v[6])


def test_laplacian_variance_falls_and_taubin_shrinks_less():
    """The noise amplitude is 0.2 (variance 0.04) because smoothing a CLEAN level-2 icosphere makes a radius variance of its own:
    its twelve vertices of valence 5 shrink at another rate than the rest, 8.8e-5 after ten sweeps.  The variance can only be
    asked to fall sweep after sweep while the noise that is left stays well above that."""
    v, f = R.noisy_sphere(2, seed=3, amp=0.2)
    var = [np.linalg.norm(v.astype(np.float64), axis=1).var()]
    for k in range(1, 11):
        var.append(np.linalg.norm(R.smooth(v, f, k, (0.5, 0.5)).astype(np.float64), axis=1).var())
    assert (np.diff(var) < 0).all()
    r0 = np.linalg.norm(v.astype(np.float64), axis=1).mean()
    lap = np.linalg.norm(R.smooth(v, f, 10, (0.5, 0.5)).astype(np.float64), axis=1).mean()
    tau = np.linalg.norm(R.smooth(v, f, 20, (0.5, -0.53)).astype(np.float64), axis=1).mean()
    assert r0 - tau < r0 - lap and r0 - lap > 0


# ------------------------------------------------------------------------------------------------ the C entry points
def test_entry_points_validate_without_gpu(hip_lib):
    """Null pointers, sizes that are not positive and a negative target fail loudly before any device work."""
    null = None
    buf = (ctypes.c_double * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = hip_lib.gsr_last_error
    assert hip_lib.gsr_abi_version() == 16
    assert hip_lib.gsr_remesh_setup(4, 4, *([null] * 6), null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_setup(0, 4, *([p] * 6), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_setup(4, 0, *([p] * 6), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_setup(2 ** 31 - 1, 4, *([p] * 6), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_keys(4, 4, *([null] * 5), null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_keys(-1, 4, *([p] * 5), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_vertex_quadrics(4, 4, *([null] * 4), null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_vertex_quadrics(4, -2, *([p] * 4), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_edge_heads(12, null, null, null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_edge_heads(0, p, p, null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_edges(12, 4, *([null] * 6), null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_edges(12, 0, *([p] * 6), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_candidates(12, null, 4, 4, *([null] * 10), null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_candidates(0, p, 4, 4, *([p] * 10), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_select(12, null, 4, *([null] * 5), null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_select(12, p, 0, *([p] * 5), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_apply(12, null, 4, 4, *([null] * 10), null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_apply(12, p, 0, 4, *([p] * 10), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_apply_attr(12, null, 4, 3, *([null] * 4), null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_apply_attr(12, p, 4, 0, *([p] * 4), null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_narrow(12, null, null, null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_narrow(0, p, p, null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_smooth(4, null, null, null, 1, 0.5, 0.5, 0, null, null, null, null, null) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_smooth(0, p, p, null, 1, 0.5, 0.5, 0, p, p, p, p, null) != 0 and b"positive" in err()
    assert hip_lib.gsr_remesh_smooth(4, p, p, null, -1, 0.5, 0.5, 0, p, p, p, p, null) != 0 and b"negative" in err()
    # the cap is host arithmetic: min(n_selected, (live - target + 1) / 2)
    n = ctypes.c_int(7)
    assert hip_lib.gsr_remesh_cap(100, -1, 5, ctypes.byref(n)) != 0 and b"target_faces" in err() and n.value == 0
    assert hip_lib.gsr_remesh_cap(100, 50, 5, None) != 0 and b"null" in err()
    assert hip_lib.gsr_remesh_cap(-1, 50, 5, ctypes.byref(n)) != 0 and b"negative" in err()
    for live, target, sel, want in ((100, 50, 40, 25), (100, 51, 40, 25), (100, 50, 7, 7), (50, 50, 9, 0), (40, 50, 9, 0), (3, 0, 9, 2)):
        assert hip_lib.gsr_remesh_cap(live, target, sel, ctypes.byref(n)) == 0 and n.value == want
