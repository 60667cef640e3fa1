"""The stitch of gaustar_amd.regions on the GPU against the numpy restatement tests/stitch_ref.py (itself pinned by
tests/test_stitch.py).  Every output is an integer or an exactly defined float, so every comparison is exact: np.array_equal,
floats by their bits.  No tolerances."""
import functools

import numpy as np
import pytest
import torch

import regions_ref as rr
import stitch_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _n(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _consts():
    from gaustar_amd import regions
    return regions.NN_TILE, regions.NN_QUERIES


# ---------------------------------------------------------------------------------------------------- nearest vertex
@functools.lru_cache(maxsize=None)
def _cloud(kind, n, seed):
    """n points, read-only: 'lattice' = integers in [0, 6)^3 (exact ties, duplicates), 'random' = f32 in [-1, 1)^3."""
    rng = np.random.default_rng(seed)
    pts = rng.integers(0, 6, (n, 3)).astype(np.float32) if kind == "lattice" else rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    pts.setflags(write=False)
    return pts


def _check_nearest(q, c):
    from gaustar_amd import regions
    want_idx, want_d2 = ref.nearest_vertices(q, c)
    tq, tc = _t(q), _t(c)
    idx, d2, mx = regions.nearest_vertices(tq, tc, return_max=True)
    assert idx.dtype == torch.int32 and d2.dtype == torch.float64
    assert np.array_equal(_n(idx), want_idx), np.flatnonzero(_n(idx) != want_idx)[:8]
    assert _same_bits(_n(d2), want_d2)
    assert _same_bits(np.float64(mx), np.float64(want_d2.max()))
    idx2, d22 = regions.nearest_vertices(tq, tc)                  # the same bits over two calls
    assert np.array_equal(_n(idx2), _n(idx)) and _same_bits(_n(d22), _n(d2))
    return want_idx


def _sizes():
    T, Q = _consts()
    return [1, Q - 1, Q, Q + 1, 63, 64, 65, T - 1, T, T + 1, 3 * T + 3]


@pytest.mark.parametrize("kind", ["lattice", "random"])
@pytest.mark.parametrize("ci", range(11))
def test_nearest_sizes(kind, ci):
    """Bq and Bc over 1, 63, 64, 65, the tile size and the queries of a workgroup with their neighbours, and three tiles and a
    bit.  The answer for a prefix of the queries is the prefix of the answer, so the restatement runs once per Bc."""
    from gaustar_amd import regions
    sizes = _sizes()
    Bc = sizes[ci]
    q, c = _cloud(kind, max(sizes), 1), _cloud(kind, max(sizes), 2)[:Bc]
    want_idx, want_d2 = ref.nearest_vertices(q, c)
    if kind == "lattice" and Bc > 64:
        assert (want_d2 == 0).any() and len(np.unique(c, axis=0)) < Bc          # ties and duplicates are there
    tc = _t(c)
    for Bq in sizes:
        idx, d2, mx = regions.nearest_vertices(_t(q[:Bq]), tc, return_max=True)
        assert np.array_equal(_n(idx), want_idx[:Bq]), (Bq, Bc)
        assert _same_bits(_n(d2), want_d2[:Bq]), (Bq, Bc)
        assert _same_bits(np.float64(mx), np.float64(want_d2[:Bq].max())), (Bq, Bc)
    _check_nearest(q[:sizes[-2]], c)


def test_nearest_duplicates_across_tile_and_wave_share():
    """One position at candidates that fall into different lanes' shares, different waves' shares and different tiles: the
    lowest index wins, for queries on it and around it."""
    T, Q = _consts()
    c = _cloud("random", 2 * T + 40, 3).copy()
    spot = np.array([0.25, -0.5, 0.125], np.float32)
    twins = [T + 3, 7, 8, 23, T - 1, T, 2 * T + 5]                 # 7: the lowest
    c[twins] = spot
    c[5] = spot + np.float32(1e-3)                                 # a near miss with a lower index
    q = np.concatenate([spot[None], spot[None] + _cloud("random", 4 * Q + 1, 4) * np.float32(1e-4), _cloud("random", 70, 5)])
    want = _check_nearest(q.astype(np.float32), c)
    assert want[0] == 7 and (want[:4 * Q + 2] == 7).all()
    c[7] = c[9]
    assert _check_nearest(q.astype(np.float32), c)[0] == 8


def test_nearest_negative_zero():
    T, _Q = _consts()
    c = _cloud("lattice", T + 9, 6).copy()
    c[::3, 0] = -0.0
    c[1::3, 1] *= -1
    q = _cloud("lattice", 200, 7).copy()
    q[::2, 0] = -0.0
    q[::5] = [-0.0, -0.0, -0.0]
    want = _check_nearest(q, c)
    assert (c[want[::5]] == 0).all(axis=1).any()                   # (-0, -0, -0) found (+0, +0, +0) or its like at distance 0


# ---------------------------------------------------------------------------------------------------- connect_two_meshes
def _check_connect(v1, f1, b1, v2, f2, b2, **kw):
    from gaustar_amd import regions
    args = [_t(v1), _t(f1), _t(np.asarray(b1, np.int32)), _t(v2), _t(f2), _t(np.asarray(b2, np.int32))]
    before = [a.clone() for a in args]
    got = regions.connect_two_meshes(*args, **kw)
    for a, b in zip(args, before):
        assert torch.equal(a, b)                                   # the inputs are not modified
    want = ref.connect_two_meshes(v1, f1, b1, v2, f2, b2, **kw)
    assert got.faces.dtype == torch.int32 and got.vert_map.dtype == torch.int32 and got.face_mask.dtype == torch.bool
    assert np.array_equal(_n(got.faces), want["faces"]) and _same_bits(_n(got.verts), want["verts"])
    assert np.array_equal(_n(got.face_mask), want["face_mask"]) and np.array_equal(_n(got.vert_map), want["vert_map"])
    assert got.n_faces_from_first == want["n_faces_from_first"] and got.watertight is want["watertight"]
    assert isinstance(got.max_dist, float) and _same_bits(np.float64(got.max_dist), np.float64(want["max_dist"]))
    return got, want


@functools.lru_cache(maxsize=None)
def _torus_case():
    """M: a closed 24 x 16 torus; M': M with its vertices permuted and jittered by less than a tenth of the shortest edge; a box
    over x > x0, x0 between two columns of vertices and further from every vertex than the jitter."""
    v, f = ref.torus(24, 16)
    e = rr.face_edges(f).reshape(-1, 2)
    shortest = float(np.linalg.norm(v[e[:, 0]].astype(np.float64) - v[e[:, 1]].astype(np.float64), axis=1).min())
    bound = 0.1 * shortest
    rng = np.random.default_rng(11)
    order = rng.permutation(len(v))
    inv = np.empty(len(v), np.int64)
    inv[order] = np.arange(len(v))
    jitter = rng.uniform(-1, 1, v.shape) * (0.99 * bound / np.sqrt(3))
    vp = (v[order].astype(np.float64) + jitter[order]).astype(np.float32)
    fp = inv[f].astype(np.int32)
    xs = np.unique(np.concatenate([v[:, 0], vp[:, 0]]).astype(np.float64))
    xs = xs[(xs > 0.5) & (xs < 1.8)]
    g = int(np.argmax(np.diff(xs)))
    box = np.array([[0.5 * (xs[g] + xs[g + 1]), -5, -5], [5, 5, 5]], np.float64)
    assert np.array_equal(rr.inside_box(v, box), rr.inside_box(vp, box)[inv])
    assert np.linalg.norm(vp[inv].astype(np.float64) - v, axis=1).max() < bound
    for a in (v, f, vp, fp, box):
        a.setflags(write=False)
    return v, f, vp, fp, box, bound


def test_closed_surface_is_restored():
    """The base cut and the patch are complementary parts of one closed surface and share exactly the boundary ring: the
    stitch has the surface's face and vertex counts, keeps every face and is watertight -- whatever the restatement says."""
    v, f, vp, fp, box, bound = _torus_case()
    base = rr.cut_mesh_by_box(v, f, box, True)
    patch = rr.cut_mesh_by_box(vp, fp, box, False)
    assert base["face_mask"].sum() + patch["face_mask"].sum() == len(f) and 0 < base["face_mask"].sum() < len(f)
    b1 = rr.boundary_vertices(base["verts"], base["faces"])
    b2 = rr.boundary_vertices(patch["verts"], patch["faces"])
    assert len(b1) == len(b2) > 16
    got, _want = _check_connect(base["verts"], base["faces"], b1, patch["verts"], patch["faces"], b2)
    assert got.watertight is True
    assert got.faces.shape[0] == len(f) and got.verts.shape[0] == len(v)
    assert bool(got.face_mask.all()) and got.n_faces_from_first == len(base["faces"])
    assert 0 < got.max_dist <= bound
    vm = _n(got.vert_map)
    assert (vm >= 0).all() and len(np.unique(vm)) == len(v)
    assert _same_bits(_n(got.verts)[vm[:len(base["verts"])]], base["verts"])        # the base's vertices did not move


@pytest.mark.parametrize("max_hole", [0, 10])
def test_duplicate_base_boundary_positions(max_hole):
    """Base boundary vertices 1 and 4 share a position and 4 is listed first: the group's representative is 4."""
    v1 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [1, 0, 0], [2, 1, 0]], np.float32)
    f1 = np.array([[0, 1, 2], [3, 5, 4]], np.int32)
    v2 = np.array([[1.01, -0.02, 0], [0.9, 0.01, 0], [1, -1, 0], [2.02, 0, 0], [-0.03, 0, 0]], np.float32)
    f2 = np.array([[0, 2, 3], [1, 4, 2], [0, 1, 2]], np.int32)
    got, want = _check_connect(v1, f1, [4, 0, 1, 3], v2, f2, [3, 0, 1, 4], max_hole_vert_num=max_hole)
    if max_hole == 0:
        vm = _n(got.vert_map)
        assert vm[1] == vm[4] == vm[6 + 0] == vm[6 + 1] and vm[3] == vm[6 + 3] and vm[0] == vm[6 + 4]
        assert _n(got.face_mask).tolist() == [True, True, True, True, False]          # patch face (0, 1, 2) collapsed
        faces = _n(got.faces)
        assert faces[0, 1] == faces[1, 2] == vm[4]                                     # rewritten to 4's new index


@pytest.mark.parametrize("max_hole", [0, 10])
def test_dense_patch_boundary_gives_degenerate_faces(max_hole):
    """The patch's boundary row has twice the base's vertices (the odd ones midway: exact ties, the lower base index wins):
    several snap to one base vertex, their faces degenerate and go."""
    v1, f1 = rr.quad_grid(4, 1)
    v2, f2 = rr.quad_grid(8, 1)
    v2 = (v2 * np.float32([0.5, 1, 1]) + np.float32([0, 1, 0])).astype(np.float32)
    got, want = _check_connect(v1, f1, np.arange(5, 10), v2, f2, np.arange(0, 9), max_hole_vert_num=max_hole)
    mask = _n(got.face_mask)
    assert got.faces.shape[0] == mask.sum() and got.n_faces_from_first == mask[:len(f1)].sum()
    if max_hole == 0:
        assert mask[:len(f1)].all() and 0 < (~mask[len(f1):]).sum() < len(f2)


# ---------------------------------------------------------------------------------------------------- holes
def _check_merge(verts, faces, **kw):
    from gaustar_amd import regions
    tv, tf = _t(verts), _t(faces)
    bv, bf = tv.clone(), tf.clone()
    got = regions.merge_vertices_around_holes(tv, tf, **kw)
    assert torch.equal(tv, bv) and torch.equal(tf, bf)
    want = ref.merge_vertices_around_holes(verts, faces, **kw)
    assert np.array_equal(_n(got.faces), want["faces"]) and _same_bits(_n(got.verts), want["verts"])
    assert np.array_equal(_n(got.face_mask), want["face_mask"]) and np.array_equal(_n(got.vert_map), want["vert_map"])
    return got


def _fan(n, centre=(0, 0, 0), phase=0.0, v0=0):
    a = 2 * np.pi * np.arange(n) / n + phase
    verts = (np.concatenate([np.zeros((1, 3)), np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)]) + np.asarray(centre)).astype(np.float32)
    faces = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32) + v0
    return verts, faces


def test_holes_of_3_10_and_11_vertices():
    parts, v0 = [], 0
    for n, cx in ((3, 0), (10, 4), (11, 8)):
        v, f = _fan(n, (cx, 0, 0), v0=v0)
        parts.append((v, f))
        v0 += len(v)
    verts, faces = np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])
    got = _check_merge(verts, faces)
    assert np.array_equal(_n(got.faces), parts[2][1] - 15) and got.verts.shape[0] == 12          # only the 11-fan is left
    got = _check_merge(verts, faces, max_hole_vert_num=3)
    assert got.faces.shape[0] == 21


def test_two_small_holes_that_land_on_one_position():
    """Two 4-vertex holes in one sheet whose lowest vertices share a position: after the move all eight are one group, and the
    faces around both holes name its lowest vertex."""
    verts, faces = rr.quad_grid(7, 3)
    faces = np.delete(faces, [2 * (7 + 1), 2 * (7 + 1) + 1, 2 * (7 + 4), 2 * (7 + 4) + 1], axis=0)      # quads (1, 1) and (4, 1)
    verts[12] = verts[9]                                          # the holes' lowest vertices
    got = _check_merge(verts, faces)
    vm = _n(got.vert_map)
    assert vm[9] >= 0 and (vm[[9, 10, 17, 18, 12, 13, 20, 21]] == vm[9]).all()
    assert (_n(got.faces) == vm[9]).sum() > 8 and got.verts.shape[0] == len(verts) - 7


@pytest.mark.parametrize("F", [1, 63, 64, 65, 257])
def test_hole_merging_sizes(F):
    nq = (F + 1) // 2
    verts, faces = rr.quad_grid(nq, 1)
    _check_merge(verts, faces[:F])
    verts, faces = rr.quad_grid(nq, 2)                               # small holes inside a rim that is too long to merge
    gone = [2 * q + k for q in range(1, nq, 3) for k in (0, 1)]
    faces = np.delete(faces, gone, axis=0)[:max(F, 2)]
    _check_merge(verts, faces)
    _check_merge(verts, faces, max_hole_vert_num=3)


# ---------------------------------------------------------------------------------------------------- select, watertight
def test_select_faces():
    from gaustar_amd import regions
    v, f = ref.torus(9, 7)
    colours = np.random.default_rng(2).uniform(0, 1, (len(v), 3)).astype(np.float32)
    ids = np.arange(len(v), dtype=np.int32)
    for mask in (np.zeros(len(f), bool), np.ones(len(f), bool), np.random.default_rng(3).random(len(f)) < 0.2):
        got = regions.select_faces(_t(v), _t(f), _t(mask), attrs=(_t(colours), _t(ids)))
        want = ref.select_faces(v, f, mask, attrs=(colours, ids))
        assert np.array_equal(_n(got.faces), want["faces"]) and _same_bits(_n(got.verts), want["verts"])
        assert np.array_equal(_n(got.face_mask), want["face_mask"]) and np.array_equal(_n(got.vert_map), want["vert_map"])
        assert _same_bits(_n(got.attrs[0]), want["attrs"][0]) and np.array_equal(_n(got.attrs[1]), want["attrs"][1])


def test_is_watertight():
    from gaustar_amd import regions
    _v, torus = ref.torus(24, 16)
    assert regions.is_watertight(_t(torus)) is True
    assert regions.is_watertight(_t(rr.quad_grid(7, 5)[1])) is False
    assert regions.is_watertight(_t(np.zeros((0, 3), np.int32))) is False
    assert regions.is_watertight(_t(torus[:-1])) is False
    assert regions.is_watertight(_t(np.concatenate([torus, torus[:1]]))) is False     # an edge of three faces


# ---------------------------------------------------------------------------------------------------- the harness
def test_stitch_update_region():
    from gaustar_amd import harness, regions
    v, f, vp, fp, box, bound = _torus_case()
    model = harness.SurfaceGaussians(_t(v), _t(f, torch.long), n_gaussians_per_surface_triangle=1, sh_levels=1)
    colours = np.random.default_rng(8).uniform(0, 1, (len(vp), 3)).astype(np.float32)
    cut = regions.RegionCut(box=box, fusion_patch=regions.cut_mesh_by_box(_t(vp), _t(fp), box, False, attrs=(_t(colours),)),
                            base_cut=regions.cut_mesh_by_box(_t(v), _t(f), box, True))
    out = model.stitch_update_region(cut, pad=1.0)
    base = rr.cut_mesh_by_box(v, f, box, True)
    patch = rr.cut_mesh_by_box(vp, fp, box, False, attrs=(colours,))
    keep = rr.outlier_component_mask(patch["faces"], 50)
    patch = ref.select_faces(patch["verts"], patch["faces"], keep, attrs=patch["attrs"])
    b1 = rr.boundary_vertices(base["verts"], base["faces"], box, True, 1.0)
    b2 = rr.boundary_vertices(patch["verts"], patch["faces"], box, False)
    want = ref.connect_two_meshes(base["verts"], base["faces"], b1, patch["verts"], patch["faces"], b2)
    st = out.stitched
    assert np.array_equal(_n(st.faces), want["faces"]) and _same_bits(_n(st.verts), want["verts"])
    assert np.array_equal(_n(st.face_mask), want["face_mask"]) and st.watertight is True and want["watertight"] is True
    assert _same_bits(_n(out.patch.attrs[0]), patch["attrs"][0])
    m = base["face_mask"].copy()                                     # :656-658
    m[base["face_mask"]] = want["face_mask"][:len(base["faces"])]
    assert out.base_face_mask.dtype == torch.bool and np.array_equal(_n(out.base_face_mask), m)
    # a pad that reaches no base boundary vertex, an empty patch
    assert model.stitch_update_region(cut, pad=1e-6) is None
    far = np.array([[50, 50, 50], [51, 51, 51]], np.float64)
    empty = regions.RegionCut(box=far, fusion_patch=regions.cut_mesh_by_box(_t(vp), _t(fp), far, False, attrs=(_t(colours),)),
                              base_cut=regions.cut_mesh_by_box(_t(v), _t(f), far, True))
    assert empty.fusion_patch.faces.shape[0] == 0 and model.stitch_update_region(empty) is None


def test_stitch_update_region_is_the_public_primitives():
    """stitch_update_region equals, bit for bit, the sequence of public calls its docstring names -- whatever private helpers
    the harness and update_mesh_topology share to state one box."""
    from gaustar_amd import harness, regions
    v, f, vp, fp, box, _bound = _torus_case()
    model = harness.SurfaceGaussians(_t(v), _t(f, torch.long), n_gaussians_per_surface_triangle=1, sh_levels=1)
    colours = np.random.default_rng(8).uniform(0, 1, (len(vp), 3)).astype(np.float32)
    cut = regions.RegionCut(box=box, fusion_patch=regions.cut_mesh_by_box(_t(vp), _t(fp), box, False, attrs=(_t(colours),)),
                            base_cut=regions.cut_mesh_by_box(_t(v), _t(f), box, True))
    out = model.stitch_update_region(cut, pad=1.0)
    patch, base = cut.fusion_patch, cut.base_cut
    keep = regions.outlier_component_mask(patch.faces, 50)
    patch = regions.select_faces(patch.verts, patch.faces, keep, attrs=patch.attrs)
    b2 = regions.boundary_vertices(patch.verts, patch.faces, box, cut_inner=False)
    b1 = regions.boundary_vertices(base.verts, base.faces, box, cut_inner=True, pad=1.0)
    assert b1.shape[0] > 16 and b2.shape[0] > 16
    st = regions.connect_two_meshes(base.verts, base.faces, b1, patch.verts, patch.faces, b2)
    mask = regions.compose_face_mask(base.face_mask, st.face_mask[:int(base.faces.shape[0])])
    assert torch.equal(out.stitched.faces, st.faces) and _same_bits(_n(out.stitched.verts), _n(st.verts))
    assert torch.equal(out.stitched.face_mask, st.face_mask) and torch.equal(out.base_face_mask, mask)
    assert torch.equal(out.patch.faces, patch.faces) and _same_bits(_n(out.patch.attrs[0]), _n(patch.attrs[0]))


# ---------------------------------------------------------------------------------------------------- errors
def test_errors():
    """Bad lists are caught by the err word before anything is gathered through them: nothing here faults the device."""
    from gaustar_amd import regions
    v1, f1 = rr.quad_grid(4, 1)
    v2, f2 = rr.quad_grid(4, 1)
    v2 = v2 + np.float32([0, 1, 0])
    good1, good2 = np.arange(5, 10, dtype=np.int32), np.arange(0, 5, dtype=np.int32)

    def call(b1=good1, b2=good2, verts1=v1):
        return regions.connect_two_meshes(_t(verts1), _t(f1), _t(b1), _t(v2), _t(f2), _t(b2))

    assert call().faces.shape[0] > 0
    for bad in (np.array([5, 6, 10], np.int32), np.array([-1, 6], np.int32)):
        with pytest.raises(ValueError, match="outside"):
            call(b1=bad)
        with pytest.raises(ValueError, match="outside"):
            call(b2=bad)
    with pytest.raises(ValueError, match="twice"):
        call(b1=np.array([5, 6, 5], np.int32))
    with pytest.raises(ValueError, match="twice"):
        call(b2=np.array([1, 1], np.int32))
    with pytest.raises(ValueError, match="empty"):
        call(b1=np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="empty"):
        call(b2=np.zeros(0, np.int32))
    with pytest.raises(ValueError, match="int32"):
        call(b1=good1.astype(np.int64))
    nan = v1.copy()
    nan[7, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        call(verts1=nan)
    with pytest.raises(ValueError, match="NaN"):
        regions.nearest_vertices(_t(nan), _t(v2))
    with pytest.raises(ValueError, match="NaN"):
        regions.nearest_vertices(_t(v2), _t(nan))
    with pytest.raises(ValueError, match="candidates"):
        regions.nearest_vertices(_t(v2), _t(np.zeros((0, 3), np.float32)))
    idx, d2 = regions.nearest_vertices(_t(np.zeros((0, 3), np.float32)), _t(v2))
    assert idx.shape == (0,) and d2.shape == (0,)
    assert call().faces.shape[0] > 0                                # and the device is as it was
