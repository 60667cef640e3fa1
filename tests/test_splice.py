"""tests/splice_ref.py, the numpy restatement of fill_small_holes, the loop over the boxes and the choice of the pad, pinned
against answers written by hand and against scipy's connected_components.  The functions of gaustar_amd.regions that run
without a GPU (choose_aabb_pad, TopologyUpdate.save / gaussian_mask) are tested here as well.  No GPU."""
import functools
import os

import numpy as np
import pytest
import torch

import regions_ref as rr
import splice_ref as ref
import stitch_ref as sr

TETRA = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [2, 3, 0]], np.int32)
# a cube of 12 triangles, outward winding; vertex = x + 2 y + 4 z
CUBE = np.array([[0, 2, 3], [0, 3, 1], [4, 5, 7], [4, 7, 6], [0, 1, 5], [0, 5, 4], [2, 6, 7], [2, 7, 3], [0, 4, 6], [0, 6, 2],
                 [1, 3, 7], [1, 7, 5]], np.int32)


def directed_edges(faces):
    f = np.asarray(faces).reshape(-1, 3)
    return [(int(t[e]), int(t[(e + 1) % 3])) for t in f for e in range(3)]


def consistently_wound(faces):
    """Closed and every directed edge occurs exactly once."""
    d = directed_edges(faces)
    return sr.is_watertight(faces) and len(set(d)) == len(d)


def test_meshes_are_closed():
    assert consistently_wound(TETRA) and consistently_wound(CUBE)
    v, f = ref.icosahedron()
    assert consistently_wound(f) and len(f) == 20
    v3, f3 = ref.icosphere(3)
    assert f3.shape == (1280, 3) and consistently_wound(f3)
    assert np.allclose(np.linalg.norm(v3, axis=1), 1, atol=1e-6)
    assert (ref.face_areas(v3, f3) > 0).all()


def test_triangle_hole():
    for k in range(4):
        out = ref.fill_small_holes(np.delete(TETRA, k, axis=0))
        assert out["n_new"] == 1 and out["watertight"] and consistently_wound(out["faces"])
        assert out["rim_of_new"].tolist() == [int(TETRA[k].min())]
        assert np.array_equal(out["faces"][:3], np.delete(TETRA, k, axis=0))
        assert out["faces"][3, 0] == TETRA[k].min() and sorted(out["faces"][3]) == sorted(TETRA[k])
    # by hand: without (0, 1, 2) the rim's edges run 1->0, 2->1, 0->2 in their faces; m = 0, x = 1, y = 2; 0 -> 1 does not
    # occur, so the face stays (0, 1, 2)
    assert ref.fill_small_holes(TETRA[1:])["faces"][3].tolist() == [0, 1, 2]
    # without (0, 3, 1): m = 0, x = 1, y = 3, and 0 -> 1 is a boundary edge of (0, 1, 2): reversed
    assert ref.fill_small_holes(np.delete(TETRA, 1, axis=0))["faces"][3].tolist() == [0, 3, 1]


def test_lone_triangle_gains_its_twin():
    out = ref.fill_small_holes(np.array([[4, 2, 7]], np.int32))
    assert out["faces"].tolist() == [[4, 2, 7], [2, 4, 7]] and out["watertight"] and out["rim_of_new"].tolist() == [2]
    assert consistently_wound(out["faces"])


@pytest.mark.parametrize("corner", range(4))
def test_quad_hole(corner):
    """The cube without its z = 0 face (vertices 0, 2, 3, 1 around), numbered so that the lowest rim vertex sits at each of
    the four corners in turn: the diagonal passes through it."""
    ring = [0, 2, 3, 1]
    perm = np.arange(8)
    low = ring[corner]
    perm[[0, low]] = perm[[low, 0]]                     # old vertex `low` becomes vertex 0, the lowest
    faces = perm[CUBE[2:]].astype(np.int32)
    out = ref.fill_small_holes(faces)
    assert out["n_new"] == 2 and out["watertight"] and consistently_wound(out["faces"])
    A, B = out["faces"][-2:]
    shared = set(A.tolist()) & set(B.tolist())
    new_ring = [int(perm[r]) for r in ring]
    opposite = new_ring[(new_ring.index(0) + 2) % 4]
    assert shared == {0, opposite} and out["rim_of_new"].tolist() == [0, 0]
    assert A[0] == 0 and B[0] == opposite
    x, y = sorted(set(new_ring) - {0, opposite})
    assert x in A and y in B


def test_quad_hole_by_hand():
    # CUBE without (0, 2, 3), (0, 3, 1): boundary edges in their faces 2->0 (0, 6, 2), 3->2 (2, 7, 3), 1->3 (1, 3, 7),
    # 0->1 (0, 1, 5).  m = 0, x = 1, y = 2, o = 3.  A = (0, 1, 3): 0->1 is a boundary edge, reversed to (0, 3, 1).
    # B = (3, 2, 0): 3->2 is a boundary edge, reversed to (3, 0, 2).
    out = ref.fill_small_holes(CUBE[2:])
    assert out["faces"][-2:].tolist() == [[0, 3, 1], [3, 0, 2]]


def test_rims_that_stay():
    v, f = ref.icosahedron()
    fan = f[(f != 0).all(axis=1)]
    out = ref.fill_small_holes(fan)
    assert len(fan) == 15 and out["n_new"] == 0 and np.array_equal(out["faces"], fan) and not out["watertight"]
    assert ref.rim_census(fan) == (0, 0, 1)
    # two triangle holes that share vertex 0: its degree is 4
    two = np.array([t for t in f.tolist() if t not in ([0, 11, 5], [0, 1, 7])], np.int32)
    assert len(two) == 18 and ref.rim_census(two) == (0, 0, 1)
    assert ref.fill_small_holes(two)["n_new"] == 0
    # an edge of three faces next to a hole: TETRA without (0, 1, 2), and a fin (1, 2, 9) on the rim edge 1-2.  The edge 1-2
    # has count 2 now and is no boundary edge; the component {0, 1, 2, 9} has the edges 0-1, 0-2, 1-9, 2-9: a rim of 4
    fin = np.concatenate([TETRA[1:], [[1, 2, 9]]]).astype(np.int32)
    assert sorted(tuple(sorted(e)) for e in ref.boundary_edges(fin)) == [(0, 1), (0, 2), (1, 9), (2, 9)]
    assert ref.fill_small_holes(fin)["n_new"] == 2
    # and with a second fin the edge has count 3 and links nothing: 0-1, 0-2 and the two fins' outer edges
    fins = np.concatenate([fin, [[2, 1, 8]]]).astype(np.int32)
    assert (1, 2) not in [tuple(sorted(e)) for e in ref.boundary_edges(fins)]
    out = ref.fill_small_holes(fins)
    assert ref.rim_census(fins) == (0, 0, 1) and out["n_new"] == 0          # vertices 1 and 2 have degree 3


def flipped_quad_case():
    """CUBE without its z = 0 face, with the face (2, 7, 3) flipped: the rim's edges are not consistently directed."""
    faces = CUBE[2:].copy()
    k = [i for i, t in enumerate(faces.tolist()) if t == [2, 7, 3]][0]
    faces[k] = [2, 3, 7]
    return faces


def test_winding_rule_tests_each_face_on_its_own_edge():
    faces = flipped_quad_case()
    # boundary edges now: 2->0, 2->3, 1->3, 0->1.  A = (0, 1, 3) reversed (0->1 runs); B = (3, 2, 0) NOT reversed (3->2 does not)
    out = ref.fill_small_holes(faces)
    assert out["faces"][-2:].tolist() == [[0, 3, 1], [3, 2, 0]]
    tied = ref.fill_small_holes(faces, tie_windings=True)
    second = ref.fill_small_holes(faces, test_second_edge=True)
    assert not np.array_equal(tied["faces"], out["faces"]) and not np.array_equal(second["faces"], out["faces"])
    # on the consistent cube the tied variant is indistinguishable: the flipped case is what tells them apart
    assert np.array_equal(ref.fill_small_holes(CUBE[2:], tie_windings=True)["faces"], ref.fill_small_holes(CUBE[2:])["faces"])


@functools.lru_cache(maxsize=None)
def grid_case():
    """A 40 x 40 quad grid (3 200 triangles) without about 100 scattered single triangles and diagonal pairs, no two holes
    touching, the vertices renumbered by a seeded permutation.  Read-only."""
    _v, f = rr.quad_grid(40, 40)
    rng = np.random.default_rng(5)
    drop = []
    for j in range(2, 38, 4):
        for i in range(2, 38, 3):
            q = 2 * (j * 40 + i)
            kind = rng.integers(0, 3)
            drop += [q] if kind == 0 else ([q + 1] if kind == 1 else [q, q + 1])
    f = np.delete(f, drop, axis=0)
    perm = rng.permutation(41 * 41).astype(np.int32)
    f = perm[f]
    f.setflags(write=False)
    return f, 41 * 41


def test_rims_against_scipy():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    faces, V = grid_case()
    n3, n4, other = ref.rim_census(faces)
    print("rims of 3:", n3, "rims of 4:", n4, "other components:", other)
    assert n3 > 0 and n4 > 0 and other > 0 and n3 + n4 > 90
    e = np.asarray(ref.boundary_edges(faces))
    g = coo_matrix((np.ones(len(e)), (e[:, 0], e[:, 1])), shape=(V, V))
    _n, label = connected_components(g, directed=False)
    touched = np.unique(e)
    comps = ref.rim_components(faces)
    assert len(comps) == len(np.unique(label[touched]))
    for comp, _ok in comps:
        assert len(set(label[comp])) == 1 and (label[touched] == label[comp[0]]).sum() == len(comp)
    assert [c[0][0] for c in comps] == sorted(c[0][0] for c in comps)
    out = ref.fill_small_holes(faces)
    assert out["n_new"] == n3 + 2 * n4 and list(out["rim_of_new"]) == sorted(out["rim_of_new"])
    assert ref.rim_census(out["faces"]) == (0, 0, 1)                   # only the grid's outline is left
    d = directed_edges(out["faces"])
    assert len(set(d)) == len(d)                                       # the grid is consistently wound, and stays so


def test_areas_and_means():
    v = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [0, 0, 1]], np.float32)
    a = ref.face_areas(v, [[0, 1, 2], [0, 1, 3], [1, 1, 2]])
    assert a.dtype == np.float64 and a.tolist() == [6.0, 1.5, 0.0]
    assert ref.exact_mean([1.0, 2.0, 6.0]) == 3.0 and np.isnan(ref.exact_mean([]))
    assert ref.mean_edge_length(v, [[0, 1, 2], [0, 2, 1]]) == 4.0      # 3, 4, 5, each once


# ---------------------------------------------------------------------------------------------------- the driver
def _rotation():
    a, b = 0.3, 0.2
    return (np.array([[np.cos(a), -np.sin(a), 0], [np.sin(a), np.cos(a), 0], [0, 0, 1]])
            @ np.array([[1, 0, 0], [0, np.cos(b), -np.sin(b)], [0, np.sin(b), np.cos(b)]]))


@functools.lru_cache(maxsize=None)
def chain_case():
    """Base: a level-3 icosphere (1 280 faces) of radius 0.1; fusion: a level-4 icosphere of radius 0.101, rotated, so its
    tessellation differs everywhere; two regions, around the two poles.  -> (bv, bf, fv, ff, raw_boxes [2,2,3])."""
    s, h = 0.1, 0.3
    bv, bf = ref.icosphere(3, s)
    fv, ff = ref.icosphere(4, s * 1.01)
    fv = (fv.astype(np.float64) @ _rotation().T).astype(np.float32)
    raw = s * np.array([[[-h, -h, 0.8], [h, h, 1.2]], [[-h, -h, -1.2], [h, h, -0.8]]])
    for a in (bv, bf, fv, ff, raw):
        a.setflags(write=False)
    return bv, bf, fv, ff, raw


@functools.lru_cache(maxsize=None)
def chain_want(pad=0.02, **kw):
    bv, bf, fv, ff, raw = chain_case()
    return ref.update_mesh_topology(bv, bf, 2, rr.padded_boxes(raw, pad), fv, ff, **kw)


GAP_FACE = 1360        # a face of the fusion sphere inside the first box whose loss the stitch's own vertex merging does not heal


def test_chain_restatement():
    bv, bf, _fv, _ff, _raw = chain_case()
    want = chain_want()
    assert want["n_spliced"] == 2 and want["cc_update_num"] == 2 and sr.is_watertight(want["faces"])
    tn = want["track_face_num"]
    assert 0 < tn < len(bf) and int(want["track_face_mask"].sum()) == tn
    # the surviving input faces are the prefix, in order: the same triangles at the same positions
    ok, n_exact = ref.prefix_is_original(want["verts"], want["faces"], want["track_face_mask"], bv, bf, rr.padded_boxes(_raw, 0.02))
    assert ok and n_exact > 200
    shuffled = want["faces"].copy()
    shuffled[:tn] = shuffled[:tn][::-1]
    assert not ref.prefix_is_original(want["verts"], shuffled, want["track_face_mask"], bv, bf, rr.padded_boxes(_raw, 0.02))[0]
    assert want["new_ref_area"].dtype == np.float32 and len(want["new_ref_area"]) == len(want["faces"])
    assert len(np.unique(want["new_ref_area"][tn:])) == 1 and want["max_dist_in_connection"] > 0
    # the second box was cut from what the first left
    assert not np.array_equal(chain_want(cut_from_uncut=True)["faces"], want["faces"])
    # a region count of 0 is "nothing to update"; three regions of which the boxes were merged to two still count as three
    assert ref.update_mesh_topology(bv, bf, 0, [], _fv, _ff)["cc_update_num"] == -1
    far = np.array([[5, 5, 5], [6, 6, 6]], np.float64)
    out = ref.update_mesh_topology(bv, bf, 1, [far], _fv, _ff)
    assert out["cc_update_num"] == 0 and out["n_spliced"] == 0 and out["track_face_mask"].all()


def test_gap_restatement():
    """Without filling, the hole left by GAP_FACE keeps the stitch from being watertight and the box is skipped; with it, the
    box is spliced."""
    bv, bf, fv, ff, raw = chain_case()
    box = rr.padded_boxes(raw[:1], 0.02)[0]
    ff = np.delete(ff, GAP_FACE, axis=0)
    patch = rr.cut_mesh_by_box(fv, ff, box, False)
    assert ref.rim_census(patch["faces"])[0] == 1
    base = rr.cut_mesh_by_box(bv, bf, box, True)
    patch = sr.select_faces(patch["verts"], patch["faces"], rr.outlier_component_mask(patch["faces"], 50))
    st = sr.connect_two_meshes(base["verts"], base["faces"], rr.boundary_vertices(base["verts"], base["faces"], box, True, 0.02),
                               patch["verts"], patch["faces"], rr.boundary_vertices(patch["verts"], patch["faces"], box, False))
    assert st["watertight"] is False
    out = ref.update_mesh_topology(bv, bf, 1, [box], fv, ff)
    assert out["n_spliced"] == 1 and sr.is_watertight(out["faces"])


# ---------------------------------------------------------------------------------------------------- pads, files (no GPU)
class _Run:
    def __init__(self, cc, dist, nothing=False):
        self.cc_update_num, self.max_dist_in_connection, self.nothing_to_update = cc, dist, nothing


def _recorded(rows):
    calls = []

    def run(pad):
        calls.append(pad)
        return _Run(*rows[len(calls) - 1])
    return run, calls


def test_choose_aabb_pad():
    from gaustar_amd import regions
    pads = (0.01, 0.015, 0.02, 0.025, 0.03)
    for rows, best in (([(1, 0.5), (2, 0.25), (1, 0.25), (0, 0.01), (1, 0.3)], 0.015),      # equal scores: the first wins; cc == 0 scores 100
                       ([(0, 0.1)] * 5, 0.01),                                               # all 100
                       ([(1, 0.2), (1, 0.1), (-1, 0.0, True), (1, 0.01), (1, 0.01)], None)):   # an early nothing_to_update
        run, calls = _recorded(rows)
        got, scores = regions.choose_aabb_pad(run)
        want, want_scores = ref.choose_aabb_pad(lambda p, it=iter(rows): dict(zip(("cc_update_num", "max_dist_in_connection"), next(it)[:2])))
        assert got == best and got == want and scores == want_scores
        assert calls == list(pads[:3 if best is None else 5])
    run, _calls = _recorded([(1, 3.0), (1, 2.0)])
    assert regions.choose_aabb_pad(run, pads=(0.5, 0.25)) == (0.25, [3.0, 2.0])


def test_save_and_gaussian_mask(tmp_path):
    from gaustar_amd import formats, regions
    want = chain_want()
    t = torch.from_numpy
    upd = regions.TopologyUpdate(verts=t(want["verts"]), faces=t(want["faces"]), track_face_mask=t(want["track_face_mask"]),
                                 track_face_num=want["track_face_num"], new_ref_area=t(want["new_ref_area"]),
                                 new_area_mean=want["new_area_mean"], cc_update_num=2, n_spliced=2,
                                 max_dist_in_connection=want["max_dist_in_connection"], nothing_to_update=False)
    obj, npz = upd.save(str(tmp_path / "out"))
    assert os.path.basename(obj) == "updated_mesh.obj" and os.path.basename(npz) == "face_corr.npz"
    z = np.load(npz)
    assert sorted(z.files) == ["ref_area", "track_face_mask"]
    assert z["track_face_mask"].dtype == np.bool_ and z["track_face_mask"].shape == (1280,)
    assert z["ref_area"].dtype == np.float32 and z["ref_area"].shape == (len(want["faces"]),)
    assert np.array_equal(z["track_face_mask"], want["track_face_mask"]) and np.array_equal(z["ref_area"], want["new_ref_area"])
    v, f, _c = formats.load_obj(obj)
    assert np.array_equal(f, want["faces"]) and np.array_equal(v.astype(np.float32), want["verts"])
    g = upd.gaussian_mask(3)
    assert g.shape == (3 * 1280,) and np.array_equal(g.numpy(), np.repeat(want["track_face_mask"], 3))
    none = regions.TopologyUpdate(t(want["verts"]), t(want["faces"]), t(want["track_face_mask"]), 1280, None, float("nan"), -1, 0, 0.0, True)
    with pytest.raises(ValueError):
        none.save(str(tmp_path / "none"))
