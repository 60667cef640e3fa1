"""tests/stitch_ref.py -- the numpy restatement the GPU stitch is compared with bit for bit -- against answers written out by
hand.  No GPU."""
import numpy as np

import regions_ref
import stitch_ref as ref


def _d2(a, b):
    a, b = np.asarray(a, np.float32).astype(np.float64), np.asarray(b, np.float32).astype(np.float64)
    d = a - b
    return (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]


# ---------------------------------------------------------------------------------------------------- nearest vertex
def test_nearest_duplicate_candidate_lowest_index_wins():
    c = np.array([[5, 0, 0], [1, 0, 0], [0, 0, 0], [1, 0, 0]], np.float32)
    idx, d2 = ref.nearest_vertices(np.array([[0.9, 0, 0], [1, 0, 0]], np.float32), c)
    assert idx.tolist() == [1, 1] and idx.dtype == np.int32
    assert d2[0] == _d2([0.9, 0, 0], [1, 0, 0]) and d2[1] == 0.0 and d2.dtype == np.float64


def test_nearest_equidistant_tie_on_integer_coordinates():
    c = np.array([[2, 0, 0], [0, 0, 1], [0, 1, 0], [-1, 0, 0], [0, 0, -1]], np.float32)
    idx, d2 = ref.nearest_vertices(np.zeros((1, 3), np.float32), c)
    assert idx.tolist() == [1] and d2.tolist() == [1.0]
    idx, _ = ref.nearest_vertices(np.zeros((1, 3), np.float32), c[::-1].copy())
    assert idx.tolist() == [0]                       # (0, 0, -1) comes first now
    # -0 and +0 are one position
    idx, d2 = ref.nearest_vertices(np.array([[-0.0, 0, 0]], np.float32), np.array([[1, 0, 0], [0.0, -0.0, 0]], np.float32))
    assert idx.tolist() == [1] and d2.tolist() == [0.0]


# ---------------------------------------------------------------------------------------------------- connect_two_meshes
def _two_triangles():
    v1 = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float32)
    f1 = np.array([[0, 1, 2]], np.int32)
    v2 = np.array([[1.1, 0.05, 0], [0.05, 1.1, 0], [1, 1, 0]], np.float32)
    f2 = np.array([[0, 2, 1]], np.int32)
    return v1, f1, np.array([1, 2], np.int32), v2, f2, np.array([0, 1], np.int32)


def test_two_triangles_share_the_snapped_edge():
    args = _two_triangles()
    out = ref.connect_two_meshes(*args, max_hole_vert_num=3)       # (the 4-vertex rim stays)
    assert np.array_equal(out["verts"], np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [1, 1, 0]], np.float32))
    assert out["faces"].tolist() == [[0, 1, 2], [1, 3, 2]] and out["faces"].dtype == np.int32
    assert out["face_mask"].tolist() == [True, True]
    assert out["vert_map"].tolist() == [0, 1, 2, 1, 2, 3]
    assert out["n_faces_from_first"] == 1 and out["watertight"] is False
    assert out["max_dist"] == float(np.sqrt(_d2([1.1, 0.05, 0], [1, 0, 0])))
    # the inputs are untouched
    assert np.array_equal(args[0], _two_triangles()[0]) and np.array_equal(args[3], _two_triangles()[3])


def test_a_four_vertex_hole_merges_away():
    """The two triangles' rim is one hole of 4 vertices: with the default bound of 10 it collapses onto vertex 0 and both faces
    become degenerate."""
    out = ref.connect_two_meshes(*_two_triangles())
    assert out["faces"].shape == (0, 3) and out["verts"].shape == (0, 3)
    assert out["face_mask"].tolist() == [False, False] and out["vert_map"].tolist() == [-1] * 6
    assert out["n_faces_from_first"] == 0 and out["watertight"] is False


def test_inner_hole_of_four_merges_outer_rim_of_twelve_stays():
    verts, faces = regions_ref.quad_grid(3, 3)
    faces = np.delete(faces, [8, 9], axis=0)                      # the centre quad: its corners 5, 6, 9, 10 ring a hole
    out = ref.merge_vertices_around_holes(verts, faces)
    # 5, 6, 9, 10 -> 5: of every side quad the triangle with two of them goes
    dropped = {(1, 6, 5), (4, 5, 9), (6, 11, 10), (9, 10, 14)}
    keep = np.array([tuple(f) not in dropped for f in faces.tolist()])
    assert np.array_equal(out["face_mask"], keep) and keep.sum() == 12
    vm = np.array([0, 1, 2, 3, 4, 5, 5, 6, 7, 5, 5, 8, 9, 10, 11, 12], np.int32)
    assert np.array_equal(out["vert_map"], vm)
    assert np.array_equal(out["faces"], vm[faces[keep]])
    assert np.array_equal(out["verts"], np.delete(verts, [6, 9, 10], axis=0))


def _fan(n):
    """A centre (vertex 0) and n rim vertices: n faces, the rim a hole of n vertices."""
    a = 2 * np.pi * np.arange(n) / n
    verts = np.concatenate([np.zeros((1, 3)), np.stack([np.cos(a), np.sin(a), np.zeros(n)], 1)]).astype(np.float32)
    faces = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
    return verts, faces


def test_an_eleven_vertex_hole_stays_a_ten_vertex_hole_goes():
    verts, faces = _fan(11)
    out = ref.merge_vertices_around_holes(verts, faces)
    assert np.array_equal(out["faces"], faces) and np.array_equal(out["verts"], verts) and out["face_mask"].all()
    assert np.array_equal(out["vert_map"], np.arange(12))
    verts, faces = _fan(10)
    out = ref.merge_vertices_around_holes(verts, faces)
    assert out["faces"].shape == (0, 3) and not out["face_mask"].any() and (out["vert_map"] == -1).all()
    out = ref.merge_vertices_around_holes(verts, faces, max_hole_vert_num=9)
    assert np.array_equal(out["faces"], faces)


def test_a_hole_edge_shared_by_three_faces():
    """A closed tetrahedron and a fin on its edge (0, 1): that edge has three faces, the fin's other two edges one."""
    faces = np.array([[0, 1, 2], [0, 3, 1], [0, 2, 3], [1, 3, 2], [0, 1, 4]], np.int32)
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1], [1, 1, 1]], np.float32)
    assert sorted(regions_ref.face_edge_counts(faces).reshape(-1).tolist()) == [1, 1] + [2] * 10 + [3, 3, 3]
    hv, label = ref.hole_components(faces)
    assert hv.tolist() == [0, 1, 4] and label.tolist() == [0, 0, 0]
    out = ref.merge_vertices_around_holes(verts, faces)          # 1, 4 -> 0: the three faces on (0, 1) go
    assert out["face_mask"].tolist() == [False, False, True, True, False]
    assert out["faces"].tolist() == [[0, 1, 2], [0, 2, 1]] and out["vert_map"].tolist() == [0, 0, 1, 2, 0]
    # three caps over one triangle: its three edges have three faces each, every other edge two
    caps = np.array([[u, v, a] for a in (3, 4, 5) for u, v in ((0, 1), (1, 2), (2, 0))], np.int32)
    assert sorted(regions_ref.face_edge_counts(caps).reshape(-1).tolist()) == [2] * 18 + [3] * 9
    hv, label = ref.hole_components(caps)
    assert hv.tolist() == [0, 1, 2] and label.tolist() == [0, 0, 0]


def test_hole_components_match_scipy():
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    _verts, faces = regions_ref.quad_grid(12, 9)
    gone = [j * 12 + i for j in range(9) for i in range(12) if (i % 4 == 1 and j % 3 == 1) or (i, j) in ((6, 4), (7, 4), (7, 5))]
    faces = np.delete(faces, [2 * q + k for q in gone for k in (0, 1)], axis=0)      # separate holes of 4 and one of 8 vertices
    hv, label = ref.hole_components(faces)
    edges = np.stack([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]], 1)
    he = edges[regions_ref.face_edge_counts(faces) != 2]
    assert np.array_equal(hv, np.unique(he))
    pos = np.searchsorted(hv, he)
    n, want = connected_components(coo_matrix((np.ones(len(pos)), (pos[:, 0], pos[:, 1])), shape=(len(hv), len(hv))), directed=False)
    assert n == label.max() + 1 and n > 3
    assert np.array_equal(label, want)                           # both number by ascending lowest vertex


def test_position_groups_take_the_earliest_listed():
    verts = np.array([[1, 2, 3], [0, 0, 0], [1, 2, 3], [-0.0, 0, 0], [1, 2, 3], [np.nan, 0, 0], [np.nan, 0, 0]], np.float32)
    assert ref.position_remap(verts, [4, 3, 1, 2, 5, 6]).tolist() == [0, 3, 4, 3, 4, 5, 6]      # (vertex 0 is not listed)
    assert ref.position_remap(verts, [0, 1, 2, 3, 4]).tolist() == [0, 1, 0, 1, 0, 5, 6]


# ---------------------------------------------------------------------------------------------------- watertight, select
def test_watertight():
    _v, torus = ref.torus(6, 5)
    assert ref.is_watertight(torus) is True
    assert ref.is_watertight(regions_ref.quad_grid(4, 3)[1]) is False
    assert ref.is_watertight(np.zeros((0, 3), np.int32)) is False
    assert ref.is_watertight(torus[1:]) is False


def test_select_faces():
    verts, faces = regions_ref.quad_grid(2, 1)
    out = ref.select_faces(verts, faces, [False, False, True, False], attrs=(np.arange(6) * 10,))
    assert out["faces"].tolist() == [[0, 1, 2]] and out["vert_map"].tolist() == [-1, 0, 1, -1, -1, 2]
    assert out["attrs"][0].tolist() == [10, 20, 50] and np.array_equal(out["verts"], verts[[1, 2, 5]])
