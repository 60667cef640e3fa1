"""tests/regions_ref.py, the numpy restatement the GPU tests of gaustar_amd.regions compare with, pinned on hand-built meshes
whose answers are written out here; and the host parts of gaustar_amd.regions (the box merge, the box decoding, the size
limit).  No GPU."""
import numpy as np
import pytest

import regions_ref as rr

CUBE = lambda lo, hi: np.array([[lo] * 3, [hi] * 3], np.float64)


# ---------------------------------------------------------------------------------------------------- 1. edge multiplicity
def test_edge_counts_of_two_triangles_on_one_edge():
    faces = [(0, 1, 2), (0, 2, 3)]
    assert rr.face_edge_counts(faces).tolist() == [[1, 1, 2], [2, 1, 1]]
    assert sorted(rr.face_adjacency(faces)) == [(0, 1)]
    assert rr.face_edge_counts(faces, mask=[True, False]).tolist() == [[1, 1, 1], [0, 0, 0]]


def test_a_fan_of_three_faces_on_one_edge_links_nothing():
    faces = [(0, 1, 2), (0, 1, 3), (1, 0, 4)]
    assert rr.face_edge_counts(faces).tolist() == [[3, 1, 1]] * 3
    assert rr.face_adjacency(faces) == []
    label, count = rr.face_components(faces)
    assert label.tolist() == [0, 1, 2] and count.tolist() == [1, 1, 1]
    # with one of the three masked out the other two are adjacent (counts are taken among the masked faces)
    label, count = rr.face_components(faces, mask=[True, False, True])
    assert label.tolist() == [0, -1, 0] and count.tolist() == [2]


def test_a_degenerate_face_links_nothing_through_its_own_two_edges():
    assert rr.face_edge_counts([(0, 0, 1)]).tolist() == [[1, 2, 2]]
    assert rr.face_adjacency([(0, 0, 1)]) == []
    faces = [(0, 0, 1), (0, 1, 2)]             # edge (0, 1) now has three face-edges
    assert rr.face_edge_counts(faces).tolist() == [[1, 3, 3], [3, 1, 1]]
    label, count = rr.face_components(faces)
    assert label.tolist() == [0, 1] and count.tolist() == [1, 1]


# ---------------------------------------------------------------------------------------------------- 2. components
def test_components_are_numbered_by_their_smallest_face():
    # faces 0 and 2 share edge (0, 2), faces 1 and 3 share edge (11, 12)
    faces = [(0, 1, 2), (10, 11, 12), (0, 2, 3), (11, 13, 12)]
    label, count = rr.face_components(faces)
    assert label.tolist() == [0, 1, 0, 1] and count.tolist() == [2, 2]
    label, count = rr.face_components(faces[::-1])
    assert label.tolist() == [0, 1, 0, 1]
    label, count = rr.face_components(faces, mask=[False, True, True, True])
    assert label.tolist() == [-1, 0, 1, 0] and count.tolist() == [2, 1]


def test_two_grids_touching_in_one_vertex_are_two_components():
    va, fa = rr.quad_grid(4, 4)
    vb, fb = rr.quad_grid(4, 4, v0=len(va) - 1)       # its first vertex IS the last vertex of the first grid
    label, count = rr.face_components(np.concatenate([fa, fb]))
    assert count.tolist() == [32, 32]
    assert label.tolist() == [0] * 32 + [1] * 32


def test_a_strip_is_one_component_and_a_masked_strip_falls_apart():
    _v, f = rr.quad_grid(5, 1)
    label, count = rr.face_components(f)
    assert count.tolist() == [10] and set(label.tolist()) == {0}
    mask = np.ones(10, bool)
    mask[4] = False                                    # quad 2's first triangle
    label, count = rr.face_components(f, mask)
    # the chain runs 1-0-3-2-5-4-7-6-9-8 (a quad's first triangle meets the NEXT quad's second): face 5 stays with the head
    assert label.tolist() == [0, 0, 0, 0, -1, 0, 1, 1, 1, 1] and count.tolist() == [5, 4]


def test_components_match_scipy():
    csgraph = pytest.importorskip("scipy.sparse.csgraph")
    sparse = pytest.importorskip("scipy.sparse")
    rng = np.random.default_rng(3)
    for trial in range(20):
        V, F = int(rng.integers(4, 30)), int(rng.integers(1, 80))
        faces = rng.integers(0, V, size=(F, 3))
        mask = rng.random(F) < 0.8
        label, count = rr.face_components(faces, mask)
        ids = np.where(mask)[0]
        pos = -np.ones(F, int)
        pos[ids] = np.arange(len(ids))
        adj = np.array([(pos[a], pos[b]) for a, b in rr.face_adjacency(faces, mask)], int).reshape(-1, 2)
        g = sparse.coo_matrix((np.ones(len(adj)), (adj[:, 0], adj[:, 1])), shape=(len(ids), len(ids)))
        n, want = csgraph.connected_components(g, directed=False)
        assert n == len(count) and np.array_equal(label[mask], want)
        assert np.array_equal(count, np.bincount(want, minlength=n))


# ---------------------------------------------------------------------------------------------------- 3. / 4. selection, boxes
def _combines():
    from gaustar_amd import regions
    return [rr.combine_overlap_aabbs, regions.combine_overlap_aabbs]


@pytest.mark.parametrize("which", [0, 1])
def test_combine_first_and_third_overlap(which):
    combine = _combines()[which]
    out = combine([CUBE(0, 1), CUBE(5, 6), CUBE(0.5, 1.5)])
    assert len(out) == 2 and np.array_equal(out[0], CUBE(0, 1.5)) and np.array_equal(out[1], CUBE(5, 6))


@pytest.mark.parametrize("which", [0, 1])
def test_combine_depends_on_the_order(which):
    """Only the NEW box's corners are tested: a small box inside a big one joins it when it comes second, and stays apart
    when it comes first (no corner of the big box is inside the small one).  Touching boxes do not overlap (strict)."""
    combine = _combines()[which]
    big, small = CUBE(0, 10), CUBE(4, 5)
    out = combine([big, small])
    assert len(out) == 1 and np.array_equal(out[0], big)
    out = combine([small, big])
    assert len(out) == 2 and np.array_equal(out[0], small) and np.array_equal(out[1], big)
    assert len(combine([CUBE(0, 1), CUBE(1, 2)])) == 2
    assert combine([]) == []


@pytest.mark.parametrize("which", [0, 1])
def test_combine_chain_needs_the_recursion(which):
    """B joins A; C overlaps the merged box but is tested against A as it came in (:269), so it joins only in the second pass."""
    combine = _combines()[which]
    out = combine([CUBE(0, 1), CUBE(0.5, 2), CUBE(1.5, 3)])
    assert len(out) == 1 and np.array_equal(out[0], CUBE(0, 3))


@pytest.mark.parametrize("which", [0, 1])
def test_combine_tests_the_input_list_not_the_merged_one(which):
    """A, B, C, D: B joins A, C stands alone as merged entry 1.  D overlaps B only -- and B is entry 1 of the INPUT list, so D
    is merged into merged entry 1, which is C (:269 vs :279).  The second pass then finds that box's corner inside A + B."""
    combine = _combines()[which]
    out = combine([CUBE(0, 1), CUBE(0.5, 1.5), CUBE(10, 11), CUBE(1.2, 1.4)])
    assert len(out) == 1 and np.array_equal(out[0], CUBE(0, 11))


def test_selection_on_a_strip():
    v, f = rr.quad_grid(10, 1)                         # 20 faces
    G = 3
    rng = np.random.default_rng(0)
    pts = np.repeat(v[f].mean(1), G, axis=0).astype(np.float32)
    pts[:, 2] = rng.random(len(pts)).astype(np.float32) * 0.25 + 0.25          # the centres float above the plane
    colour = np.zeros(20, np.uint8)
    colour[0:6] = 153                                  # quads 0..2: kept (6 > 5)
    colour[8:12] = 255                                 # quads 4 and 5: 4 faces, not more than 5
    colour[14:20] = 152                                # below the cut-off
    out = rr.select_update_regions(v, f, pts, colour, G, cc_face_threshold=5)
    assert out["n_components"] == 2 and out["labels"].tolist() == [0] and out["counts"].tolist() == [6]
    assert out["region"].tolist() == [0] * 6 + [-1] * 14
    assert out["component"].tolist() == [0] * 6 + [-1, -1] + [1] * 4 + [-1] * 8
    box = out["raw_boxes"][0]
    assert box[0].tolist() == [0.0, 0.0, 0.0] and box[1, :2].tolist() == [3.0, 1.0]
    assert box[1, 2] == float(pts[:6 * G, 2].max()) and 0.25 <= box[1, 2] <= 0.5      # grown by the centres
    none = rr.select_update_regions(v, f, pts, colour, G, cc_face_threshold=6)
    assert len(none["labels"]) == 0 and none["raw_boxes"].shape == (0, 2, 3)
    merged = rr.padded_boxes(out["raw_boxes"], 0.02)
    assert merged.shape == (1, 2, 3) and merged[0, 0, 0] == -0.02 and merged[0, 1, 0] == 3.02


def test_box_decoding_inverts_the_kernels_encoding():
    from gaustar_amd import regions
    vals = np.array([0.0, 1.0, -1.0, 3.5e-38, -3.5e-38, 1e30, -1e30, np.float32(0.1), -np.float32(0.1), 2.0, -2.0, 7.0], np.float32)
    bits = vals.view(np.uint32)
    enc = np.where(bits & np.uint32(0x80000000), ~bits, bits | np.uint32(0x80000000)).astype(np.uint32)
    assert np.array_equal(np.argsort(enc, kind="stable"), np.argsort(vals, kind="stable"))       # unsigned order = float order
    back = regions._decode_boxes(enc.reshape(2, 2, 3))
    assert back.dtype == np.float64 and np.array_equal(back.reshape(-1), vals.astype(np.float64))


# ---------------------------------------------------------------------------------------------------- 5. cut
def test_cut_on_two_quads():
    v, f = rr.quad_grid(2, 1)      # vertices (0,0) (1,0) (2,0) (0,1) (1,1) (2,1); faces (0,1,4) (0,4,3) (1,2,5) (1,5,4)
    assert f.tolist() == [[0, 1, 4], [0, 4, 3], [1, 2, 5], [1, 5, 4]]
    colours = np.arange(18, dtype=np.float32).reshape(6, 3)
    box = np.array([[-0.5, -0.5, -1.0], [0.5, 0.5, 1.0]])          # vertex 0 only
    out = rr.cut_mesh_by_box(v, f, box, cut_inner=False, attrs=(colours,))
    assert out["face_mask"].tolist() == [True, True, False, False]
    assert out["vert_map"].tolist() == [0, 1, -1, 2, 3, -1]
    assert out["faces"].tolist() == [[0, 1, 3], [0, 3, 2]]
    assert np.array_equal(out["verts"], v[[0, 1, 3, 4]]) and np.array_equal(out["attrs"][0], colours[[0, 1, 3, 4]])
    out = rr.cut_mesh_by_box(v, f, box, cut_inner=True)
    assert out["face_mask"].tolist() == [False, False, True, True]
    assert out["vert_map"].tolist() == [-1, 0, 1, -1, 2, 3]
    assert out["faces"].tolist() == [[0, 1, 3], [0, 3, 2]]
    # a vertex exactly on a face of the box is outside: nothing is kept, and that is a legal result
    on = np.array([[0.0, -0.5, -1.0], [0.5, 0.5, 1.0]])
    out = rr.cut_mesh_by_box(v, f, on, cut_inner=False)
    assert out["faces"].shape == (0, 3) and out["verts"].shape == (0, 3) and not out["face_mask"].any()
    assert (out["vert_map"] == -1).all()
    # one f32 ulp inside a float64 bound is inside
    v2 = v.copy()
    v2[0, 0] = np.nextafter(np.float32(0.25), np.float32(1))
    ulp = np.array([[0.25, -0.5, -1.0], [0.5, 0.5, 1.0]])
    assert rr.cut_mesh_by_box(v2, f, ulp, cut_inner=False)["face_mask"].tolist() == [True, True, False, False]
    v2[0, 0] = np.float32(0.25)
    assert not rr.cut_mesh_by_box(v2, f, ulp, cut_inner=False)["face_mask"].any()


# ---------------------------------------------------------------------------------------------------- 6. / 7. primitives
def test_boundary_vertices_on_two_quads_and_a_fan():
    v, f = rr.quad_grid(2, 1)
    assert rr.boundary_vertices(v, f).tolist() == [0, 1, 2, 3, 4, 5]
    box = np.array([[-0.5, -0.5, -1.0], [0.5, 0.5, 1.0]])          # vertex 0 only
    # cut_inner=False: boundary vertices on faces that straddle the box: faces 0 and 1 -> vertices 0, 1, 3, 4
    assert rr.boundary_vertices(v, f, box, cut_inner=False).tolist() == [0, 1, 3, 4]
    # cut_inner=True: boundary vertices inside the box grown by pad: 0.5 + 0.6 > 1 takes in vertices 1, 3 and 4
    assert rr.boundary_vertices(v, f, box, cut_inner=True, pad=0.02).tolist() == [0]
    assert rr.boundary_vertices(v, f, box, cut_inner=True, pad=0.6).tolist() == [0, 1, 3, 4]
    # an edge of three faces is no boundary edge: vertices 0 and 1 are still on the fan's outer edges, so close it up
    fan = [(0, 1, 2), (0, 1, 3), (1, 0, 4)]
    vf = np.zeros((5, 3), np.float32)
    assert rr.boundary_vertices(vf, fan).tolist() == [0, 1, 2, 3, 4]
    tetra = [(0, 1, 2), (0, 3, 1), (1, 3, 2), (2, 3, 0)]           # closed: no boundary
    assert rr.boundary_vertices(vf, tetra).tolist() == []
    # the closed tetrahedron plus a third face on edge (0, 1): the edge has count 3 and the new face's other two edges are
    # boundary edges -- vertices 0, 1 and 4 come from THOSE, and a lone count-3 edge would give nothing
    assert rr.boundary_vertices(vf, tetra + [(0, 1, 4)]).tolist() == [0, 1, 4]
    assert rr.face_edge_counts(tetra + [(0, 1, 4)])[4].tolist() == [3, 1, 1]


def test_outlier_component_mask():
    _va, fa = rr.quad_grid(5, 1)                # 10 faces
    _vb, fb = rr.quad_grid(1, 1, v0=100)        # 2 faces
    _vc, fc = rr.quad_grid(2, 1, v0=200)        # 4 faces
    f = np.concatenate([fa, fb, fc])
    assert rr.outlier_component_mask(f).tolist() == [True] * 10 + [False] * 2 + [True] * 4           # bound 3.0
    assert rr.outlier_component_mask(f, 50).tolist() == [True] * 10 + [False] * 2 + [True] * 4       # min(50, 3.0)
    assert rr.outlier_component_mask(f, 1).all()
    assert rr.outlier_component_mask(np.zeros((0, 3), int)).shape == (0,)


# ---------------------------------------------------------------------------------------------------- limits
def test_too_many_faces_is_a_value_error():
    import torch
    from gaustar_amd import regions
    assert regions.MAX_FACES == (2 ** 31 - 1) // 3
    huge = torch.empty((regions.MAX_FACES + 1, 3), dtype=torch.int32, device="meta")
    for call in (lambda: regions.face_edge_counts(huge), lambda: regions.face_components(huge),
                 lambda: regions.outlier_component_mask(huge)):
        with pytest.raises(ValueError, match="2\\^31 / 3"):
            call()
