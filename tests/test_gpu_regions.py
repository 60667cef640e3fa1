"""gaustar_amd.regions on the GPU against the numpy restatement tests/regions_ref.py (itself pinned by tests/test_regions.py).
Every output is an integer or an exactly defined float, so every comparison is exact: np.array_equal, floats by their bits.
No tolerances."""
import types

import numpy as np
import pytest
import torch

import regions_ref as rr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _n(t):
    return t.cpu().numpy()


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def _check_components(faces, mask=None):
    from gaustar_amd import regions
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    m = None if mask is None else _t(np.asarray(mask, bool))
    counts = _n(regions.face_edge_counts(_t(faces), m))
    label, count = regions.face_components(_t(faces), m)
    want_label, want_count = rr.face_components(faces, mask)
    assert counts.dtype == np.int32 and np.array_equal(counts, rr.face_edge_counts(faces, mask))
    assert label.dtype == torch.int32 and count.dtype == torch.int32
    assert np.array_equal(_n(label), want_label) and np.array_equal(_n(count), want_count)
    return _n(label), _n(count)


def _check_cut(verts, faces, box, cut_inner, attrs=()):
    from gaustar_amd import regions
    got = regions.cut_mesh_by_box(_t(verts), _t(faces), box, cut_inner, attrs=tuple(_t(a) for a in attrs))
    want = rr.cut_mesh_by_box(verts, faces, box, cut_inner, attrs=attrs)
    assert got.faces.dtype == torch.int32 and got.vert_map.dtype == torch.int32 and got.face_mask.dtype == torch.bool
    assert np.array_equal(_n(got.faces), want["faces"]) and np.array_equal(_n(got.face_mask), want["face_mask"])
    assert np.array_equal(_n(got.vert_map), want["vert_map"]) and _same_bits(_n(got.verts), want["verts"])
    assert len(got.attrs) == len(attrs)
    for g, w in zip(got.attrs, want["attrs"]):
        assert _same_bits(_n(g), w)
    return got


def _strip_chain(n_quads):
    """The order in which the faces of rr.quad_grid(n, 1) hang together: 1-0-3-2-5-4-..."""
    return [q * 2 + k for q in range(n_quads) for k in (1, 0)]


# ---------------------------------------------------------------------------------------------------- adjacency edge cases
def test_hand_built_adjacency_cases(hip_lib):
    va, fa = rr.quad_grid(4, 4)
    _vb, fb = rr.quad_grid(4, 4, v0=len(va) - 1)                      # two grids that touch in one vertex only
    label, count = _check_components(np.concatenate([fa, fb]))
    assert count.tolist() == [32, 32] and label.tolist() == [0] * 32 + [1] * 32
    label, count = _check_components([(0, 1, 2), (0, 1, 3), (1, 0, 4)])   # a fan of three faces on one edge
    assert label.tolist() == [0, 1, 2] and count.tolist() == [1, 1, 1]
    label, count = _check_components([(0, 1, 2), (0, 1, 3), (1, 0, 4)], mask=[True, False, True])
    assert label.tolist() == [0, -1, 0] and count.tolist() == [2]
    label, count = _check_components([(0, 0, 1)])                     # a degenerate face
    assert label.tolist() == [0] and count.tolist() == [1]
    label, count = _check_components([(0, 0, 1), (0, 1, 2), (5, 5, 5)])
    assert label.tolist() == [0, 1, 2]
    label, count = _check_components([(0, 1, 2), (10, 11, 12), (0, 2, 3), (11, 13, 12)], mask=[False, True, True, True])
    assert label.tolist() == [-1, 0, 1, 0] and count.tolist() == [2, 1]


@pytest.mark.parametrize("F", [0, 1, 63, 64, 65, 257])
def test_sizes_around_the_wave_and_the_block(hip_lib, F):
    rng = np.random.default_rng(F)
    _v, strip = rr.quad_grid(max(F // 2, 1), 1)
    faces = np.concatenate([strip[:F // 2], rng.integers(0, F // 3 + 3, size=(F - F // 2, 3)).astype(np.int32) + 10_000]).astype(np.int32)
    faces = faces[rng.permutation(F)] if F else faces.reshape(0, 3)
    _check_components(faces)
    _check_components(faces, rng.random(F) < 0.7)
    from gaustar_amd import regions
    assert np.array_equal(_n(regions.outlier_component_mask(_t(faces), 3)), rr.outlier_component_mask(faces, 3))


# ---------------------------------------------------------------------------------------------------- long chains
@pytest.fixture(scope="module")
def shuffled_strip():
    """A 1 x 700 quad strip, 1 400 faces, in a seeded random face order: the smallest face sits mid-strip and the paths to it
    cross many workgroups.  (verts, faces, position of every face along the strip's chain)."""
    v, f = rr.quad_grid(700, 1)
    perm = np.random.default_rng(7).permutation(len(f))
    where = np.empty(len(f), int)
    where[np.asarray(_strip_chain(700))] = np.arange(len(f))          # original face -> position in the chain
    return v, f[perm], where[perm]


def test_long_chain_is_one_component(hip_lib, shuffled_strip):
    _v, f, _where = shuffled_strip
    label, count = _check_components(f)
    assert count.tolist() == [1400] and not label.any()


def test_components_of_exactly_80_and_81_faces(hip_lib, shuffled_strip):
    from gaustar_amd import regions
    v, f, where = shuffled_strip
    colour = np.zeros(len(f), np.uint8)
    colour[(where >= 100) & (where < 180)] = 255                      # 80 faces in a row along the chain
    colour[(where >= 181) & (where < 262)] = 200                      # 81 faces, one face apart
    pts = v[f].mean(1).astype(np.float32)
    got = regions.select_update_regions(_t(v), _t(f), _t(pts), _t(colour), 1)
    want = rr.select_update_regions(v, f, pts, colour, 1)
    assert sorted(rr.face_components(f, colour >= 153)[1].tolist()) == [80, 81]
    assert got.n_components == 2 and got.n_regions == 1 and got.counts.tolist() == [81] and not got.nothing_to_update
    assert np.array_equal(got.labels, want["labels"]) and np.array_equal(_n(got.component), want["component"])
    assert np.array_equal(_n(got.region), want["region"]) and _same_bits(got.raw_boxes, want["raw_boxes"])
    assert np.array_equal(_n(got.region) >= 0, (where >= 181) & (where < 262))


def test_flatten_leaves_every_face_at_its_components_smallest_face(hip_lib):
    """40 strips of 70 faces with their faces shuffled into one another: every component's root has other components' roots
    on both sides of it, so a parent left at an ancestor that is not the root would pick up another component's label.
    After the flatten pass parent[parent[f]] == parent[f] and parent[f] is the smallest face of f's component, on every call."""
    from gaustar_amd import regions
    strips = [rr.quad_grid(35, 1, v0=1000 * k)[1] for k in range(40)]
    faces = np.concatenate(strips)[np.random.default_rng(13).permutation(40 * 70)].astype(np.int32)
    mask = np.random.default_rng(14).random(len(faces)) < 0.9
    for m in (None, mask):
        want_label, want_count = rr.face_components(faces, m)
        on = np.ones(len(faces), bool) if m is None else m
        smallest = np.arange(len(faces))
        for lab in range(len(want_count)):
            smallest[want_label == lab] = np.where(want_label == lab)[0].min()
        for _call in range(3):
            err = torch.zeros(1, dtype=torch.int32, device=DEV)
            label, count, n, parent = regions._components(_t(faces), None if m is None else _t(m).view(torch.uint8), None, 0, err)
            parent = _n(parent).astype(np.int64)
            assert int(err.cpu()) == 0 and int(n.cpu()) == len(want_count)
            assert np.array_equal(parent[parent], parent)
            assert np.array_equal(parent[on], smallest[on]) and np.array_equal(parent[~on], np.arange(len(faces))[~on])
            assert np.array_equal(_n(label), want_label) and np.array_equal(_n(count)[:len(want_count)], want_count)


# ---------------------------------------------------------------------------------------------------- selection
def test_selection_cut_off_and_boxes(hip_lib):
    from gaustar_amd import regions
    v, f = rr.quad_grid(10, 1)
    v = v - np.float32(1.5)                                           # (negative and zero coordinates among the bounds)
    G = 3
    rng = np.random.default_rng(0)
    pts = np.repeat(v[f].mean(1), G, axis=0).astype(np.float32)
    pts[:, 2] += rng.random(len(pts)).astype(np.float32) * 0.25 + 0.25     # the centres float above the vertices' plane
    colour = np.zeros(20, np.uint8)
    colour[0:6] = 153                                                 # at the cut-off: 153 >= 255 * 0.6
    colour[8:12] = 255
    colour[14:20] = 152                                               # one below
    got = regions.select_update_regions(_t(v), _t(f), _t(pts), _t(colour), G, cc_face_threshold=5)
    want = rr.select_update_regions(v, f, pts, colour, G, cc_face_threshold=5)
    assert got.n_components == want["n_components"] == 2 and got.n_regions == 1
    assert np.array_equal(got.labels, want["labels"]) and np.array_equal(got.counts, want["counts"]) and got.counts.tolist() == [6]
    assert np.array_equal(_n(got.component), want["component"]) and np.array_equal(_n(got.region), want["region"])
    assert got.raw_boxes.dtype == np.float64 and _same_bits(got.raw_boxes, want["raw_boxes"])
    assert got.raw_boxes[0, 1, 2] > v[:, 2].max()                     # the box grew beyond the vertices
    for pad in (0.0, 0.02, 0.05):
        assert _same_bits(got.boxes(pad), rr.padded_boxes(want["raw_boxes"], pad))
    # 6 faces are not MORE than 6; and nothing above the cut-off at all
    none = regions.select_update_regions(_t(v), _t(f), _t(pts), _t(colour), G, cc_face_threshold=6)
    assert none.nothing_to_update and none.n_regions == 0 and none.n_components == 2 and none.raw_boxes.shape == (0, 2, 3)
    assert none.boxes(0.02).shape == (0, 2, 3) and (_n(none.region) == -1).all()
    low = regions.select_update_regions(_t(v), _t(f), _t(pts), _t(np.full(20, 152, np.uint8)), G, cc_face_threshold=0)
    assert low.nothing_to_update and low.n_components == 0 and (_n(low.component) == -1).all()
    # a NaN among a kept region's coordinates has no box: ValueError, as for a bad index (numpy's min / max would answer NaN)
    bad = pts.copy()
    bad[2, 1] = np.nan
    with pytest.raises(ValueError, match="NaN"):
        regions.select_update_regions(_t(v), _t(f), _t(bad), _t(colour), G, cc_face_threshold=5)
    bad = pts.copy()
    bad[-1, 1] = np.nan                                               # (a face of no kept region: not looked at)
    assert regions.select_update_regions(_t(v), _t(f), _t(bad), _t(colour), G, cc_face_threshold=5).n_regions == 1
    # every face its own region's worth: threshold 0 keeps both components, in label order
    both = regions.select_update_regions(_t(v), _t(f), _t(pts), _t(colour), G, cc_face_threshold=0)
    want = rr.select_update_regions(v, f, pts, colour, G, cc_face_threshold=0)
    assert both.n_regions == 2 and both.counts.tolist() == [6, 4] and _same_bits(both.raw_boxes, want["raw_boxes"])
    assert np.array_equal(_n(both.region), want["region"])


# ---------------------------------------------------------------------------------------------------- cut
def test_cut_edge_cases(hip_lib):
    v, f = rr.quad_grid(2, 1)
    colours = np.arange(18, dtype=np.float32).reshape(6, 3)
    box = np.array([[-0.5, -0.5, -1.0], [0.5, 0.5, 1.0]])
    got = _check_cut(v, f, box, False, attrs=(colours,))
    assert _n(got.faces).tolist() == [[0, 1, 3], [0, 3, 2]] and _n(got.vert_map).tolist() == [0, 1, -1, 2, 3, -1]
    got = _check_cut(v, f, box, True, attrs=(colours,))
    assert _n(got.faces).tolist() == [[0, 1, 3], [0, 3, 2]] and _n(got.vert_map).tolist() == [-1, 0, 1, -1, 2, 3]
    # a vertex exactly on a face of the box is outside: an empty result
    on = np.array([[0.0, -0.5, -1.0], [0.5, 0.5, 1.0]])
    got = _check_cut(v, f, on, False, attrs=(colours,))
    assert got.faces.shape == (0, 3) and got.verts.shape == (0, 3) and got.attrs[0].shape == (0, 3) and not got.face_mask.any()
    assert _n(_check_cut(v, f, on, True).face_mask).all()
    # an f32 coordinate one ulp inside a float64 bound / exactly on it
    ulp = np.array([[0.25, -0.5, -1.0], [0.5, 0.5, 1.0]])
    v2 = v.copy()
    v2[0, 0] = np.nextafter(np.float32(0.25), np.float32(1))
    assert _n(_check_cut(v2, f, ulp, False).face_mask).tolist() == [True, True, False, False]
    v2[0, 0] = np.float32(0.25)
    assert not _n(_check_cut(v2, f, ulp, False).face_mask).any()
    # a float64 bound between two f32 values: 0.1 (double) < float32(0.1)
    v2[0, 0] = np.float32(0.1)
    assert _n(_check_cut(v2, f, np.array([[0.1, -0.5, -1.0], [0.5, 0.5, 1.0]]), False).face_mask).tolist() == [True, True, False, False]
    # empty meshes
    _check_cut(np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32), box, False)
    _check_cut(v, np.zeros((0, 3), np.int32), box, True)


@pytest.mark.parametrize("cut_inner", [False, True])
def test_cut_sizes_off_the_wave_with_attrs(hip_lib, cut_inner):
    from gaustar_amd import scene
    v, f = scene.icosphere(2)                                         # V = 162, F = 320
    v, f = v.astype(np.float32)[:, :], f.astype(np.int32)[:317]       # F = 317
    rng = np.random.default_rng(5)
    f = f[rng.permutation(len(f))]
    attrs = (rng.random((len(v), 3)).astype(np.float32), rng.integers(0, 99, size=(len(v), 4)).astype(np.int32),
             rng.random(len(v)).astype(np.float32), rng.random((len(v), 2, 5)).astype(np.float32))
    for box in (np.array([[-0.3, 0.2, -2.0], [2.0, 2.0, 0.4]]), np.array([[-2.0, -2.0, -2.0], [2.0, 2.0, 2.0]]),
                np.array([[0.99, 0.99, 0.99], [1.0, 1.0, 1.0]])):
        got = _check_cut(v, f, box, cut_inner, attrs=attrs)
        assert got.attrs[1].dtype == torch.int32 and got.attrs[3].shape[1:] == (2, 5)


def test_bad_vertex_index_is_a_value_error(hip_lib):
    from gaustar_amd import regions
    v = np.zeros((3, 3), np.float32)
    box = np.array([[-1.0] * 3, [1.0] * 3])
    for faces in ([(0, 1, 5)], [(0, -1, 2)]):
        with pytest.raises(ValueError, match="vertex index"):
            regions.cut_mesh_by_box(_t(v), _t(np.asarray(faces, np.int32)), box, False)
        with pytest.raises(ValueError, match="vertex index"):
            regions.boundary_vertices(_t(v), _t(np.asarray(faces, np.int32)))
    with pytest.raises(ValueError, match="vertex index"):
        regions.face_components(_t(np.asarray([(0, -1, 2)], np.int32)))


# ---------------------------------------------------------------------------------------------------- boundary, outliers
@pytest.fixture(scope="module")
def sphere():
    from gaustar_amd import scene
    v, f = scene.icosphere(3, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)      # 1 280 faces, 642 vertices
    return v.astype(np.float32), f.astype(np.int32), np.asarray(scene.SUBJECT_CENTER, np.float64), float(scene.SUBJECT_RADIUS)


def test_boundary_vertices_and_outlier_mask_on_the_icosphere(hip_lib, sphere):
    from gaustar_amd import regions
    v, f, c, r = sphere
    bv = lambda faces, *a, **k: _n(regions.boundary_vertices(_t(v), _t(faces), *a, **k))
    got = bv(f)
    assert got.dtype == np.int32 and got.shape == (0,)                # closed
    up = (v[f].mean(1)[:, 1] - c[1]) / r                              # the face centroid's height, -1 .. 1
    opened = f[up < 0.8]                                              # the top cap removed
    ring = bv(opened)
    assert len(ring) > 8 and np.array_equal(ring, rr.boundary_vertices(v, opened))
    # a box around the upper half: its lower face cuts through the sphere, its upper part holds the ring
    box = np.array([c - [2 * r, 0.0, 2 * r], c + [2 * r, 2 * r, 2 * r]])
    for cut_inner in (False, True):
        for pad in (0.02, 0.3):
            assert np.array_equal(bv(opened, box, cut_inner, pad), rr.boundary_vertices(v, opened, box, cut_inner, pad))
    assert np.array_equal(bv(opened, box, True), ring) and len(bv(opened, box, False)) == 0
    # a box whose faces cross the ring
    half = np.array([c - [2 * r, 2 * r, 2 * r], c + [0.0, 2 * r, 2 * r]])
    for cut_inner in (False, True):
        got = bv(opened, half, cut_inner, 0.01)
        assert 0 < len(got) < len(ring) and np.array_equal(got, rr.boundary_vertices(v, opened, half, cut_inner, 0.01))
    # a third face on an edge of the closed sphere: that edge has count 3 and is no boundary edge; the new face's other two are
    a, b = int(f[0, 0]), int(f[0, 1])
    extra = np.concatenate([f, [[a, b, len(v) - 1]]]).astype(np.int32)
    far = len(v) - 1
    assert far not in f[0] and np.array_equal(bv(extra), rr.boundary_vertices(v, extra)) and bv(extra).tolist() == sorted({a, b, far})
    assert _n(regions.face_edge_counts(_t(extra)))[-1].tolist() == [3, 1, 1]
    # the band 0.55 <= up < 0.8 removed: the cap and the body are two components
    two = f[(up < 0.55) | (up >= 0.8)]
    label, count = rr.face_components(two)
    assert len(count) == 2 and count.min() < 0.3 * count.max()
    for thr in (None, 50, int(count.min()), int(count.min()) + 1, 1):
        got = regions.outlier_component_mask(_t(two), thr)
        assert got.dtype == torch.bool and np.array_equal(_n(got), rr.outlier_component_mask(two, thr))
    assert _n(regions.outlier_component_mask(_t(two), int(count.min()))).all()
    assert _n(regions.outlier_component_mask(_t(two))).sum() == count.max()


# ---------------------------------------------------------------------------------------------------- determinism, invariance
def test_two_calls_give_the_same_bits_and_a_permutation_permutes(hip_lib, sphere):
    from gaustar_amd import regions
    v, f, c, r = sphere
    rng = np.random.default_rng(11)
    G = 2
    up = (v[f].mean(1)[:, 1] - c[1]) / r
    colour = np.where(np.abs(up) > 0.75, 255, np.where(np.abs(up) < 0.1, 160, 0)).astype(np.uint8)   # two caps and a belt
    pts = (np.repeat(v[f].mean(1), G, axis=0) + rng.normal(size=(len(f) * G, 3)) * 0.01).astype(np.float32)
    box = np.array([c - [2 * r, 2 * r, 2 * r], c + [2 * r, 0.3 * r, 0.2 * r]])

    def run(faces, colour, pts):
        sel = regions.select_update_regions(_t(v), _t(faces), _t(pts), _t(colour), G, cc_face_threshold=20)
        label, count = regions.face_components(_t(faces), _t(colour > 100))
        cut = regions.cut_mesh_by_box(_t(v), _t(faces), box, False, attrs=(_t(v),))
        return dict(component=_n(sel.component), region=_n(sel.region), labels=sel.labels, counts=sel.counts, raw=sel.raw_boxes,
                    boxes=sel.boxes(0.02), label=_n(label), count=_n(count), edge=_n(regions.face_edge_counts(_t(faces))),
                    cv=_n(cut.verts), cf=_n(cut.faces), cm=_n(cut.face_mask), cmap=_n(cut.vert_map), ca=_n(cut.attrs[0]),
                    bv=_n(regions.boundary_vertices(_t(v), _t(faces[colour > 100]))), out=_n(regions.outlier_component_mask(_t(faces[colour > 100]))))

    one, two = run(f, colour, pts), run(f, colour, pts)
    for k in one:
        assert _same_bits(one[k], two[k]), k
    assert len(one["labels"]) == 3

    perm = rng.permutation(len(f))
    moved = run(f[perm], colour[perm], pts.reshape(len(f), G, 3)[perm].reshape(-1, 3))
    want = rr.select_update_regions(v, f[perm], pts.reshape(len(f), G, 3)[perm].reshape(-1, 3), colour[perm], G, cc_face_threshold=20)
    assert np.array_equal(moved["region"], want["region"]) and _same_bits(moved["raw"], want["raw_boxes"])
    # the same partition: the pairs (label before, label after) of a face are a bijection between the label sets
    pairs = {(int(a), int(b)) for a, b in zip(one["component"][perm], moved["component"])}
    assert len(pairs) == len({a for a, _ in pairs}) == len({b for _, b in pairs})
    assert np.array_equal(moved["region"] >= 0, (one["region"] >= 0)[perm])                       # the same faces are kept
    assert sorted(moved["counts"].tolist()) == sorted(one["counts"].tolist())
    key = lambda b: sorted(map(bytes, np.ascontiguousarray(b).reshape(len(b), -1)))
    assert key(moved["raw"]) == key(one["raw"])                                                   # the same boxes, in another order at most
    assert np.array_equal(moved["cm"], one["cm"][perm]) and _same_bits(moved["cv"], one["cv"]) and np.array_equal(moved["cmap"], one["cmap"])
    assert np.array_equal(moved["edge"], one["edge"][perm])


# ---------------------------------------------------------------------------------------------------- end to end
def test_end_to_end_on_a_surface_gaussians_model(hip_lib, sphere):
    from gaustar_amd import fusion, harness, regions, scene
    v, f, c, r = sphere
    model = harness.SurfaceGaussians(_t(v), _t(f, torch.long), n_gaussians_per_surface_triangle=6, sh_levels=2)
    d = (v[f].mean(1) - c) / r                                        # unit-ish direction of every face
    colour = np.zeros(len(f), np.uint8)
    colour[d[:, 1] > 0.8] = 255                                       # two caps of more than 80 faces ...
    colour[d[:, 1] < -0.8] = 255
    colour[d[:, 0] > 0.95] = 255                                      # ... and one of fewer
    sizes = sorted(rr.face_components(f, colour == 255)[1].tolist())
    assert len(sizes) == 3 and sizes[0] < 80 < sizes[1]
    res = types.SimpleNamespace(face_colour=_t(colour))
    found = model.topology_update_regions(res)
    with torch.no_grad():
        pts = _n(model.points.detach())
    want = rr.select_update_regions(v, f, pts, colour, 6)
    assert isinstance(found, regions.UpdateRegions) and found.n_regions == 2 and found.n_components == 3
    assert np.array_equal(found.counts, want["counts"]) and np.array_equal(_n(found.region), want["region"])
    assert _same_bits(found.raw_boxes, want["raw_boxes"])

    fv, ff = scene.icosphere(4, r * 1.01, tuple(c))                   # 5 120 faces standing in for the fused surface
    fv, ff = fv.astype(np.float32), ff.astype(np.int32)
    fc = np.random.default_rng(2).random((len(fv), 3)).astype(np.float32)
    mesh = fusion.FusionMesh(verts=_t(fv), faces=_t(ff), colors=_t(fc), n_blocks=0, n_views=0)
    for pad in (0.02, 0.05):
        cuts = model.cut_update_regions(found, mesh, aabb_pad=pad)
        boxes = rr.padded_boxes(want["raw_boxes"], pad)
        assert len(cuts) == len(boxes) == 2
        for cut, box in zip(cuts, boxes):
            assert _same_bits(cut.box, box)
            patch = rr.cut_mesh_by_box(fv, ff, box, False, attrs=(fc,))
            base = rr.cut_mesh_by_box(v, f, box, True)
            assert 0 < len(patch["faces"]) < len(ff) and 0 < len(base["faces"]) < len(f)
            for got, ref in ((cut.fusion_patch, patch), (cut.base_cut, base)):
                assert _same_bits(_n(got.verts), ref["verts"]) and np.array_equal(_n(got.faces), ref["faces"])
                assert np.array_equal(_n(got.face_mask), ref["face_mask"]) and np.array_equal(_n(got.vert_map), ref["vert_map"])
            assert _same_bits(_n(cut.fusion_patch.attrs[0]), patch["attrs"][0]) and cut.base_cut.attrs == ()
    nothing = model.topology_update_regions(types.SimpleNamespace(face_colour=_t(np.zeros(len(f), np.uint8))))
    assert nothing.nothing_to_update and model.cut_update_regions(nothing, mesh) == []
