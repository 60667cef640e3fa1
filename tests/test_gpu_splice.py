"""fill_small_holes, face_areas, update_mesh_topology and the pad trials of gaustar_amd.regions on the GPU against the numpy
restatement tests/splice_ref.py (itself pinned by tests/test_splice.py).  Every integer output and every mask is compared bit
for bit.  new_ref_area is the one exception: an f64 sqrt that is a few f64 ulps off can move an f32 rounding by at most one f32
ulp, so its entries are compared within 1 f32 ulp; the f64 mean of n areas is compared with the correctly rounded mean within a
relative n 2^-53, the bound of any summation order over positive terms.

Largest deviations seen on an MI355X (printed by the tests): see NOTEBOOK.md."""
import functools

import numpy as np
import pytest
import torch

import regions_ref as rr
import splice_ref as ref
from test_splice import CUBE, GAP_FACE, TETRA, chain_case, chain_want, flipped_quad_case, grid_case

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))          # (a copy: the shared inputs are read-only)
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _n(t):
    return t.cpu().numpy()


def _check_fill(faces, V):
    """fill_small_holes on the GPU equals the restatement; the input is not modified.  -> (got, want)."""
    from gaustar_amd import regions
    faces = np.asarray(faces, np.int32).reshape(-1, 3)
    tf = _t(faces)
    before = tf.clone()
    got = regions.fill_small_holes(tf, V)
    assert torch.equal(tf, before)
    want = ref.fill_small_holes(faces)
    assert got.faces.dtype == torch.int32 and got.rim_of_new.dtype == torch.int32
    assert got.n_new == want["n_new"] and tuple(got.faces.shape) == (len(faces) + want["n_new"], 3)
    assert np.array_equal(_n(got.faces), want["faces"]), (_n(got.faces)[len(faces):], want["faces"][len(faces):])
    assert np.array_equal(_n(got.rim_of_new), want["rim_of_new"]) and got.watertight is want["watertight"]
    return got, want


def _ulps_f32(a, b):
    """The distance of two f32 arrays in units in the last place (both finite, same sign or zero)."""
    ia, ib = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return np.abs(ia - ib)


# ---------------------------------------------------------------------------------------------------- the rule
def test_triangle_hole():
    for k in range(4):
        got, _want = _check_fill(np.delete(TETRA, k, axis=0), 4)
        f = _n(got.faces)
        d = [(int(t[e]), int(t[(e + 1) % 3])) for t in f for e in range(3)]
        assert got.n_new == 1 and got.watertight and len(set(d)) == len(d)
        assert _n(got.rim_of_new).tolist() == [int(TETRA[k].min())]


@pytest.mark.parametrize("corner", range(4))
def test_quad_hole(corner):
    ring = [0, 2, 3, 1]
    perm = np.arange(8)
    low = ring[corner]
    perm[[0, low]] = perm[[low, 0]]
    got, _want = _check_fill(perm[CUBE[2:]], 8)
    A, B = _n(got.faces)[-2:]
    new_ring = [int(perm[r]) for r in ring]
    opposite = new_ring[(new_ring.index(0) + 2) % 4]
    assert got.n_new == 2 and got.watertight and set(A.tolist()) & set(B.tolist()) == {0, opposite}


def test_rims_that_stay():
    _v, f = ref.icosahedron()
    fan = f[(f != 0).all(axis=1)]
    got, _want = _check_fill(fan, 12)
    assert got.n_new == 0 and tuple(got.rim_of_new.shape) == (0,) and np.array_equal(_n(got.faces), fan)
    two = np.array([t for t in f.tolist() if t not in ([0, 11, 5], [0, 1, 7])], np.int32)
    assert _check_fill(two, 12)[0].n_new == 0
    fin = np.concatenate([TETRA[1:], [[1, 2, 9]]]).astype(np.int32)
    assert _check_fill(fin, 10)[0].n_new == 2
    fins = np.concatenate([fin, [[2, 1, 8]]]).astype(np.int32)            # the edge 1-2 has three faces: not a boundary edge
    assert _check_fill(fins, 10)[0].n_new == 0


def test_lone_triangle():
    got, _want = _check_fill([[4, 2, 7]], 9)
    assert _n(got.faces).tolist() == [[4, 2, 7], [2, 4, 7]] and got.watertight


def test_winding_rule():
    """One face next to the quad hole is flipped: A is reversed, B is not.  An emit pass that tests the wrong edge, or that
    reverses B whenever it reverses A, gives other faces (the restatement's two wrong variants)."""
    faces = flipped_quad_case()
    got, want = _check_fill(faces, 8)
    assert _n(got.faces)[-2:].tolist() == [[0, 3, 1], [3, 2, 0]]
    for wrong in (dict(tie_windings=True), dict(test_second_edge=True)):
        assert not np.array_equal(ref.fill_small_holes(faces, **wrong)["faces"], _n(got.faces))


def test_many_rims_across_workgroups():
    from gaustar_amd import regions
    faces, V = grid_case()
    n3, n4, other = ref.rim_census(faces)
    print("rims of 3:", n3, "rims of 4:", n4, "other components:", other)
    assert n3 > 0 and n4 > 0 and other > 0
    got, want = _check_fill(faces, V)
    assert got.n_new == n3 + 2 * n4
    again = regions.fill_small_holes(_t(np.asarray(faces)), V)
    assert torch.equal(again.faces, got.faces) and torch.equal(again.rim_of_new, got.rim_of_new)


def test_bad_index_empty_and_closed():
    from gaustar_amd import _lib, regions
    bad = np.concatenate([TETRA[1:], [[1, 2, 4]]]).astype(np.int32)      # vertex 4 of a mesh of 4 vertices
    with pytest.raises(ValueError):
        regions.fill_small_holes(_t(bad), 4)
    with pytest.raises(ValueError):
        regions.fill_small_holes(_t(np.array([[0, -1, 2]], np.int32)), 4)
    with pytest.raises(ValueError):
        regions.face_areas(_t(np.zeros((4, 3), np.float32)), _t(bad))
    # the err word itself, and that the face is left out: the other three faces' hole is still found
    lib = _lib.load()
    p, st = _lib.ptr, torch._C._cuda_getCurrentRawStream(DEV.index)
    tf = _t(bad)
    err = torch.zeros(1, dtype=torch.int32, device=DEV)
    counts = _t(rr.face_edge_counts(bad))
    F, V = 4, 4
    pairs = torch.empty(3 * F, 2, dtype=torch.int32, device=DEV)
    on = torch.empty(V, dtype=torch.uint8, device=DEV)
    degree, parent, flag = (torch.empty(V, dtype=torch.int32, device=DEV) for _ in range(3))
    slots = torch.empty(V, 2, dtype=torch.int32, device=DEV)
    _lib.check(lib.gsr_splice_rim_edges(F, V, p(tf), p(counts), p(pairs), p(on), p(degree), p(slots), p(parent), p(flag), p(err), st), "rim_edges")
    assert int(err.cpu()) == 1
    assert _n(pairs)[9:].tolist() == [[-1, -1]] * 3                       # the bad face gives no pair
    assert _n(degree).tolist() == [2, 1, 1, 0]                            # 1-0 and 0-2 only: the edge 1-2 is shared with the bad face
    # F == 0 and a closed mesh return the input
    none = regions.fill_small_holes(_t(np.zeros((0, 3), np.int32)), 5)
    assert none.n_new == 0 and tuple(none.faces.shape) == (0, 3) and none.watertight is False
    got, _want = _check_fill(CUBE, 8)
    assert got.n_new == 0 and got.watertight and np.array_equal(_n(got.faces), CUBE)


def test_one_err_word_through_every_entry():
    """A vertex index equal to V on a 2-quad grid (4 faces, 6 vertices): every entry that shares the err word (csrc/gsr_mesh.h)
    raises the decoder's ValueError, and the same call with the valid faces then succeeds on the same stream.  Each kernel
    tests the index before it indexes anything with it, so nothing here faults the device."""
    from gaustar_amd import handover, regions
    v, f = rr.quad_grid(2, 1)
    bad = f.copy()
    bad[3, 2] = len(v)
    box = np.array([[-1.0] * 3, [3.0] * 3])
    tv, colours = _t(v), _t(np.full((len(v), 3), 0.5, np.float32))
    every = torch.ones(len(f), dtype=torch.bool, device=DEV)
    calls = dict(cut_mesh_by_box=lambda m: regions.cut_mesh_by_box(tv, m, box, False).faces,
                 select_faces=lambda m: regions.select_faces(tv, m, every).faces,
                 fill_small_holes=lambda m: regions.fill_small_holes(m, len(v)).faces,
                 face_areas=lambda m: regions.face_areas(tv, m),
                 vertex_to_face_colors=lambda m: handover.vertex_to_face_colors(m, colours))
    for name, call in calls.items():
        with pytest.raises(ValueError, match="outside"):
            call(_t(bad))
        assert call(_t(f)).shape[0] == len(f), name


# ---------------------------------------------------------------------------------------------------- areas
def test_face_areas_and_mean_are_reproducible():
    from gaustar_amd import regions
    bv, bf, fv, ff, _raw = chain_case()
    worst = 0
    for v, f in ((bv, bf), (fv, ff), (np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0]], np.float32), np.array([[0, 1, 2], [0, 0, 1]], np.int32))):
        got = _n(regions.face_areas(_t(v), _t(f)))
        want = ref.face_areas(v, f)
        assert got.dtype == np.float64 and got.shape == want.shape
        rel = np.abs(got - want) / np.maximum(want, np.finfo(np.float64).tiny)
        worst = max(worst, float(rel.max()) / 2.0 ** -53)
        assert (_ulps_f32(got.astype(np.float32), want.astype(np.float32)) <= 1).all()
    print("face_areas: largest deviation from numpy, in units of 2^-53 relative:", worst)
    area = regions.face_areas(_t(fv), _t(ff))
    for n in (1, 255, 256, 257, len(ff)):                          # one workgroup, its edge, several
        x = area[:n].contiguous()
        a, b = regions._mean_f64(x), regions._mean_f64(x)
        assert _n(a).tobytes() == _n(b).tobytes()
        want = ref.exact_mean(_n(x))
        dev = abs(float(a.cpu()) - want) / want
        print(f"mean of {n} areas: relative deviation {dev:.3e} (bound {n * 2.0 ** -53:.3e})")
        assert dev <= n * 2.0 ** -53
    got = regions.mean_edge_length(_t(bv), _t(bf))
    want = ref.mean_edge_length(bv, bf)
    print(f"mean_edge_length: relative deviation {abs(got - want) / want:.3e}")
    assert abs(got - want) <= (3 * len(bf) // 2) * 2.0 ** -53 * want             # 3 F / 2 unique edges of a closed mesh


# ---------------------------------------------------------------------------------------------------- the driver
def _regions_of(raw):
    from gaustar_amd import regions
    none = torch.empty(0, dtype=torch.int32, device=DEV)
    n = len(raw)
    return regions.UpdateRegions(component=none, region=none, n_components=n, n_regions=n, labels=np.arange(n, dtype=np.int32),
                                 counts=np.full(n, 100, np.int32), raw_boxes=np.asarray(raw, np.float64).copy())


class _Mesh:
    def __init__(self, verts, faces):
        self.verts, self.faces = _t(verts), _t(faces)


def _check_update(got, want, n_input_faces):
    assert got.faces.dtype == torch.int32 and got.track_face_mask.dtype == torch.bool and got.new_ref_area.dtype == torch.float32
    assert np.array_equal(_n(got.faces), want["faces"]) and _n(got.verts).tobytes() == want["verts"].tobytes()
    assert np.array_equal(_n(got.track_face_mask), want["track_face_mask"]) and got.track_face_num == want["track_face_num"]
    assert tuple(got.track_face_mask.shape) == (n_input_faces,)
    assert (got.cc_update_num, got.n_spliced, got.nothing_to_update) == (want["cc_update_num"], want["n_spliced"], False)
    assert np.float64(got.max_dist_in_connection).tobytes() == np.float64(want["max_dist_in_connection"]).tobytes()
    ulps = _ulps_f32(_n(got.new_ref_area), want["new_ref_area"])
    n_rest = len(want["faces"]) - want["track_face_num"]
    dev = abs(got.new_area_mean - want["new_area_mean"]) / want["new_area_mean"] if n_rest else 0.0
    print(f"new_ref_area: largest deviation {int(ulps.max())} f32 ulp; mean of {n_rest} areas: relative deviation {dev:.3e} "
          f"(bound {n_rest * 2.0 ** -53:.3e})")
    assert (ulps <= 1).all() and dev <= n_rest * 2.0 ** -53


@functools.lru_cache(maxsize=None)
def _chain_got(pad=0.02):
    from gaustar_amd import regions
    bv, bf, fv, ff, raw = chain_case()
    return regions.update_mesh_topology(_t(bv), _t(bf), _regions_of(raw), _Mesh(fv, ff), aabb_pad=pad)


def test_chain():
    bv, bf, _fv, _ff, raw = chain_case()
    want = chain_want()
    assert want["n_spliced"] == 2 and want["cc_update_num"] == 2          # (the restatement alone: not boxes that were all skipped)
    got = _chain_got()
    _check_update(got, want, len(bf))
    ok, n_exact = ref.prefix_is_original(_n(got.verts), _n(got.faces), _n(got.track_face_mask), bv, bf, rr.padded_boxes(raw, 0.02))
    assert ok and n_exact > 200
    # the second box was cut from the first box's result: a restatement that cuts from the uncut mesh disagrees
    mutant = chain_want(cut_from_uncut=True)
    assert mutant["n_spliced"] == 2 and not np.array_equal(mutant["faces"], _n(got.faces))
    from gaustar_amd import regions
    assert regions.is_watertight(got.faces)
    g = got.gaussian_mask(2)
    assert np.array_equal(_n(g), np.repeat(want["track_face_mask"], 2))


# update_mesh_topology's calls of Tensor.cpu for one spliced box of the chain case, counted by this test at the commit
# "Carry colours through the frame hand-over: colour mesh, update, re-bind" (32c4fe4), before the wrappers were shared: the
# two cuts 1 + 1, the three fillings 1 + 1 + 1, the outlier mask 2, select_faces 1, the two boundaries 1 + 1,
# connect_two_meshes 4, the surviving faces' number 1, the areas 1.
HOST_READS_ONE_BOX = 16


def test_update_host_reads(monkeypatch):
    """A host read is a discrete event: sharing code between the wrappers may not add one.  No margin."""
    from gaustar_amd import regions
    bv, bf, fv, ff, raw = chain_case()
    args = (_t(bv), _t(bf), _regions_of(raw[:1]), _Mesh(fv, ff))
    calls = []
    real = torch.Tensor.cpu
    monkeypatch.setattr(torch.Tensor, "cpu", lambda self, *a, **kw: calls.append(1) or real(self, *a, **kw))
    got = regions.update_mesh_topology(*args)
    monkeypatch.undo()
    print("Tensor.cpu calls in update_mesh_topology, one box:", len(calls))
    assert got.n_spliced == 1 and got.cc_update_num == 1
    assert len(calls) == HOST_READS_ONE_BOX


def test_nothing_to_update_and_failed_boxes():
    from gaustar_amd import regions
    bv, bf, fv, ff, _raw = chain_case()
    none = regions.update_mesh_topology(_t(bv), _t(bf), _regions_of(np.zeros((0, 2, 3))), _Mesh(fv, ff))
    assert none.nothing_to_update and none.cc_update_num == -1 and none.new_ref_area is None and bool(none.track_face_mask.all())
    far = np.array([[[5, 5, 5], [6, 6, 6]]], np.float64)
    out = regions.update_mesh_topology(_t(bv), _t(bf), _regions_of(far), _Mesh(fv, ff))
    assert out.cc_update_num == 0 and out.n_spliced == 0 and torch.equal(out.faces, _t(bf)) and np.isnan(out.new_area_mean)
    want = ref.face_areas(bv, bf).astype(np.float32)
    assert (_ulps_f32(_n(out.new_ref_area), want) <= 1).all()


def test_the_gap_this_closes():
    """A patch with one missing triangle: the stitch without hole filling is not watertight (the reference would skip the box),
    update_mesh_topology fills the hole first and splices the box."""
    from gaustar_amd import harness, regions
    bv, bf, fv, ff, raw = chain_case()
    ff = np.delete(ff, GAP_FACE, axis=0)
    sel = _regions_of(raw[:1])
    box = sel.boxes(0.02)[0]
    model = harness.SurfaceGaussians(_t(bv), _t(bf, torch.long), n_gaussians_per_surface_triangle=1, sh_levels=1)
    cut = regions.RegionCut(box=box, fusion_patch=regions.cut_mesh_by_box(_t(fv), _t(ff), box, False),
                            base_cut=regions.cut_mesh_by_box(_t(bv), _t(bf), box, True))
    assert ref.rim_census(_n(cut.fusion_patch.faces))[0] == 1              # the one triangle rim
    assert model.stitch_update_region(cut).stitched.watertight is False
    got = regions.update_mesh_topology(_t(bv), _t(bf), sel, _Mesh(fv, ff))
    want = ref.update_mesh_topology(bv, bf, 1, rr.padded_boxes(raw[:1], 0.02), fv, ff)
    assert want["n_spliced"] == 1
    _check_update(got, want, len(bf))
    assert got.n_spliced == 1 and regions.is_watertight(got.faces)


def test_pads_and_files(tmp_path):
    """aabb_pad=None: the five trials and the best pad again, through the harness; then save()."""
    from gaustar_amd import formats, harness, regions
    bv, bf, fv, ff, raw = chain_case()
    want_pad, want_scores = ref.choose_aabb_pad(lambda pad: chain_want(pad))
    sel = _regions_of(raw)
    seen = []

    def run(pad):
        seen.append(regions.update_mesh_topology(_t(bv), _t(bf), sel, _Mesh(fv, ff), aabb_pad=pad))
        return seen[-1]

    pad, scores = regions.choose_aabb_pad(run)
    assert pad == want_pad and scores == want_scores and len(seen) == 5
    model = harness.SurfaceGaussians(_t(bv), _t(bf, torch.long), n_gaussians_per_surface_triangle=1, sh_levels=1)
    model.topology_update_regions = lambda res, **kw: sel               # (the selection has its own tests)
    got = model.update_mesh_topology(None, _Mesh(fv, ff))
    _check_update(got, chain_want(want_pad), len(bf))
    far = _regions_of(np.array([[[5, 5, 5], [6, 6, 6]]], np.float64))
    model.topology_update_regions = lambda res, **kw: far
    assert model.update_mesh_topology(None, _Mesh(fv, ff)) is None        # cc_update_num == 0
    obj, npz = got.save(str(tmp_path))
    z = np.load(npz)
    assert sorted(z.files) == ["ref_area", "track_face_mask"]
    assert z["track_face_mask"].dtype == np.bool_ and z["track_face_mask"].shape == (len(bf),)
    assert z["ref_area"].dtype == np.float32 and z["ref_area"].shape == (int(got.faces.shape[0]),)
    v, f, _c = formats.load_obj(obj)
    assert np.array_equal(f, _n(got.faces)) and v.astype(np.float32).tobytes() == _n(got.verts).tobytes()
