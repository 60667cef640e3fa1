"""tests/tracking_ref.py, the numpy restatement of gaustar_amd.tracking, pinned on cases whose answers are known without it.
No GPU.  tests/test_gpu_tracking.py holds the kernels to the restatement bit for bit."""
import numpy as np
import pytest

import tracking_ref as ref

TRI = np.array([[0.25, 0.5, 0.125], [1.75, 0.25, 0.5], [0.5, 2.0, -0.375]], np.float64)


# e0 = (2, 0, 0), e1 = (1, 2, 0): the determinant d00 d11 - d01 d01 = 16 is a power of two, so det (1.0 / det) is exactly 1
POW2 = np.array([[0.25, 0.5, 0.125], [2.25, 0.5, 0.125], [1.25, 2.5, 0.125]], np.float64)


def test_vertex_gives_unit_barycentrics():
    for k in range(3):
        want = np.zeros(3)
        want[k] = 1.0
        got = ref.point_to_bary(POW2, POW2[k])
        assert np.array_equal(got, want), (k, got)
        assert np.array_equal(ref.bary_to_point(POW2, want), POW2[k])
        # any triangle: the two other weights are exactly 0 at vertices 1 and 2, and the vertex's own is 1 within an ulp
        got = ref.point_to_bary(TRI, TRI[k])
        assert np.abs(got - want).max() <= 2.0 ** -52


def test_centre_and_round_trip():
    cen = ref.centres(TRI, np.array([[0, 1, 2]]))[0]
    assert np.array_equal(cen, ((TRI[0] + TRI[1]) + TRI[2]) / 3.0)
    assert np.abs(ref.point_to_bary(TRI, cen) - 1.0 / 3.0).max() <= 1e-15
    rng = np.random.default_rng(1)
    b = rng.dirichlet(np.ones(3), size=200)
    b = np.concatenate([b, 1.5 * b - 0.5 / 3.0])                    # in the plane, half of them outside the triangle
    p = ref.bary_to_point(TRI[None], b)
    back = ref.bary_to_point(TRI[None], ref.point_to_bary(TRI[None], p))
    assert np.abs(back - p).max() <= 1e-12
    # batched and single calls are the same function
    assert np.array_equal(ref.point_to_bary(TRI[None], p)[7], ref.point_to_bary(TRI, p[7]))


def test_dot_and_bary_to_point_orders():
    a, b = np.array([1e16, 1.0, -1e16]), np.array([1.0, 1.0, 1.0])
    assert ref.dot(a, b) == (1e16 + 1.0) - 1e16 and ref.dot(a, b) != 1.0
    t = np.array([[1e16, 0, 0], [1.0, 0, 0], [-1e16, 0, 0]], np.float64)
    assert ref.bary_to_point(t, np.ones(3))[0] == (1e16 + 1.0) - 1e16


def test_nearest_against_a_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    cen, q = rng.random((2000, 3)), rng.random((500, 3))
    d, i = cKDTree(cen).query(q, k=2)
    tied = d[:, 0] == d[:, 1]
    assert tied.sum() == 0                                           # (the seed was chosen for this)
    got = np.array([ref.nearest(p, cen) for p in q])
    assert np.array_equal(got[~tied], i[~tied, 0])


def test_nearest_takes_the_lowest_index_among_equals():
    cen = np.array([[1.0, 0, 0], [0.5, 0, 0], [3.0, 0, 0], [0.5, 0, 0], [-0.5, 0, 0]])
    assert ref.nearest(np.zeros(3), cen) == 1


@pytest.mark.parametrize("F,want", [(10, []), (11, []), (210, []), (211, [10]), (411, [10, 210]), (1000, [10, 210, 410, 610])])
def test_sample_rule(F, want):
    got = ref.sample_ids(F)
    assert got.tolist() == want and got.shape == (len(want),)


def test_rank_rule():
    mask = np.array([0, 0, 1, 1, 0, 1, 0, 1, 0, 0], bool)
    assert [ref.rank_of(mask, i) for i in range(len(mask))] == [0, 0, 0, 1, 2, 2, 3, 3, 4, 4]
    # the surviving faces are a prefix of the new mesh in their old order: rank is their new index
    assert [ref.rank_of(mask, i) for i in np.nonzero(mask)[0]] == [0, 1, 2, 3]
    excl = np.cumsum(mask) - mask
    assert excl.tolist() == [ref.rank_of(mask, i) for i in range(len(mask))]


def test_sqrt_collision_generator_finds_its_pair():
    found = ref.sqrt_collision()
    assert found is not None
    x_far, x_near, y, i, j = found
    assert i < j and x_far > x_near
    d_far, d_near = (x_far * x_far + y * y) + 0.0, (x_near * x_near + y * y) + 0.0
    assert d_far > d_near and np.sqrt(d_far) == np.sqrt(d_near)
    one = np.array([[0, 1, 2]])
    for x in (x_far, x_near):
        assert np.array_equal(ref.centres(ref.centre_face(x, y), one)[0], [x, y, 0.0])
    # the farther centre at the lower index wins, and the order decides
    cen = np.array([[x_far, y, 0.0], [x_near, y, 0.0]])
    assert ref.nearest(np.zeros(3), cen) == 0 and ref.nearest(np.zeros(3), cen[::-1]) == 0


def test_branches_case_fills_every_branch():
    c = ref.branches_case()
    assert len(c["faces"]) == 1152 and len(c["new_faces"]) == 4152
    pos = ref.positions(c["verts"], c["faces"], c["ids"], c["bary"])
    ids, bary, (kept, moved, lost) = ref.rebind(c["ids"], c["bary"], pos, c["mask"], c["new_verts"], c["new_faces"])
    assert min(kept, moved, lost) >= 100 and kept + moved + lost == 1152
    assert (bary >= 0).all() and np.abs(bary.sum(axis=1) - 1).max() < 1e-12
    back = ref.positions(c["new_verts"], c["new_faces"], ids, bary)
    assert np.linalg.norm(back - pos, axis=-1).max() < 0.05         # every point lands within about a cell (1 / 24) of itself


def test_degenerate_nearest_face_fails_the_reference_assert():
    verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 0], [5, 5, 0], [6, 5, 0]], np.float64)
    old_faces = np.array([[0, 1, 2]])
    new_faces = np.array([[3, 4, 5]])
    pos = ref.positions(verts, old_faces, np.array([0]), np.ones((1, 3)) / 3)
    with pytest.raises(AssertionError):
        ref.rebind(np.array([0]), np.ones((1, 3)) / 3, pos, np.array([False]), verts, new_faces)
