"""The restatement of the K-nearest-neighbour search (tests/knn_ref.py) pinned on answers known without it: a kd-tree, a
lattice whose ties are counted by hand, simple-knn's mean of three, hand cases of the weighted mean and of the voxel
post-processing.  No GPU: tests/test_gpu_knn.py holds the kernels against this restatement bit for bit."""
import ctypes

import numpy as np
import pytest

import knn_ref as kr
import topo_ref as tr


def _lattice(n=6):
    g = np.arange(n, dtype=np.float32)
    return np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)


def test_rows_against_a_kd_tree():
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    q, c = rng.random((3000, 3), np.float32), rng.random((4000, 3), np.float32)
    d, i = cKDTree(c.astype(np.float64)).query(q.astype(np.float64), k=17)
    # a row whose neighbours the f32 rounding of d2 could reorder would have to be left out: the seed has none
    gap = (d[:, 1:] ** 2 - d[:, :-1] ** 2) / np.maximum(d[:, 1:] ** 2, 1e-300)
    risky = (gap < 4e-7).any(1)
    assert risky.sum() == 0                                          # (the seed was chosen for this)
    idx, d2 = kr.knn(q, c, 16)
    assert np.array_equal(idx, i[:, :16])
    np.testing.assert_allclose(d2, d[:, :16] ** 2, rtol=4e-7, atol=0)
    assert idx.dtype == np.int64 and d2.dtype == np.float32


def test_lattice_ties_go_to_the_lower_index():
    p = _lattice()
    idx9, d9 = kr.knn(p, p, 9)
    tied = d9[:, 7] == d9[:, 8]
    assert tied.sum() == 208                                         # all but the 8 corners
    idx, d2 = kr.knn(p, p, 8)
    assert np.array_equal(idx, idx9[:, :8]) and np.array_equal(d2, d9[:, :8])
    assert np.array_equal(idx[:, 0], np.arange(216)) and not d2[:, 0].any()
    assert (np.diff(d2, axis=1) >= 0).all()
    same = np.diff(d2, axis=1) == 0
    assert (np.diff(idx, axis=1)[same] > 0).all() and same[tied].any(1).all()
    # the exact lattice distances: every row is the 8 smallest (d2, index) pairs of the full table
    full = ((p[:, None, :] - p[None, :, :]) ** 2).sum(-1)
    for r in (0, 43, 100, 215):
        want = sorted((float(full[r, j]), j) for j in range(216))[:8]
        assert [(float(a), int(b)) for a, b in zip(d2[r], idx[r])] == want


def test_empty_slots_ineligible_points_and_self():
    c = np.array([[0, 0, 0], [1, 0, 0], [np.nan, 0, 0], [0, 2, 0], [np.inf, 0, 0], [1, 0, 0]], np.float32)
    idx, d2 = kr.knn(c, c, 5)
    assert idx[0].tolist() == [0, 1, 5, 3, -1] and d2[0].tolist() == [0.0, 1.0, 1.0, 4.0, np.inf]
    assert (idx[2] == -1).all() and np.isinf(d2[2]).all() and (idx[4] == -1).all()
    idx, d2 = kr.knn(c, c, 2, exclude_self=True)
    assert idx[1].tolist() == [5, 0] and d2[1].tolist() == [0.0, 1.0]        # the duplicate at another index counts
    assert idx[5].tolist() == [1, 0]
    idx, d2 = kr.knn(c, np.zeros((0, 3), np.float32), 3)
    assert (idx == -1).all() and np.isinf(d2).all() and idx.shape == (6, 3)
    # a squared distance that overflows belongs to an eligible point: it keeps its index
    far = np.array([[0, 0, 0], [3e19, 0, 0]], np.float32)
    idx, d2 = kr.knn(far[:1], far, 3)
    assert idx[0].tolist() == [0, 1, -1] and d2[0].tolist() == [0.0, np.inf, np.inf]


def test_dist2_mean3():
    """distCUDA2's value.  With P points a row has P - 1 neighbours and a missing one counts as FLT_MAX (simple_knn.cu:157):
    P <= 2 gives (x + FLT_MAX) + FLT_MAX = inf; P = 3 gives (d0 + d1) + FLT_MAX = FLT_MAX after rounding, a third of it after
    the division -- not inf, which the sum reaches only with two slots missing."""
    from scipy.spatial import cKDTree
    rng = np.random.default_rng(0)
    p = rng.random((5000, 3), np.float32)
    d, _ = cKDTree(p.astype(np.float64)).query(p.astype(np.float64), k=4)
    want = (d[:, 1:] ** 2).mean(1)
    got = kr.dist2_mean3(p)
    rel = np.abs(got - want) / want
    print(f"\ndist2_mean3 vs the f64 kd-tree: max rel {rel.max():.2e}")
    assert got.dtype == np.float32 and rel.max() <= 1e-6
    assert np.isinf(kr.dist2_mean3(p[:1])).all() and np.isinf(kr.dist2_mean3(p[:2])).all()
    three = kr.dist2_mean3(p[:3])
    assert np.array_equal(three, np.full(3, kr.FLT_MAX / np.float32(3), np.float32)) and (three > 1e38).all()
    assert np.isfinite(kr.dist2_mean3(p[:4])).all()
    q = np.array([[0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 2, 0], [5, 5, 5]], np.float32)
    got = kr.dist2_mean3(q)
    assert got[0] == np.float32((0.0 + 1.0 + 4.0) / 3) and got[1] == got[0]       # the duplicate at 0, not the point itself
    assert got[2] == np.float32((1.0 + 1.0 + 5.0) / 3)


def test_exp_neg_is_within_two_ulp():
    x = -np.concatenate([np.linspace(0, 60, 20001), np.geomspace(1e-12, 700, 5001), [0.0, 700.0]])
    got, want = kr.exp_neg(x), np.exp(x)
    assert (np.abs(got - want) <= 2 * np.spacing(want)).all()
    assert kr.exp_neg(0.0) == 1.0 and kr.exp_neg(-701.0) == 0.0 and kr.exp_neg(-np.inf) == 0.0 and np.isnan(kr.exp_neg(np.nan))


def test_weighted_mean_hand_cases():
    vals = np.array([[2.0, -0.5, 0.25], [10.0, 20.0, 30.0]])
    # one voxel in every slot: its value, exactly (powers of two, so that v w / w rounds nowhere)
    out = kr.weighted_mean(np.zeros((2, 1), np.int64), np.array([[0.3], [7.0]], np.float32), vals[:1], 1 / 0.04 ** 2)
    assert np.array_equal(out, np.tile(vals[:1], (2, 1)))
    # an empty slot is voxel 0 at distance 0: weights (exp(-1) + 1e-8, 1 + 1e-8)
    out = kr.weighted_mean(np.array([[1, -1]]), np.array([[1.0, np.inf]], np.float32), vals, 1.0)
    w = np.array([np.exp(-1.0) + 1e-8, 1.0 + 1e-8])
    np.testing.assert_allclose(out[0], (vals[1] * w[0] + vals[0] * w[1]) / w.sum(), rtol=1e-15)
    # against topo_ref's interpolate (numpy's exp) on random rows
    rng = np.random.default_rng(1)
    pts, cen, v = rng.random((50, 3), np.float32), rng.random((20, 3), np.float32), rng.random(20)
    idx, d2 = kr.knn(pts, cen, 8)
    np.testing.assert_allclose(kr.weighted_mean(idx, d2, v[:, None], 1 / 0.3 ** 2)[:, 0], tr.interpolate(pts, cen, v, 0.3), rtol=1e-14)


def test_voxel_post_processing_on_four_vertices():
    """Vertices 0 and 1 share a voxel, 2 has its own, 3 is not observed.  The grid of size 1 has its origin half a voxel below
    the lowest observed vertex, at -0.25: voxels (0, 0, 0) and (2, 0, 0), centres (0.25, 0.25, 0.25) and (2.25, 0.25, 0.25)."""
    verts = np.array([[0.25, 0.25, 0.25], [0.5, 0.5, 0.5], [2.5, 0.25, 0.25], [1.5, 0.75, 0.75]])
    move = np.array([[1.0, 0, 0], [3.0, 0, 2.0], [0, 4.0, 0], [9, 9, 9]])
    count = np.array([4, 5, 4, 3])
    out, centre, vox = kr.voxel_post_processing(verts, move, count, 4, 1.0, K=8)
    assert np.array_equal(centre, np.array([[0.25, 0.25, 0.25], [2.25, 0.25, 0.25]], np.float32))
    assert np.array_equal(vox, np.array([[2.0, 0, 1.0], [0, 4.0, 0]]))
    # K = 8 > 2 voxels: six empty slots, each voxel 0 at distance 0
    for i, v in enumerate(verts):
        d = ((v[None] - centre.astype(np.float64)) ** 2).sum(1)
        w = np.concatenate([np.exp(-d) + 1e-8, np.full(6, 1.0 + 1e-8)])
        vals = np.concatenate([vox, np.tile(vox[:1], (6, 1))])
        np.testing.assert_allclose(out[i], (vals * w[:, None]).sum(0) / w.sum(), rtol=1e-14)
    # K = 1: the nearest voxel's move, exactly (powers of two: v w / w rounds nowhere); vertex 3 is nearer to the second
    # centre, 0.5625 + 0.5 against 1.5625 + 0.5
    out1, _, _ = kr.voxel_post_processing(verts, move, count, 4, 1.0, K=1)
    assert np.array_equal(out1, vox[[0, 0, 1, 1]])


def test_python_surface_refuses_what_is_not_implemented():
    """No GPU: the adapters check their arguments before they touch the device."""
    import torch
    from gaustar_amd import knn
    p = torch.zeros(1, 4, 3)
    with pytest.raises(ValueError, match="lengths"):
        knn.knn_points(p, p, lengths1=torch.tensor([4]))
    with pytest.raises(ValueError, match="norm"):
        knn.knn_points(p, p, norm=1)
    with pytest.raises(ValueError, match="D=4"):
        knn.knn_points(torch.zeros(1, 4, 4), torch.zeros(1, 4, 4))
    with pytest.raises(ValueError, match="GPU"):
        knn.nearest_neighbors(p[0], K=1)
    from simple_knn._C import distCUDA2
    assert distCUDA2 is knn.dist_cuda2
    import gaustar_amd
    assert gaustar_amd.knn_points is knn.knn_points and gaustar_amd.nearest_neighbors is knn.nearest_neighbors


def test_entry_points_validate_without_gpu(hip_lib):
    from gaustar_amd import build
    assert "gsr_knn.hip" in build.SOURCES
    T, S, Q = hip_lib.gsr_knn_tile(), hip_lib.gsr_knn_seed(), hip_lib.gsr_knn_queries()
    assert T >= 1 and Q == 64 and hip_lib.gsr_knn_max_k() == 32 and 2 * S + 1 >= 32 + 1      # the seed can fill a list, self excluded
    tiles = lambda m: (m + T - 1) // T
    assert hip_lib.gsr_knn_workspace_bytes(10, 0, 4) == 0
    for m in (1, T, T + 1, 491520):
        assert hip_lib.gsr_knn_workspace_bytes(7, m, 16) == tiles(m) * (16 * T + 32)
    null = None
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    err = lambda: hip_lib.gsr_last_error()
    assert hip_lib.gsr_knn_search(4, 4, 33, p, p, p, p, 0, 1, p, p, null, null) != 0 and b"between 1 and 32" in err()
    assert hip_lib.gsr_knn_search(4, 4, 0, p, p, p, p, 0, 1, p, p, null, null) != 0 and b"between 1 and 32" in err()
    assert hip_lib.gsr_knn_search(-1, 4, 3, p, p, p, p, 0, 1, p, p, null, null) != 0 and b"negative" in err()
    assert hip_lib.gsr_knn_search(4, 5, 3, p, p, p, p, 1, 1, p, p, null, null) != 0 and b"exclude_self" in err()
    assert hip_lib.gsr_knn_search(4, 4, 3, null, p, p, p, 0, 1, p, p, null, null) != 0 and b"null" in err()
    assert hip_lib.gsr_knn_search(4, 4, 3, p, p, null, p, 0, 1, p, p, null, null) != 0 and b"null" in err()
    assert hip_lib.gsr_knn_search(0, 4, 3, null, null, null, null, 0, 1, null, null, null, null) == 0
    assert hip_lib.gsr_knn_prepare(0, null, null, null, null) == 0
    assert hip_lib.gsr_knn_prepare(3, p, null, p, null) != 0 and b"null" in err()
    assert hip_lib.gsr_knn_prepare(-3, p, p, p, null) != 0 and b"negative" in err()
    assert hip_lib.gsr_knn_mean_d2(5, 2, p, p, null) != 0 and b"at least 3" in err()
    assert hip_lib.gsr_knn_mean_d2(5, 3, null, p, null) != 0 and b"null" in err()
    assert hip_lib.gsr_knn_mean_d2(0, 3, null, null, null) == 0
    assert hip_lib.gsr_knn_segment_mean(4, 2, 3, null, p, p, p, p, null) != 0 and b"null" in err()
    assert hip_lib.gsr_knn_segment_mean(0, 0, 3, null, null, null, null, null, null) == 0
    assert hip_lib.gsr_knn_weighted_mean(4, 8, 3, 0, p, p, p, 1.0, p, null) != 0 and b"at least one" in err()
    assert hip_lib.gsr_knn_weighted_mean(4, 8, 3, 2, p, null, p, 1.0, p, null) != 0 and b"null" in err()
    assert hip_lib.gsr_knn_weighted_mean(0, 8, 3, 2, null, null, null, 1.0, null, null) == 0
