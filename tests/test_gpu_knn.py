"""GPU: the exact K-nearest-neighbour search (gaustar_amd.knn, gsr_knn.hip) against the numpy restatement (tests/knn_ref.py)
bit for bit -- indices equal, squared distances equal as bits -- in the culling and in the exhaustive mode, and the adapters
built on it: knn_points, distCUDA2, the model's neighbour tables and warp_mesh's voxel post-processing."""
import os

import numpy as np
import pytest
import torch

import knn_ref as kr
import warp_ref as wr
from test_gpu_warp import _faces_t, _frames, _mesh, _small_rig

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(x):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(DEV)


def _bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.int32)


def _check(q, c, K, exclude_self=False, what=""):
    """Both modes against the restatement and against each other; -> the culling mode's (idx, d2) as numpy."""
    from gaustar_amd import knn
    q = np.ascontiguousarray(q, np.float32)
    self_search = c is None
    cn = q if self_search else np.ascontiguousarray(c, np.float32)
    want_i, want_d = kr.knn(q, cn, K, exclude_self)
    qt = _t(q)
    ct = None if self_search else _t(cn)
    got = []
    with np.errstate(invalid="ignore"):
        for cull in (True, False):
            idx, d2 = knn.nearest_neighbors(qt, ct, K=K, exclude_self=exclude_self, cull=cull)
            assert idx.dtype == torch.int64 and d2.dtype == torch.float32 and tuple(idx.shape) == (len(q), K) == tuple(d2.shape)
            i, d = idx.cpu().numpy(), d2.cpu().numpy()
            bad = np.nonzero((i != want_i).any(1) | (_bits(d) != _bits(want_d)).any(1))[0]
            assert bad.size == 0, (what, f"cull={cull}", len(q), len(cn), K, bad[:5], i[bad[:2]], want_i[bad[:2]], d[bad[:2]], want_d[bad[:2]])
            got.append((i, d))
    assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(_bits(got[0][1]), _bits(got[1][1]))
    return got[0]


def _grid_points(rng, n, cells=16, span=4.0):
    """Points on a coarse grid: many exactly equal distances, a few exact duplicates."""
    return (rng.integers(0, cells, (n, 3)) * (span / cells)).astype(np.float32)


def _getters(hip_lib):
    return hip_lib.gsr_knn_tile(), hip_lib.gsr_knn_seed(), hip_lib.gsr_knn_queries()


@pytest.mark.parametrize("K", [1, 3, 4, 5, 8, 16, 17, 32])
def test_sizes_at_every_boundary(hip_lib, K):
    T, S, Q = _getters(hip_lib)
    rng = np.random.default_rng(K)
    for M in sorted({1, K - 1, K, K + 1, T - 1, T, T + 1, 2 * T + 3, 2 * S, 2 * S + 2}):
        c = _grid_points(rng, M)
        for N in (1, Q - 1, Q, Q + 1, 3 * Q + 5):
            _check(_grid_points(rng, N), c, K, what="sizes")
    # the queries as the candidates, with and without the point itself, at the same boundaries
    for M in (1, K, K + 1, T, T + 1, 2 * S + 2, 3 * Q + 5):
        p = _grid_points(rng, M)
        _check(p, None, K, what="self")
        _check(p, None, K, exclude_self=True, what="exclude_self")


def test_k_beyond_the_maximum_is_refused(hip_lib):
    from gaustar_amd import knn
    p = _t(np.zeros((40, 3)))
    with pytest.raises(ValueError, match="K = 33 is not implemented"):
        knn.nearest_neighbors(p, K=33)
    with pytest.raises(ValueError, match="K = 0"):
        knn.nearest_neighbors(p, K=0)
    with pytest.raises(ValueError, match="float32"):
        knn.nearest_neighbors(p.double(), K=1)
    with pytest.raises(ValueError, match="K = 33"):
        knn.knn_points(p[None], p[None], K=33)


def test_no_points(hip_lib):
    from gaustar_amd import knn
    p, none = _t(np.random.default_rng(0).random((70, 3))), _t(np.zeros((0, 3)))
    for cull in (True, False):
        idx, d2 = knn.nearest_neighbors(p, none, K=3, cull=cull)
        assert (idx == -1).all() and torch.isinf(d2).all() and tuple(idx.shape) == (70, 3)
        idx, d2 = knn.nearest_neighbors(none, p, K=3, cull=cull)
        assert tuple(idx.shape) == (0, 3) == tuple(d2.shape)
        idx, d2, st = knn.nearest_neighbors(none, none, K=3, cull=cull, return_stats=True)
        assert tuple(idx.shape) == (0, 3) and st == {"pairs": 0, "tiles_skipped": 0}


def test_lattice_ties(hip_lib):
    g = np.arange(6, dtype=np.float32)
    p = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1).reshape(-1, 3)
    for K in (8, 27):
        idx, d2 = _check(p, None, K, what="lattice")
        same = np.diff(d2, axis=1) == 0
        assert same.any() and (np.diff(idx, axis=1)[same] > 0).all()
        _check(p, None, K, exclude_self=True, what="lattice, no self")
    perm = np.random.default_rng(3).permutation(216)            # the caller's order is not the lattice's
    _check(p[perm], p, 8, what="lattice, shuffled queries")
    _check(p[perm], None, 8, what="lattice, shuffled")


def test_equidistant_candidates_across_a_tile_boundary(hip_lib):
    """2 K = 16 candidates at squared distance 14 exactly (sign flips and rotations of (1, 2, 3)) around a query at the centre, 3
    nearer ones and T + 21 farther ones: the row is the 3 nearer ones and the 5 lowest indices of the 16.  The sorted order
    puts the 16 into both tiles (asserted), so the tie is decided across a tile boundary, whichever tile comes first."""
    from gaustar_amd import knn
    T, _, _ = _getters(hip_lib)
    K = 8
    rng = np.random.default_rng(7)
    signs = np.array([[sx, sy, sz] for sx in (1, -1) for sy in (1, -1) for sz in (1, -1)], np.float32)
    tied = np.concatenate([signs * np.array([1, 2, 3], np.float32), signs * np.array([3, 1, 2], np.float32)])
    near = np.array([[1, 0, 0], [0, -1, 1], [1, 1, 1]], np.float32)
    far = rng.integers(3, 9, (T + 21, 3)).astype(np.float32) * rng.choice([-1.0, 1.0], (T + 21, 3)).astype(np.float32)
    centre = np.array([16, 16, 16], np.float32)
    c = np.concatenate([tied, near, far]) + centre
    assert len(c) == T + 40 and (((c - centre) ** 2).sum(1) == 14).sum() == 16
    perm = rng.permutation(len(c))
    c = c[perm]
    ct = _t(c)
    lo, scale = knn._box(ct)
    order = torch.sort(knn._morton(ct, lo, scale), stable=True)[1].cpu().numpy()
    where = np.nonzero((((c[order] - centre) ** 2).sum(1) == 14))[0]
    assert (where < T).any() and (where >= T).any(), where
    q = np.stack([centre, centre + np.float32(0.0)])
    idx, d2 = _check(q, c, K, what="equidistant")
    tied_ids = np.sort(np.nonzero(((c - centre) ** 2).sum(1) == 14)[0])
    assert d2[0].tolist() == [1, 2, 3] + [14] * 5 and idx[0, 3:].tolist() == tied_ids[:5].tolist()
    idx, d2 = _check(q, c, 2 * K, what="equidistant, K = 16")
    assert idx[0, 3:].tolist() == tied_ids[:13].tolist()


def test_degenerate_extents(hip_lib):
    rng = np.random.default_rng(11)
    same = np.tile(np.array([[0.3, -1.7, 2.5]], np.float32), (150, 1))       # zero extent on every axis
    idx, d2 = _check(same, None, 8, what="identical")
    assert np.array_equal(idx, np.tile(np.arange(8), (150, 1))) and not d2.any()
    idx, _ = _check(same, None, 8, exclude_self=True, what="identical, no self")
    assert idx[3].tolist() == [0, 1, 2, 4, 5, 6, 7, 8]
    _check(same[:5] + np.float32(1), same, 32, what="identical candidates")
    line = same.copy()                                                         # zero extent on two axes
    line[:, 0] = rng.integers(0, 40, 150).astype(np.float32) * np.float32(0.125)
    _check(line, None, 5, what="collinear")
    _check(_grid_points(rng, 70), line, 17, what="collinear candidates")
    plane = _grid_points(rng, 200)
    plane[:, 1] = 1.0
    _check(plane, None, 16, exclude_self=True, what="coplanar")


def test_points_that_are_not_finite(hip_lib):
    rng = np.random.default_rng(13)
    c = rng.random((300, 3)).astype(np.float32)
    q = rng.random((150, 3)).astype(np.float32)
    for a, j in ((c, [0, 17, 64, 65, 299]), (q, [1, 63, 64, 149])):
        for n, k in enumerate(j):
            a[k, n % 3] = (np.nan, np.inf, -np.inf)[n % 3]
    idx, d2 = _check(q, c, 8, what="non-finite")
    assert (idx[[1, 63, 64, 149]] == -1).all() and np.isinf(d2[[1, 63, 64, 149]]).all()
    assert not np.isin(idx, [0, 17, 64, 65, 299]).any() and (idx[0] >= 0).all()
    idx, _ = _check(c, None, 4, exclude_self=True, what="non-finite, self")
    assert (idx[[0, 17, 64, 65, 299]] == -1).all()
    # nothing eligible at all; fewer eligible candidates than K
    bad = np.full((70, 3), np.nan, np.float32)
    _check(q, bad, 3, what="all NaN")
    c2 = bad.copy()
    c2[[5, 69]] = [[0.1, 0.2, 0.3], [0.9, 0.8, 0.7]]
    idx, _ = _check(q, c2, 4, what="two eligible")
    assert idx[0].tolist() in ([5, 69, -1, -1], [69, 5, -1, -1])
    # a squared distance that overflows f32 is still a neighbour, after every finite one
    far = np.array([[0, 0, 0], [3e19, 0, 0], [1, 0, 0], [-3e19, 1, 0]], np.float32)
    idx, d2 = _check(far[:1], far, 4, what="overflow")
    assert idx[0].tolist() == [0, 2, 1, 3] and np.isinf(d2[0, 2:]).all()


def test_exclude_self_keeps_duplicates_at_other_indices(hip_lib):
    rng = np.random.default_rng(17)
    p = rng.random((130, 3)).astype(np.float32)
    p[100:130] = p[0:30]
    idx, d2 = _check(p, None, 3, exclude_self=True, what="duplicates")
    assert np.array_equal(idx[:30, 0], np.arange(100, 130)) and np.array_equal(idx[100:, 0], np.arange(30)) and not d2[:30, 0].any()
    assert (idx != np.arange(130)[:, None]).all()


def test_two_clusters_are_culled(hip_lib):
    """Two unit cubes 100 apart, 2 048 points each, K = 8 among themselves.  pairs <= N M / 2 (the tiles of the own cluster) +
    Q M (the one workgroup that can straddle the clusters) + N (T + 2 S + 1) (the one straddling tile, the seed window); the
    exhaustive mode evaluates N M."""
    from gaustar_amd import knn
    T, S, Q = _getters(hip_lib)
    rng = np.random.default_rng(19)
    p = rng.random((4096, 3)).astype(np.float32)
    p[rng.permutation(4096)[:2048], 0] += np.float32(100)
    N = M = 4096
    _check(p, None, 8, exclude_self=True, what="clusters")
    pt = _t(p)
    idx, d2, st = knn.nearest_neighbors(pt, K=8, exclude_self=True, return_stats=True)
    idx0, d20, st0 = knn.nearest_neighbors(pt, K=8, exclude_self=True, cull=False, return_stats=True)
    assert torch.equal(idx, idx0) and torch.equal(d2.view(torch.int32), d20.view(torch.int32))
    print(f"\ntwo clusters: pairs {st['pairs']} of {N * M}, tiles skipped {st['tiles_skipped']}")
    assert st0 == {"pairs": N * M, "tiles_skipped": 0}
    assert st["pairs"] <= N * M // 2 + Q * M + N * (T + 2 * S + 1)
    assert st["tiles_skipped"] >= (N // Q - 1) * (M // T // 2 - 1)


def test_a_far_outlier_query(hip_lib):
    rng = np.random.default_rng(23)
    c = rng.random((500, 3)).astype(np.float32)
    q = np.concatenate([rng.random((70, 3)).astype(np.float32), np.array([[1e3, 1e3, 1e3], [-5e4, 0.5, 0.5]], np.float32)])
    idx, d2 = _check(q, c, 8, what="outlier")
    assert (idx[-2:] >= 0).all() and (d2[-2:] > 1e5).all()
    _check(q, c[:5], 8, what="outlier, K > M")


def test_knn_points_adapter(hip_lib):
    from gaustar_amd import knn
    rng = np.random.default_rng(29)
    p1, p2 = rng.random((2, 90, 3)).astype(np.float32), rng.random((2, 140, 3)).astype(np.float32)
    res = knn.knn_points(_t(p1), _t(p2), K=5, return_nn=True)
    assert isinstance(res, tuple) and res._fields == ("dists", "idx", "knn")
    assert tuple(res.dists.shape) == (2, 90, 5) == tuple(res.idx.shape) and tuple(res.knn.shape) == (2, 90, 5, 3)
    for b in range(2):
        wi, wd = kr.knn(p1[b], p2[b], 5)
        assert np.array_equal(res.idx[b].cpu().numpy(), wi) and np.array_equal(_bits(res.dists[b].cpu().numpy()), _bits(wd))
        assert np.array_equal(res.knn[b].cpu().numpy(), p2[b][wi])
    assert knn.knn_points(_t(p1), _t(p2), K=5).knn is None
    # K > M: the slots beyond M are (0, 0) and a zero point
    res = knn.knn_points(_t(p1), _t(p2[:, :3]), K=5, return_nn=True)
    wi, wd = kr.knn(p1[1], p2[1, :3], 5)
    assert np.array_equal(res.idx[1, :, :3].cpu().numpy(), wi[:, :3]) and np.array_equal(res.dists[1, :, :3].cpu().numpy(), wd[:, :3])
    assert not res.idx[:, :, 3:].any() and not res.dists[:, :, 3:].any() and not res.knn[:, :, 3:].any()
    # D = 2 by zero padding
    a, b = p1[:1, :, :2], p2[:1, :, :2]
    res = knn.knn_points(_t(a), _t(b), K=4, return_nn=True)
    wi, wd = kr.knn(np.pad(a[0], ((0, 0), (0, 1))), np.pad(b[0], ((0, 0), (0, 1))), 4)
    assert np.array_equal(res.idx[0].cpu().numpy(), wi) and np.array_equal(_bits(res.dists[0].cpu().numpy()), _bits(wd))
    assert tuple(res.knn.shape) == (1, 90, 4, 2) and np.array_equal(res.knn[0].cpu().numpy(), b[0][wi])


def test_knn_points_gradients(hip_lib):
    from gaustar_amd import knn
    rng = np.random.default_rng(31)
    p1 = _t(rng.random((1, 50, 3))).requires_grad_(True)
    p2 = _t(rng.random((1, 80, 3))).requires_grad_(True)
    res = knn.knn_points(p1, p2, K=4, return_nn=True)
    plain = knn.knn_points(p1.detach(), p2.detach(), K=4)
    assert torch.equal(res.idx, plain.idx) and torch.equal(res.dists.detach().view(torch.int32), plain.dists.view(torch.int32))
    (res.dists.sum() + (res.knn * 0.5).sum()).backward()
    g1, g2 = p1.grad.clone(), p2.grad.clone()
    a, b = p1.detach().clone().requires_grad_(True), p2.detach().clone().requires_grad_(True)
    near = b[0][plain.idx[0]]
    (((a[0][:, None, :] - near) ** 2).sum() + (near * 0.5).sum()).backward()
    assert torch.allclose(g1, a.grad, rtol=1e-5, atol=1e-6) and torch.allclose(g2, b.grad, rtol=1e-5, atol=1e-6)
    assert g1.abs().sum() > 0 and g2.abs().sum() > 0


def test_dist_cuda2_and_its_shim(hip_lib):
    from gaustar_amd import knn
    from simple_knn._C import distCUDA2
    assert distCUDA2 is knn.dist_cuda2
    rng = np.random.default_rng(37)
    p = rng.random((5000, 3)).astype(np.float32)
    p[4000:4100] = p[:100]                                                    # duplicates count at distance 0
    got = distCUDA2(_t(p)).cpu().numpy()
    assert got.dtype == np.float32 and np.array_equal(_bits(got), _bits(kr.dist2_mean3(p)))
    for P in (1, 3, 4):
        got = distCUDA2(_t(p[:P])).cpu().numpy()
        assert np.array_equal(_bits(got), _bits(kr.dist2_mean3(p[:P]))), P
    assert torch.isinf(distCUDA2(_t(p[:1]))).all() and float(distCUDA2(_t(p[:3]))[0]) == float(kr.FLT_MAX / np.float32(3))
    assert tuple(distCUDA2(_t(p[:0])).shape) == (0,)


def test_model_neighbour_tables(hip_lib):
    from gaustar_amd import harness, scene
    v, f = scene.icosphere(2, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    model = harness.SurfaceGaussians(torch.from_numpy(v).float().to(DEV), torch.from_numpy(f).long().to(DEV), sh_levels=1)
    model.reset_neighbors(16)
    n = model.n_points
    assert tuple(model.knn_idx.shape) == (n, 16) == tuple(model.knn_dists.shape) and model.knn_to_track == 16
    pts = model.points.detach().float().cpu().numpy()
    wi, wd = kr.knn(pts, pts, 16)
    assert np.array_equal(model.knn_idx.cpu().numpy(), wi) and np.array_equal(_bits(model.knn_dists.cpu().numpy()), _bits(wd))
    assert not model.knn_dists[:, 0].any()
    first = model.knn_idx[:, 0].cpu().numpy()
    assert np.array_equal(pts[first], pts) and (first <= np.arange(n)).all()
    model.reset_neighbors()
    assert tuple(model.knn_idx.shape) == (n, 16)
    assert model.get_neighbors_of_random_points(-1) is model.knn_idx
    rows = model.get_neighbors_of_random_points(10)
    assert tuple(rows.shape) == (10, 16) and (rows[:, None, :] == model.knn_idx[None]).all(-1).any(1).all()


def test_two_streams_give_the_same_bits(hip_lib):
    from gaustar_amd import knn
    rng = np.random.default_rng(41)
    p = _t(_grid_points(rng, 3000, cells=12))
    torch.cuda.synchronize()
    out = []
    for _ in range(2):
        s = torch.cuda.Stream(device=DEV)
        with torch.cuda.stream(s):
            out.append(knn.nearest_neighbors(p, K=16, exclude_self=True))
        s.synchronize()
    assert torch.equal(out[0][0], out[1][0]) and torch.equal(out[0][1].view(torch.int32), out[1][1].view(torch.int32))


@pytest.fixture(scope="module")
def warp_case(hip_lib):
    """40 small cameras, edge_scalar 100, min_observe 2 (with the reference's edge scale nothing is observed at this size)."""
    rig = _small_rig()
    v, f = _mesh(4)
    fr = _frames(rig)
    torch.cuda.synchronize()
    return rig, v, f, fr


def test_warp_voxel_mode_matches_the_restatement(warp_case):
    from gaustar_amd import warp
    rig, v, f, fr = warp_case
    cfg = warp.WarpConfig(edge_scalar=100, min_observe=2, post_processing="voxel")
    res = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], cfg)
    assert res.move_propagated is None and res.verts_propagated is None
    count = res.count.cpu().numpy()
    assert 0.3 < (count >= 2).mean() < 1.0
    want, centre, _ = kr.voxel_post_processing(v, res.move_raw.cpu().numpy(), count, 2, cfg.voxel_size, cfg.knn_K)
    assert len(centre) > 100
    got = res.move_voxel.cpu().numpy()
    assert got.dtype == np.float64 and np.array_equal(got, want), np.abs(got - want).max()
    sm = wr.smooth(wr.neighbours(f, len(v)), want, 5)
    assert np.array_equal(res.move_smoothed.cpu().numpy(), sm)
    assert torch.equal(res.verts_voxel, torch.from_numpy(v).to(DEV) + res.move_voxel)
    assert torch.equal(res.verts_smoothed, torch.from_numpy(v).to(DEV) + res.move_smoothed)
    # another K and voxel size
    cfg = warp.WarpConfig(edge_scalar=100, min_observe=2, post_processing="voxel", voxel_size=0.11, knn_K=3)
    res = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], cfg)
    want, _, _ = kr.voxel_post_processing(v, res.move_raw.cpu().numpy(), res.count.cpu().numpy(), 2, 0.11, 3)
    assert np.array_equal(res.move_voxel.cpu().numpy(), want)
    with pytest.raises(ValueError, match="no vertex"):
        warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], warp.WarpConfig(edge_scalar=100, min_observe=1000, post_processing="voxel"))
    with pytest.raises(ValueError, match="not implemented"):
        warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], warp.WarpConfig(post_processing="octree"))


def test_warp_mesh_mode_is_untouched(warp_case):
    from gaustar_amd import warp
    rig, v, f, fr = warp_case
    res = warp.warp_mesh(v, _faces_t(f), rig, lambda i: fr[i], warp.WarpConfig(edge_scalar=100, min_observe=2), return_stages=True)
    assert res.move_voxel is None and res.verts_voxel is None
    want = wr.rig_stages(res.table.cpu().numpy(), v, f, min_observe=2)
    for k in ("move_raw", "move_propagated", "move_smoothed"):
        np.testing.assert_allclose(getattr(res, k).cpu().numpy(), want[k], rtol=1e-12, atol=0, equal_nan=True)
    assert torch.equal(res.count.cpu(), torch.from_numpy(want["count"]).int())


def test_warp_adapter_writes_warp_voxel_obj(tmp_path, hip_lib):
    from gaustar_amd import formats, warp
    rig = _small_rig(2)
    v, f = _mesh(3)
    fr = _frames(rig, device="cpu")
    data = tmp_path / "data"
    for d in ("0005/flow_bi", "0005/depth", "0006/depth"):
        (data / d).mkdir(parents=True)
    np.savez(data / "rgb_cameras.npz", **rig)
    for i in range(len(rig["shape"])):
        ff, fb, dc, dn = (x.numpy() for x in fr[i])
        np.savez(data / f"0005/flow_bi/{i:04d}_f.npz", flow=ff)
        np.savez(data / f"0005/flow_bi/{i:04d}_b.npz", flow=fb)
        np.savez(data / f"0005/depth/img_{i:04d}_depth.npz", depth=dc)
        np.savez(data / f"0006/depth/img_{i:04d}_depth.npz", depth=dn)
    col = np.random.default_rng(0).random((len(v), 3))
    formats.save_obj(str(tmp_path / "mesh.obj"), v, f, col)
    work = str(tmp_path / "work") + "/"
    cfg = warp.WarpConfig(edge_scalar=100, min_observe=1, post_processing="voxel")
    res = warp.warp_mesh_using_flow(str(tmp_path / "mesh.obj"), str(data) + "/", work, 5, cfg=cfg)
    out = work + "0006/coarse_mesh/"
    assert os.path.exists(out + "warp_voxel.obj") and not os.path.exists(out + "warp_mesh_prop.obj")
    assert '"post_processing": "voxel"' in open(out + "config.json").read()
    for name, key in (("warp_voxel.obj", "verts_voxel"), ("warp_smooth.obj", "verts_smoothed"), ("warp_0005.obj", "verts_raw")):
        v2, f2, c2 = formats.load_obj(out + name)
        assert np.array_equal(v2, getattr(res, key).cpu().numpy()) and np.array_equal(f2, f), name
    assert int((res.count >= 1).sum()) > 0
