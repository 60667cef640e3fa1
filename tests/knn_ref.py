"""Numpy restatement of the K-nearest-neighbour search and of what its callers make of the rows (gaustar_amd/knn.py,
gaustar_amd/csrc/gsr_knn.hip), for tests/test_knn.py and tests/test_gpu_knn.py.  The rules are the ones tests/topo_ref.py::knn
states for pytorch3d's knn_points, with what that leaves open stated here: empty slots are (-1, inf), a point with a
non-finite coordinate is never a neighbour and has an empty row as a query, exclude_self skips candidate i for query i only."""
import numpy as np

import topo_ref as tr

FLT_MAX = np.float32(np.finfo(np.float32).max)


def knn(q, c, K, exclude_self=False):
    """-> (idx [N,K] int64, d2 [N,K] f32): per query the K smallest (d2, index) pairs over the eligible candidates, d2 =
    (dx dx + dy dy) + dz dz in f32 with d = query - candidate, by a stable argsort (the lower index first among equals)."""
    q = np.asarray(q, np.float32).reshape(-1, 3)
    c = np.asarray(c, np.float32).reshape(-1, 3)
    N, M = len(q), len(c)
    idx = np.full((N, K), -1, np.int64)
    dist = np.full((N, K), np.inf, np.float32)
    cok = np.isfinite(c).all(1)
    qok = np.isfinite(q).all(1)
    if M == 0:
        return idx, dist
    for s in range(0, N, 512):
        qs = q[s:s + 512]
        with np.errstate(invalid="ignore", over="ignore"):
            d = qs[:, None, :] - c[None, :, :]
            d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        ok = np.broadcast_to(cok[None, :], d2.shape).copy()
        if exclude_self:
            r = np.arange(len(qs))
            ok[r, s + r] = False
        ok &= qok[s:s + 512, None]
        key = np.where(ok, d2, np.float32(np.inf))
        order = np.argsort(key, axis=1, kind="stable")
        # the ineligible ones share the key inf with eligible pairs whose d2 overflowed: put them last, stably
        order = np.take_along_axis(order, np.argsort(~np.take_along_axis(ok, order, 1), axis=1, kind="stable"), 1)[:, :K]
        k = order.shape[1]
        good = np.take_along_axis(ok, order, 1)
        idx[s:s + 512, :k] = np.where(good, order, -1)
        dist[s:s + 512, :k] = np.where(good, np.take_along_axis(d2, order, 1), np.float32(np.inf))
    return idx, dist


def dist2_mean3(points):
    """simple-knn's distCUDA2 (simple_knn.cu:147-183): ((d0 + d1) + d2) / 3.0f over the three nearest OTHER points; a missing
    one counts as FLT_MAX, the reference's initial `best`."""
    _, d = knn(points, points, 3, exclude_self=True)
    d = np.where(np.isinf(d), FLT_MAX, d).astype(np.float32)
    with np.errstate(over="ignore"):
        return ((d[:, 0] + d[:, 1]) + d[:, 2]) / np.float32(3.0)


def exp_neg(x):
    """exp(x) for x <= 0 in f64 from IEEE operations in a fixed order (gsr_knn.hip's kn_exp_neg, operation for operation):
    x = n ln 2 + r, the Taylor polynomial of degree 13 in r by Horner's rule, times 2^n; 0 below -700."""
    x = np.asarray(x, np.float64)
    small = ~(x >= -700.0)
    xs = np.where(small, 0.0, x)
    n = np.rint(xs * 1.4426950408889634)
    r = (xs - n * 0.693147180369123816490) - n * 1.90821492927058770002e-10
    p = np.full_like(xs, 1.0 / 6227020800.0)
    for f in (479001600.0, 39916800.0, 3628800.0, 362880.0, 40320.0, 5040.0, 720.0, 120.0, 24.0, 6.0):
        p = p * r + 1.0 / f
    p = p * r + 0.5
    p = p * r + 1.0
    p = p * r + 1.0
    out = p * np.ldexp(1.0, n.astype(np.int64))
    return np.where(small, np.where(np.isnan(x), x, 0.0), out)


def weighted_mean(idx, d2, values, inv_scale):
    """interpolate_in_voxel's average (warp_mesh.py:204-211) with f64 weights exp(-d2 inv_scale) + 1e-8, the sums from 0 for k
    ascending; an empty slot (idx < 0) counts as (index 0, distance 0).  values [M,C] -> [N,C]."""
    idx = np.asarray(idx)
    values = np.asarray(values, np.float64).reshape(len(values), -1)
    have = idx >= 0
    d = np.where(have, np.asarray(d2, np.float32), np.float32(0)).astype(np.float64)
    j = np.where(have, idx, 0)
    w = exp_neg(-d * inv_scale) + 1e-8
    sw = np.zeros(len(idx))
    swv = np.zeros((len(idx), values.shape[1]))
    for k in range(idx.shape[1]):
        swv = swv + values[j[:, k]] * w[:, k, None]
        sw = sw + w[:, k]
    return swv / sw[:, None]


def voxel_post_processing(verts, move, count, min_observe=4, voxel_size=0.04, K=8):
    """warp_mesh.py:368-371 on the aggregated moves: voxels (tests/topo_ref.py::voxel_grid, ascending key order) over the
    vertices with count >= min_observe, rounded to f32 as the GPU takes them; per voxel the mean move of its vertices in
    index order; per vertex the weighted mean over its K nearest voxel centres -> (move_voxel [V,3], centres [M,3] f32,
    voxel moves [M,3])."""
    v32 = np.asarray(verts, np.float64).astype(np.float32)
    sel = np.asarray(count) >= min_observe
    move = np.asarray(move, np.float64)
    pts = v32[sel].astype(np.float64)
    cols = [tr.voxel_grid(pts, move[sel][:, a], voxel_size) for a in range(3)]
    centre = cols[0][1].astype(np.float32)
    vox = np.stack([c[2] for c in cols], 1)
    idx, d2 = knn(v32, centre, K)
    return weighted_mean(idx, d2, vox, 1.0 / (voxel_size * voxel_size)), centre, vox
