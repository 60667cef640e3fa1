"""Numpy restatement of detect_topo_err's depth term (gaustar_trainers/refined_mesh.py:729-920 with gaustar_tools/warp_mesh.py),
steps as the reference performs them, for tests/test_topology.py and tests/test_gpu_topology.py.  cv2.blur, open3d's voxel
grid, pytorch3d's knn_points and trimesh's vertex-to-face colours are restated from their documented behaviour (none of
them is installed here): see gaustar_amd/csrc/gsr_topo.hip for the assumptions."""
import numpy as np

MAX_DEPTH = 10.0


def box3(a):
    """cv2.blur(a, (3, 3)) of an f32 map: BORDER_REFLECT_101, the 3x3 sum in double (row sums first) times 1/9, rounded to
    f32.  (For an f64 map, the same without the final rounding.)"""
    p = np.pad(np.asarray(a, np.float64), 1, mode="reflect")    # numpy "reflect" = reflect-101
    rows = p[:, :-2] + p[:, 1:-1] + p[:, 2:]
    s = rows[:-2] + rows[1:-1] + rows[2:]
    out = s * (1.0 / 9.0)
    return out.astype(np.float32) if np.asarray(a).dtype == np.float32 else out


def depth_edge(depth_gt, max_depth=MAX_DEPTH):
    """get_depth_edge(depth_gt, 3) (warp_mesh.py:120-130); None when no pixel is below max_depth (the reference raises)."""
    g = np.asarray(depth_gt, np.float32)
    below = g[g < max_depth]
    if below.size == 0:
        return None
    m = np.float32(float(below.max()) * 1.1)
    d = np.minimum(g, m)
    mean = box3(d)
    return np.maximum(box3(d * d) - mean * mean, np.float32(0))


def project(verts, intr, extr, shape):
    """warp_mesh.py:47-74: -> (pixels [V,2] = (row, col), local points [V,3]), in f64."""
    v = np.asarray(verts, np.float64)
    loc = (np.asarray(extr[:3, :3]) @ v.T + np.asarray(extr[:3, 3])[:, None]).T
    x, y = loc[:, 0] / loc[:, 2], loc[:, 1] / loc[:, 2]
    return np.stack([intr[1, 1] * y + shape[0] * 0.5, intr[0, 0] * x + shape[1] * 0.5], -1), loc


def query(image, pix):
    """query_at_image(image, pix, return_valid=True) (warp_mesh.py:106-117)."""
    with np.errstate(invalid="ignore"):
        p = (pix + 0.5).astype(np.int32)       # truncation toward zero; NaN -> INT_MIN on x86
    hi = np.int32(image.shape[:2]) - 1
    pc = np.clip(p, 0, hi)
    ok = (p == pc).all(-1)
    return image[pc[:, 0], pc[:, 1]], ok


def camera_row(verts, gt, render, surface, intr, extr, shape, max_depth=MAX_DEPTH):
    """One camera's row (refined_mesh.py:776-801): the depth loss where visible, -1 elsewhere; also the f64 pixels."""
    gt, render, surface = (np.asarray(a, np.float32) for a in (gt, render, surface))
    pix, loc = project(verts, intr, extr, shape)
    row = np.full(len(pix), -1.0, np.float32)
    var = depth_edge(gt, max_depth)
    if var is None:
        return row, pix
    vmax = var.max()
    if not vmax > 0:
        return row, pix
    depth_diff = np.abs(np.minimum(gt, np.float32(max_depth)) - render)
    sd, ok = query(surface, pix)
    vis = ok & (np.abs(loc[:, 2] - sd.astype(np.float64)) < 0.005)
    edge_vis = np.minimum(var / vmax * np.float32(1000), np.float32(1))
    ev, _ = query(edge_vis, pix)
    vis &= ev < np.float32(0.1)
    loss_map = np.minimum(depth_diff * (np.float32(1) - edge_vis) * np.float32(10), np.float32(2))
    lv, _ = query(loss_map, pix)
    row[vis] = lv[vis]
    return row, pix


def aggregate(table, verts, depth_scalar=3.0, min_observe=4, detect_floor=True):
    """refined_mesh.py:826-875 -> (value [V] f64, count [V])."""
    vis = table != -1
    cnt = vis.sum(0).astype(np.int64)
    value = np.zeros(table.shape[1])
    for v in np.nonzero(cnt >= min_observe)[0]:
        value[v] = np.average(table[vis[:, v], v].astype(np.float64))
    value = value * depth_scalar
    if detect_floor:
        y = np.asarray(verts, np.float64)[:, 1]
        floor = y < y.min() + 0.02
        value[floor] = 0
        cnt[floor] = min_observe + 1
    return value, cnt


def neighbours(faces, n_verts):
    """trimesh vertex_neighbors: the vertices sharing an edge with each vertex (ascending)."""
    nb = [set() for _ in range(n_verts)]
    for a, b, c in np.asarray(faces):
        for u, w in ((a, b), (b, c), (c, a)):
            nb[u].add(int(w)); nb[w].add(int(u))
    return [sorted(s) for s in nb]


def propagate_sequential(nbrs, valid, value, max_ite=20):
    """mesh_vert_propagate (warp_mesh.py:133-155), the reference's in-place loop."""
    value = np.array(value, np.float64)
    valid = np.array(valid, bool)
    for _ in range(max_ite):
        new_valid = valid.copy()
        cnt = 0
        for v in np.nonzero(~valid)[0]:
            n = np.array(nbrs[v], np.int64)
            m = valid[n] if n.size else np.zeros(0, bool)
            if m.any():
                value[v] = np.average(value[n[m]])
                new_valid[v] = True
                cnt += 1
        valid = new_valid
        if cnt == 0:
            break
    return value


def propagate_jacobi(nbrs, valid, value, sweeps=20):
    """The same as `sweeps` Jacobi sweeps without an early exit (what the GPU runs)."""
    value = np.array(value, np.float64)
    valid = np.array(valid, bool)
    for _ in range(sweeps):
        nv, nok = value.copy(), valid.copy()
        for v in np.nonzero(~valid)[0]:
            n = np.array([u for u in nbrs[v] if valid[u]], np.int64)
            if n.size:
                nv[v] = np.average(value[n])
                nok[v] = True
        value, valid = nv, nok
    return value


def voxel_grid(points, values, voxel_size):
    """open3d VoxelGrid.create_from_point_cloud + get_voxel_center_coordinate, voxels in ascending (ix, iy, iz) order ->
    (index [M,3], centre [M,3] f64, mean value [M])."""
    p = np.asarray(points, np.float64)
    origin = p.min(0) - voxel_size * 0.5
    idx = np.floor((p - origin) / voxel_size).astype(np.int64)
    keys, inv = np.unique(idx, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    sums = np.zeros(len(keys))
    cnt = np.zeros(len(keys))
    for i in range(len(p)):               # points in input order, as open3d accumulates them
        sums[inv[i]] += values[i]
        cnt[inv[i]] += 1
    centre = origin + (keys + 0.5) * voxel_size
    return keys, centre, sums / cnt


def knn(points, centres, K=8):
    """pytorch3d knn_points in f32: squared distances (dx^2 + dy^2) + dz^2, sorted, ties to the lower index; slots beyond
    the number of centres are (index 0, distance 0)."""
    q = np.asarray(points, np.float32)
    c = np.asarray(centres, np.float32)
    idx = np.zeros((len(q), K), np.int64)
    dist = np.zeros((len(q), K), np.float32)
    for s in range(0, len(q), 512):
        d = q[s:s + 512, None, :] - c[None, :, :]
        d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        k = min(K, len(c))
        order = np.argsort(d2, axis=1, kind="stable")[:, :k]
        idx[s:s + 512, :k] = order
        dist[s:s + 512, :k] = np.take_along_axis(d2, order, 1)
    return idx, dist


def interpolate(points, centres, vox_values, voxel_size, K=8):
    """interpolate_in_voxel (warp_mesh.py:199-213), weights in f64."""
    idx, dist = knn(points, centres, K)
    w = np.exp(-dist.astype(np.float64) / (voxel_size ** 2)) + 1e-8
    out = np.zeros(len(idx))
    for v in range(len(idx)):
        out[v] = np.average(vox_values[idx[v]], weights=w[v])
    return out


def face_colours(faces, values):
    """trimesh: vertex colour int(min(255 v, 255)), face colour = mean of its three cast to uint8 (truncation)."""
    vc = np.minimum(np.asarray(values) * 255, 255).astype(int)
    return vc[np.asarray(faces)].mean(axis=1).astype(np.uint8)


def rig_stages(table, verts, faces, depth_scalar=3.0, min_observe=4, mesh_prop=20, detect_floor=True, voxel_size=0.01):
    """Steps 8-13 from the [C, V] table -> dict of every stage."""
    value, cnt = aggregate(table, verts, depth_scalar, min_observe, detect_floor)
    prop = value.copy()
    if mesh_prop:
        prop = propagate_sequential(neighbours(faces, len(verts)), cnt >= min_observe, value, mesh_prop)
    keys, centre, vval = voxel_grid(verts, prop, voxel_size)
    interp = interpolate(np.asarray(verts, np.float64).astype(np.float32), centre.astype(np.float32), vval, voxel_size)
    fc = face_colours(faces, interp)
    return dict(value=value, count=cnt, propagated=prop, voxel_keys=keys, voxel_centre=centre, voxel_value=vval,
                interpolated=interp, face_colour=fc, face_loss=fc / 255)
