"""Numpy restatement of extract_mesh_fusion (gaustar_trainers/refined_mesh.py:311-459) for tests/test_fusion.py and
tests/test_gpu_fusion.py: the image preparation (:412-445), the integration of Open3D's legacy ScalableTSDFVolume(voxel_length,
sdf_trunc, RGB8) and marching cubes over the voxel centres.

Open3D is not installed here.  The integration and the extraction are written from the rules the feature was specified by
(include/gsr.h states them too), with their dtypes -- f64 geometry, f32 accumulation -- and their operation order, which
gsr_fusion.hip follows operation by operation.  PARITY WITH OPEN3D ITSELF IS NOT PINNED: nothing here has been compared with
an Open3D run.  Where this is known to differ from Open3D: the unit directory is dense and bounded (Open3D's hash of units
grows with the data), the colour mean is f32 (Open3D: double) and the marching-cubes table is gaustar_amd.fusion.mc_table()
(Open3D ships its own), which the kernel and this file both read.  cv2.blur is restated as in tests/topo_ref.py."""
import numpy as np

import topo_ref as tr

UNIT = 16
STRIDE = 4
f32 = np.float32


# ------------------------------------------------------------------------------------------------ image preparation
def prep(rgb, depth_alpha, depth_trunc=6.0, mask_background=True, remove_depth_edge=True):
    """refined_mesh.py:360 and :412-445: rgb, depth_alpha [H,W,3] f32 (the two renders) -> (depth [H,W] f32, rgb8 [H,W,3] uint8)."""
    rgb = np.clip(np.asarray(rgb, f32), f32(0), f32(1))
    da = np.asarray(depth_alpha, f32)
    depth, alpha = da[..., 0].copy(), da[..., 2]
    depth = depth / (alpha + f32(1e-8))
    if mask_background:
        depth[alpha < f32(0.5)] = 0
    if remove_depth_edge:
        var = tr.depth_edge(depth, 10.0)        # get_depth_edge(depth, 3), max_depth=None: m = 1.1 max(depth[depth < 10])
        if var is not None and var.max() > 0:   # (the reference raises on the empty max; a flat map gives NaN > 0.5 = False)
            edge_vis = np.minimum(var / var.max() * f32(1000), f32(1))
            depth[edge_vis > f32(0.5)] = 0
    depth[depth >= f32(depth_trunc)] = 0        # open3d create_from_color_and_depth(depth_trunc=...)
    return depth, (rgb * f32(255)).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the volume
def new_volume(lo, hi, voxel, trunc):
    """Dense directory over [lo, hi] padded by trunc and one unit: dict with u0, nu (xyz), tsdf, weight [nz,ny,nx], color [3,...]."""
    L = UNIT * float(voxel)
    u0 = np.floor((np.asarray(lo, np.float64) - trunc) / L).astype(np.int64) - 1
    u1 = np.floor((np.asarray(hi, np.float64) + trunc) / L).astype(np.int64) + 1
    nu = u1 - u0 + 1
    nz, ny, nx = (int(UNIT * n) for n in nu[::-1])
    return {"voxel": float(voxel), "trunc": float(trunc), "u0": u0, "nu": nu, "tsdf": np.zeros((nz, ny, nx), f32),
            "weight": np.zeros((nz, ny, nx), f32), "color": np.zeros((3, nz, ny, nx), f32)}


def touch(vol, depth, intr, extr):
    """The touch pass: bool [nuz, nuy, nux]."""
    fx, fy, cx, cy = intr
    Ei = np.linalg.inv(np.asarray(extr, np.float64).reshape(4, 4))
    H, W = depth.shape
    i, j = np.meshgrid(np.arange(0, H, STRIDE), np.arange(0, W, STRIDE), indexing="ij")
    d32 = depth[i, j]
    keep = d32 > 0
    i, j, d = i[keep].astype(np.float64), j[keep].astype(np.float64), d32[keep].astype(np.float64)
    x, y = (j - cx) * d / fx, (i - cy) * d / fy
    L = float(UNIT) * vol["voxel"]
    nu, u0 = vol["nu"], vol["u0"]
    touched = np.zeros(tuple(int(n) for n in nu[::-1]), bool)
    lo, hi = [], []
    ok = np.ones(len(d), bool)
    for a in range(3):
        p = Ei[a, 0] * x + Ei[a, 1] * y + Ei[a, 2] * d + Ei[a, 3]
        l, h = np.floor((p - vol["trunc"]) / L), np.floor((p + vol["trunc"]) / L)
        ok &= np.isfinite(l) & np.isfinite(h)
        lo.append(np.maximum(np.nan_to_num(l) - u0[a], 0).astype(np.int64))
        hi.append(np.minimum(np.nan_to_num(h) - u0[a], nu[a] - 1).astype(np.int64))
    for k in np.nonzero(ok)[0]:
        touched[lo[2][k]:hi[2][k] + 1, lo[1][k]:hi[1][k] + 1, lo[0][k]:hi[0][k] + 1] = True
    return touched


def _touched_voxels(vol, touched):
    """Per voxel of the touched units: its global index (gx, gy, gz) and its centre (px, py, pz; f64)."""
    voxel = vol["voxel"]
    L = float(UNIT) * voxel
    uz, uy, ux = np.nonzero(touched)
    k = np.arange(UNIT)
    kz, ky, kx = np.meshgrid(k, k, k, indexing="ij")

    def axis(u, kk, a):          # per touched unit and voxel of the unit: global voxel index, centre
        g = (u[:, None, None, None] * UNIT + kk[None]).reshape(-1)
        c = ((vol["u0"][a] + u).astype(np.float64) * L)[:, None, None, None] + ((kk.astype(np.float64) + 0.5) * voxel)[None]
        return g, c.reshape(-1)

    gx, px = axis(ux, kx, 0)
    gy, py = axis(uy, ky, 1)
    gz, pz = axis(uz, kz, 2)
    return gx, gy, gz, px, py, pz


def integrate(vol, depth, rgb8, intr, extr):
    """One view into the running means (in place); returns the touched units."""
    fx, fy, cx, cy = (float(v) for v in intr)
    E = np.asarray(extr, np.float64).reshape(4, 4)
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    touched = touch(vol, depth, intr, E)
    truncf = f32(vol["trunc"])
    if not touched.any():
        return touched
    gx, gy, gz, px, py, pz = _touched_voxels(vol, touched)
    X = E[0, 0] * px + E[0, 1] * py + E[0, 2] * pz + E[0, 3]
    Y = E[1, 0] * px + E[1, 1] * py + E[1, 2] * pz + E[1, 3]
    Z = E[2, 0] * px + E[2, 1] * py + E[2, 2] * pz + E[2, 3]
    with np.errstate(divide="ignore", invalid="ignore"):
        uf = fx * X / Z + cx + 0.5
        vf = fy * Y / Z + cy + 0.5
        m = (Z > 0) & (uf >= 1e-4) & (uf < W - 1e-4) & (vf >= 1e-4) & (vf < H - 1e-4)
    gx, gy, gz, Z, uf, vf = gx[m], gy[m], gz[m], Z[m], uf[m], vf[m]
    u, v = uf.astype(np.int64), vf.astype(np.int64)
    d = depth[v, u]
    m = d > 0
    gx, gy, gz, Z, u, v, d = gx[m], gy[m], gz[m], Z[m], u[m], v[m], d[m]
    a = (u.astype(f32) - f32(cx)) / f32(fx)
    c = (v.astype(f32) - f32(cy)) / f32(fy)
    sdf = (d - Z.astype(f32)) * np.sqrt(a * a + c * c + f32(1))
    m = sdf > -truncf
    gx, gy, gz, u, v, sdf = gx[m], gy[m], gz[m], u[m], v[m], sdf[m]
    t = np.minimum(f32(1), sdf / truncf)
    w = vol["weight"][gz, gy, gx]
    w1 = w + f32(1)
    vol["tsdf"][gz, gy, gx] = (vol["tsdf"][gz, gy, gx] * w + t) / w1
    for ch in range(3):
        vol["color"][ch][gz, gy, gx] = (vol["color"][ch][gz, gy, gx] * w + rgb8[v, u, ch].astype(f32)) / w1
    vol["weight"][gz, gy, gx] = w1
    assert vol["tsdf"].dtype == f32 and vol["color"].dtype == f32 and vol["weight"].dtype == f32
    return touched


def integration_census(vol, depth, intr, extr):
    """Where the voxels of one view's touched units end in integrate()'s chain of tests: a dict of counts -- `behind` (Z <= 0),
    `outside` the frame, on a `hole` (d == 0), `beyond` (sdf <= -trunc), `updated`, and of those `clamped` (t == 1) -- plus
    `voxels`, their number: behind + outside + hole + beyond + updated.  The volume is not changed."""
    fx, fy, cx, cy = (float(v) for v in intr)
    E = np.asarray(extr, np.float64).reshape(4, 4)
    depth = np.asarray(depth, f32)
    H, W = depth.shape
    touched = touch(vol, depth, intr, E)
    out = dict.fromkeys(("voxels", "behind", "outside", "hole", "beyond", "clamped", "updated"), 0)
    if not touched.any():
        return out
    _, _, _, px, py, pz = _touched_voxels(vol, touched)
    X = E[0, 0] * px + E[0, 1] * py + E[0, 2] * pz + E[0, 3]
    Y = E[1, 0] * px + E[1, 1] * py + E[1, 2] * pz + E[1, 3]
    Z = E[2, 0] * px + E[2, 1] * py + E[2, 2] * pz + E[2, 3]
    front = Z > 0
    with np.errstate(divide="ignore", invalid="ignore"):
        uf = fx * X / Z + cx + 0.5
        vf = fy * Y / Z + cy + 0.5
        inside = front & (uf >= 1e-4) & (uf < W - 1e-4) & (vf >= 1e-4) & (vf < H - 1e-4)
    Z, u, v = Z[inside], uf[inside].astype(np.int64), vf[inside].astype(np.int64)
    d = depth[v, u]
    seen = d > 0
    Z, u, v, d = Z[seen], u[seen], v[seen], d[seen]
    a = (u.astype(f32) - f32(cx)) / f32(fx)
    c = (v.astype(f32) - f32(cy)) / f32(fy)
    sdf = (d - Z.astype(f32)) * np.sqrt(a * a + c * c + f32(1))
    near = sdf > -f32(vol["trunc"])
    t = np.minimum(f32(1), sdf[near] / f32(vol["trunc"]))
    out.update(voxels=len(px), behind=int((~front).sum()), outside=int((front & ~inside).sum()), hole=int((~seen).sum()),
               beyond=int((~near).sum()), clamped=int((t == 1).sum()), updated=int(near.sum()))
    return {k: int(n) for k, n in out.items()}


def integrate_voxel_f64(centre, depth, rgb8, intr, extr, trunc):
    """One voxel of one view into an EMPTY volume, in Python floats (f64), from the rule as include/gsr.h states it for
    gsr_fusion_integrate -- one voxel at a time, no arrays, nothing shared with integrate() above.  centre: the voxel's centre
    (x, y, z).  -> dict: `updated` (bool) and, as far as the chain of tests got, Z, uf, vf (the pixel coordinates before
    truncation), d, norm (the depth-to-distance factor), sdf, and for an updated voxel tsdf (= t: the mean of one sample) and
    color (rgb8[v, u] as a tuple)."""
    import math
    fx, fy, cx, cy = (float(v) for v in intr)
    E = [[float(extr[r][c]) for c in range(4)] for r in range(3)]
    x, y, z = (float(v) for v in centre)
    H, W = len(depth), len(depth[0])
    X, Y, Z = (E[r][0] * x + E[r][1] * y + E[r][2] * z + E[r][3] for r in range(3))
    res = {"updated": False, "Z": Z}
    if not Z > 0.0:
        return res
    uf, vf = fx * X / Z + cx + 0.5, fy * Y / Z + cy + 0.5
    res.update(uf=uf, vf=vf)
    if not (1e-4 <= uf < W - 1e-4 and 1e-4 <= vf < H - 1e-4):
        return res
    u, v = int(uf), int(vf)
    d = float(depth[v][u])
    res["d"] = d
    if not d > 0.0:
        return res
    norm = math.sqrt(((u - cx) / fx) ** 2 + ((v - cy) / fy) ** 2 + 1.0)
    sdf = (d - Z) * norm
    res.update(norm=norm, sdf=sdf)
    if not sdf > -float(trunc):
        return res
    res.update(updated=True, tsdf=min(1.0, sdf / float(trunc)), color=tuple(int(ch) for ch in rgb8[v][u]))
    return res


# ------------------------------------------------------------------------------------------------ marching cubes
def _centres(vol, a):
    n = int(UNIT * vol["nu"][a])
    k = np.arange(n)
    L = float(UNIT) * vol["voxel"]
    return ((vol["u0"][a] + k // UNIT).astype(np.float64) * L + ((k % UNIT).astype(np.float64) + 0.5) * vol["voxel"]).astype(f32)


def marching_cubes(vol, table=None, counts=False):
    """-> (verts [Nv,3] f32, faces [Nf,3] int32, colors [Nv,3] f32), in the order the kernels emit them.  With `counts` a
    fourth item: what gsr_fusion_count writes per voxel -- edge_mask uint8 (bit a: the edge along axis a carries a vertex),
    vert_count and tri_count int32 [voxels] -- and, per cube, `valid` (bool) and `case` (0..255) [voxels]."""
    if table is None:
        from gaustar_amd import fusion
        table = fusion.mc_table()
    tsdf, w = vol["tsdf"], vol["weight"]
    nz, ny, nx = tsdf.shape
    N = nz * ny * nx
    have = w != 0
    inside = tsdf < 0
    sl = lambda o, n: slice(o, n - 1 + o)
    valid = np.zeros((nz, ny, nx), bool)                      # cube at its lowest corner
    v = np.ones((nz - 1, ny - 1, nx - 1), bool)
    case = np.zeros((nz - 1, ny - 1, nx - 1), np.int64)
    for i in range(8):
        dx, dy, dz = i & 1, (i >> 1) & 1, i >> 2
        v &= have[sl(dz, nz), sl(dy, ny), sl(dx, nx)]
        case |= inside[sl(dz, nz), sl(dy, ny), sl(dx, nx)].astype(np.int64) << i
    valid[:-1, :-1, :-1] = v
    cases = np.zeros((nz, ny, nx), np.int64)
    cases[:-1, :-1, :-1] = case
    pad = np.pad(valid, ((1, 0), (1, 0), (1, 0)))             # pad[z + 1, y + 1, x + 1] = valid[z, y, x]; index 0 = cube -1: invalid
    shift = lambda dz, dy, dx: pad[1 - dz:1 - dz + nz, 1 - dy:1 - dy + ny, 1 - dx:1 - dx + nx]   # valid[z - dz, y - dy, x - dx]
    em = np.zeros((nz, ny, nx, 3), bool)
    axes_zyx = {0: 2, 1: 1, 2: 0}                             # xyz axis -> array axis
    for a in range(3):
        hi_have = np.zeros_like(have)
        hi_in = np.zeros_like(inside)
        src = [slice(None)] * 3
        dst = [slice(None)] * 3
        src[axes_zyx[a]], dst[axes_zyx[a]] = slice(1, None), slice(0, -1)
        hi_have[tuple(dst)] = have[tuple(src)]
        hi_in[tuple(dst)] = inside[tuple(src)]
        crossing = have & hi_have & (inside != hi_in)
        b, c = (1 if a == 0 else 0), (1 if a == 2 else 2)
        around = np.zeros_like(have)
        for k in range(4):
            o = [0, 0, 0]
            o[b], o[c] = k & 1, k >> 1
            around |= shift(o[2], o[1], o[0])
        em[..., a] = crossing & around
    em = em.reshape(N, 3)
    cnt = em.sum(1)
    vid = (np.cumsum(cnt) - cnt)[:, None] + np.cumsum(em, 1) - em
    vox, ax = np.nonzero(em)
    z, y, x = np.unravel_index(vox, (nz, ny, nx))
    cen = [_centres(vol, 0), _centres(vol, 1), _centres(vol, 2)]
    verts = np.stack([cen[0][x], cen[1][y], cen[2][z]], 1).astype(f32)
    step = np.array([1, nx, nx * ny])
    other = vox + step[ax]
    fa, fb = tsdf.reshape(-1)[vox], tsdf.reshape(-1)[other]
    t = fa / (fa - fb)
    idx = np.stack([x, y, z], 1)
    pa = verts[np.arange(len(vox)), ax]
    pb = np.choose(ax, [cen[0][np.minimum(x + 1, nx - 1)], cen[1][np.minimum(y + 1, ny - 1)], cen[2][np.minimum(z + 1, nz - 1)]])
    verts[np.arange(len(vox)), ax] = pa + t * (pb - pa)
    col = vol["color"].reshape(3, N)
    ca, cb = col[:, vox].T, col[:, other].T
    colors = ((ca + t[:, None] * (cb - ca)) / f32(255)).astype(f32)
    assert t.dtype == f32 and verts.dtype == f32 and idx.shape[1] == 3
    # triangles
    ntri = (table >= 0).sum(1) // 3
    cube = np.nonzero(valid.reshape(-1) & (ntri[cases.reshape(-1)] > 0))[0]
    cc = cases.reshape(-1)[cube]
    e_axis = np.arange(12) >> 2
    e_off = np.zeros(12, np.int64)
    for e in range(12):
        a, j = e >> 2, e & 3
        b, c = (1 if a == 0 else 0), (1 if a == 2 else 2)
        o = [0, 0, 0]
        o[b], o[c] = j & 1, j >> 1
        e_off[e] = o[0] + o[1] * nx + o[2] * nx * ny
    rows = table[cc][:, :15].reshape(-1, 5, 3)
    used = rows[..., 0] >= 0
    e = np.where(rows >= 0, rows, 0)
    ids = vid[cube[:, None, None] + e_off[e], e_axis[e]]
    assert em[cube[:, None, None] + e_off[e], e_axis[e]][used].all()
    faces = ids[used].astype(np.int32)
    if counts:
        tri_count = np.where(valid.reshape(-1), ntri[cases.reshape(-1)], 0).astype(np.int32)
        return verts, faces, colors, {"edge_mask": (em << np.arange(3)).sum(1).astype(np.uint8), "vert_count": cnt.astype(np.int32),
                                      "tri_count": tri_count, "valid": valid.reshape(-1), "case": cases.reshape(-1)}
    return verts, faces, colors


# ------------------------------------------------------------------------------------------------ mesh checks and inputs
def directed_edge_stats(faces):
    """(closed, euler): closed = every undirected edge lies in exactly two triangles, with opposite directions."""
    f = np.asarray(faces, np.int64)
    d = np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]])
    und, cnt = np.unique(np.sort(d, 1), axis=0, return_counts=True)
    key = d[:, 0] * (f.max() + 1) + d[:, 1]
    rev = d[:, 1] * (f.max() + 1) + d[:, 0]
    closed = bool((cnt == 2).all() and len(np.unique(key)) == len(key) and np.isin(rev, key).all())
    return closed, int(len(np.unique(f)) - len(und) + len(f))


def signed_volume(verts, faces):
    v = np.asarray(verts, np.float64)[np.asarray(faces, np.int64)]
    return float(np.einsum("ij,ij->i", v[:, 0], np.cross(v[:, 1], v[:, 2])).sum() / 6.0)


def sphere_view(centre, radius, intr, extr, H, W, colour=(200, 120, 40), min_cos=0.5):
    """Analytic (depth [H,W] f32, rgb8 [H,W,3] uint8) of a sphere: pixel (i, j)'s ray through ((j - cx) / fx, (i - cy) / fy, 1)
    meets it at depth z (the nearer root); pixels that miss it, or see it at a grazing angle (cos between the ray and the
    normal below min_cos -- where one pixel spans many voxels of depth, the part the reference's edge removal drops), are 0."""
    fx, fy, cx, cy = intr
    E = np.asarray(extr, np.float64)
    cc = E[:3, :3] @ np.asarray(centre, np.float64) + E[:3, 3]
    i, j = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    dirs = np.stack([(j - cx) / fx, (i - cy) / fy, np.ones_like(i)], -1)
    A = (dirs * dirs).sum(-1)
    B = dirs @ cc
    disc = B * B - A * (cc @ cc - radius * radius)
    hit = disc > 0
    s = (B - np.sqrt(np.where(hit, disc, 0))) / A
    n = (s[..., None] * dirs - cc) / radius
    cos = -(n * dirs).sum(-1) / np.sqrt(A)
    depth = np.where(hit & (s > 0) & (cos >= min_cos), s, 0).astype(f32)
    rgb8 = np.zeros((H, W, 3), np.uint8)
    rgb8[depth > 0] = colour
    return depth, rgb8


def look_at_extrinsic(eye, target, up=(0.0, 1.0, 0.0)):
    """A COLMAP-axes (x right, y down, z forward) world-to-camera matrix at `eye` looking at `target`."""
    eye, target = np.asarray(eye, np.float64), np.asarray(target, np.float64)
    z = target - eye
    z /= np.linalg.norm(z)
    upv = np.asarray(up, np.float64)
    if abs(z @ upv) > 0.99:
        upv = np.array([1.0, 0.0, 0.0])
    x = np.cross(z, upv)
    x /= np.linalg.norm(x)
    y = np.cross(z, x)
    E = np.eye(4)
    E[:3, :3] = np.stack([x, y, z])
    E[:3, 3] = -E[:3, :3] @ eye
    return E


def sphere_rig(centre, dist=3.0):
    """14 extrinsics around `centre`: the 6 axis and the 8 cube-diagonal directions."""
    dirs = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
    dirs += [(a, b, c) for a in (-1, 1) for b in (-1, 1) for c in (-1, 1)]
    c = np.asarray(centre, np.float64)
    return [look_at_extrinsic(c + dist * np.asarray(d, np.float64) / np.linalg.norm(d), c) for d in dirs]
