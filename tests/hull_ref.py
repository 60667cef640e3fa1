"""numpy restatement of shape from silhouettes (gaustar_amd/csrc/gsr_hull.hip behind gaustar_amd.hull) for tests/test_hull.py and
tests/test_gpu_hull.py: a mask's capped signed squared distance, the carve of a volume by a rig, its TSDF, and hull_bounds.

The rules are those include/gsr.h states; every float expression below has the kernel's operations in the kernel's order
(numpy does not contract a * b + c; the kernels are compiled with contraction off).  The distance is written from its definition
(two unsigned transforms, one per kind, each a row scan and a column window), not from the kernel's signed one-pass form.
The volume is tests/fusion_ref.py's dict with `field` (f32, +inf) and `count` (int32, 0) added; fusion_ref.marching_cubes reads
it after finish()."""
import numpy as np

import fusion_ref as fr

ZNEAR = 0.01
f32 = np.float32


# ------------------------------------------------------------------------------------------------ distance
def _capped_sq_distance_to(target, R):
    """[H,W] int: min(R^2, squared distance to the nearest True pixel of `target`), R^2 where there is none within R."""
    H, W = target.shape
    big = 4 * (H + W + R)
    col = np.arange(W)
    left = np.maximum.accumulate(np.where(target, col, -big), axis=1)                      # nearest True at or before
    right = np.minimum.accumulate(np.where(target, col, big)[:, ::-1], axis=1)[:, ::-1]    # nearest True at or after
    h = np.minimum(np.minimum(col - left, right - col), R).astype(np.int64)                # along the row, capped
    best = np.full((H, W), R * R, np.int64)
    for dy in range(-R, R + 1):
        lo, hi = max(0, -dy), min(H, H - dy)          # rows y with y + dy on the image
        if lo >= hi:
            continue
        cand = dy * dy + h[lo + dy:hi + dy] ** 2
        np.minimum(best[lo:hi], cand, out=best[lo:hi])
    return best


def mask_distance(mask, threshold=128, radius=8):
    """d2 [H,W] int16: +min(R^2, squared distance to the nearest outside pixel) inside, -min(R^2, ... nearest inside pixel)
    outside; inside = mask >= threshold; only pixels of the image count."""
    mask = np.asarray(mask)
    assert mask.dtype == np.uint8 and mask.ndim == 2
    inside = mask.astype(np.int64) >= int(threshold)
    R = int(radius)
    return np.where(inside, _capped_sq_distance_to(~inside, R), -_capped_sq_distance_to(inside, R)).astype(np.int16)


def mask_distance_brute(mask, threshold=128, radius=8):
    """The same from the definition alone, O(n^2): for tiny masks."""
    mask = np.asarray(mask)
    inside = mask.astype(np.int64) >= int(threshold)
    H, W = inside.shape
    ys, xs = np.mgrid[0:H, 0:W]
    out = np.zeros((H, W), np.int16)
    cap = int(radius) ** 2
    for y in range(H):
        for x in range(W):
            other = inside != inside[y, x]
            d = int(((ys[other] - y) ** 2 + (xs[other] - x) ** 2).min()) if other.any() else cap
            out[y, x] = min(cap, d) * (1 if inside[y, x] else -1)
    return out


# ------------------------------------------------------------------------------------------------ the volume
def new_volume(lo, hi, voxel, trunc):
    vol = fr.new_volume(lo, hi, voxel, trunc)
    vol["field"] = np.full(vol["tsdf"].shape, np.inf, f32)
    vol["count"] = np.zeros(vol["tsdf"].shape, np.int32)
    return vol


def centres(vol, a):
    """The voxel centres along axis a (0 = x) in f64, as the kernels form them."""
    n = int(fr.UNIT * vol["nu"][a])
    k = np.arange(n)
    L = float(fr.UNIT) * vol["voxel"]
    return (vol["u0"][a] + k // fr.UNIT).astype(np.float64) * L + ((k % fr.UNIT).astype(np.float64) + 0.5) * vol["voxel"]


def camera(extr, intr, cx, cy, d2):
    extr, intr = np.asarray(extr, np.float64), np.asarray(intr, np.float64)
    return {"R": extr[:3, :3].copy(), "t": extr[:3, 3].copy(), "fx": float(intr[0, 0]), "fy": float(intr[1, 1]), "cx": float(cx),
            "cy": float(cy), "d2": np.asarray(d2, np.int16)}


def phi(e):
    e = e.astype(np.int64)
    r = np.sqrt(np.abs(e).astype(np.float64)) - 0.5
    return np.where(e < 0, -r, r)


def view_distance(cam, px, py, pz):
    """One camera at the points (px, py, pz) f64 -> (constrains [N] bool, d [N] f32; 0 where it does not constrain)."""
    R, t = cam["R"], cam["t"]
    H, W = cam["d2"].shape
    qx = ((R[0, 0] * px + R[0, 1] * py) + R[0, 2] * pz) + t[0]
    qy = ((R[1, 0] * px + R[1, 1] * py) + R[1, 2] * pz) + t[1]
    qz = ((R[2, 0] * px + R[2, 1] * py) + R[2, 2] * pz) + t[2]
    with np.errstate(all="ignore"):
        u = cam["fx"] * (qx / qz) + cam["cx"]
        v = cam["fy"] * (qy / qz) + cam["cy"]
        ok = (qz > ZNEAR) & (u >= 0.0) & (u <= float(W - 1)) & (v >= 0.0) & (v <= float(H - 1))
    u, v, z = np.where(ok, u, 0.0), np.where(ok, v, 0.0), np.where(ok, qz, 1.0)
    x0 = np.minimum(np.floor(u).astype(np.int64), W - 2)
    y0 = np.minimum(np.floor(v).astype(np.int64), H - 2)
    a, b = u - x0.astype(np.float64), v - y0.astype(np.float64)
    d2 = cam["d2"]
    p00, p01, p10, p11 = phi(d2[y0, x0]), phi(d2[y0, x0 + 1]), phi(d2[y0 + 1, x0]), phi(d2[y0 + 1, x0 + 1])
    top = p00 + a * (p01 - p00)
    bot = p10 + a * (p11 - p10)
    ph = top + b * (bot - top)
    scale = 2.0 / (cam["fx"] + cam["fy"])
    d = ((ph * z) * scale).astype(f32)
    return ok, np.where(ok, d, f32(0))


def carve(vol, cams):
    """The cameras into field / count, in place."""
    cz, cy, cx = np.meshgrid(centres(vol, 2), centres(vol, 1), centres(vol, 0), indexing="ij")
    px, py, pz = cx.reshape(-1), cy.reshape(-1), cz.reshape(-1)
    field, count = vol["field"].reshape(-1), vol["count"].reshape(-1)
    for cam in cams:
        ok, d = view_distance(cam, px, py, pz)
        field[:] = np.where(ok & (d < field), d, field)
        count[:] = count + ok.astype(np.int32)
    assert field.dtype == f32 and count.dtype == np.int32
    return vol


def finish(vol, min_views):
    """tsdf, weight and the touched units [nuz,nuy,nux] bool."""
    have = vol["count"] >= int(min_views)
    with np.errstate(all="ignore"):
        t = np.clip(-vol["field"].astype(np.float64) / vol["trunc"], -1.0, 1.0).astype(f32)
    vol["weight"][...] = have.astype(f32)
    vol["tsdf"][...] = np.where(have, t, f32(0))
    near = have & (np.abs(vol["tsdf"]) < 1)
    nz, ny, nx = (int(n) for n in vol["nu"][::-1])
    U = fr.UNIT
    return near.reshape(nz, U, ny, U, nx, U).any(axis=(1, 3, 5))


# ------------------------------------------------------------------------------------------------ host rules of gaustar_amd.hull
def rig_cameras(rig, d2s, use_principal_point=False):
    """The carve's cameras of a `cmr` rig: the principal point at the image's centre (W / 2, H / 2), or the intrinsics' own."""
    out = []
    for i, d2 in enumerate(d2s):
        H, W = (int(v) for v in rig["shape"][i])
        intr = np.asarray(rig["intrinsics"][i], np.float64)
        cx, cy = (intr[0, 2], intr[1, 2]) if use_principal_point else (W / 2, H / 2)
        out.append(camera(rig["extrinsics"][i], intr, cx, cy, d2))
    return out


def radius_for(rig, lo, hi, trunc):
    """The smallest R with (R - 0.5) z_min / f_max >= trunc over the box's corners, capped to [1, 127]."""
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    corners = np.array([[(lo, hi)[i][0], (lo, hi)[j][1], (lo, hi)[k][2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    extr, intr = np.asarray(rig["extrinsics"], np.float64), np.asarray(rig["intrinsics"], np.float64)
    z = np.einsum("cj,nj->cn", extr[:, 2, :3], corners) + extr[:, 2, 3:4]
    z_min, f_max = float(z.min()), float(max(intr[:, 0, 0].max(), intr[:, 1, 1].max()))
    if not z_min > ZNEAR:
        return 127
    return int(min(127, max(1, np.ceil(trunc * f_max / z_min + 0.5))))


def hull_bounds(rig, masks, lo, hi, coarse_voxel=0.032, pad=None, threshold=128, min_views=None):
    """(lo, hi) f64: the box of the centres of the coarse voxels within the truncation (2 coarse voxels) of the hull's inside,
    padded by `pad` (default: one coarse voxel)."""
    trunc = 2.0 * coarse_voxel
    vol = new_volume(lo, hi, coarse_voxel, trunc)
    L = fr.UNIT * float(coarse_voxel)
    R = radius_for(rig, vol["u0"] * L, (vol["u0"] + vol["nu"]) * L, trunc)      # over the volume's own extent, padding included
    carve(vol, rig_cameras(rig, [mask_distance(m, threshold, R) for m in masks]))
    C = len(masks)
    finish(vol, max(min(2, C), C // 4, 1) if min_views is None else min_views)      # gaustar_amd.hull.default_min_views
    near = (vol["weight"] == 1) & (vol["tsdf"] < 1)
    if not near.any():
        raise ValueError("the hull is empty")
    pad = coarse_voxel if pad is None else float(pad)
    out_lo, out_hi = np.zeros(3), np.zeros(3)
    for a in range(3):
        hit = np.nonzero(near.any(axis=tuple(k for k in range(3) if k != 2 - a)))[0]
        c = centres(vol, a)
        out_lo[a], out_hi[a] = c[hit[0]] - pad, c[hit[-1]] + pad
    return out_lo, out_hi


# ------------------------------------------------------------------------------------------------ the scenes of the tests
def look_at_rig(eyes, target, H, W, focal):
    """A `cmr` rig of look-at cameras (COLMAP axes) with one image size and focal length."""
    C = len(eyes)
    intr = np.tile(np.array([[focal, 0.0, W / 2], [0.0, focal, H / 2], [0.0, 0.0, 1.0]]), (C, 1, 1))
    extr = np.stack([fr.look_at_extrinsic(e, target) for e in eyes])
    return {"intrinsics": intr, "extrinsics": extr, "shape": np.tile(np.array([[H, W]], np.int32), (C, 1))}


def ring_eyes(n, dist, elevations=(0.35, -0.3), centre=(0.0, 0.0, 0.0)):
    """n eyes at `dist` from `centre`, evenly in azimuth, alternating between the elevations (radians)."""
    out = []
    for i in range(n):
        az, el = 2.0 * np.pi * i / n + 0.2, elevations[i % len(elevations)]
        out.append(np.asarray(centre, np.float64) + dist * np.array([np.cos(el) * np.cos(az), np.sin(el), np.cos(el) * np.sin(az)]))
    return out


def torus(R=0.2, r=0.07, n_major=48, n_minor=24, centre=(0.0, 0.0, 0.0)):
    """A torus around the y axis: (verts [V,3] f64, faces [F,3] int64), outward orientation."""
    i, j = np.meshgrid(np.arange(n_major), np.arange(n_minor), indexing="ij")
    th, ph = 2 * np.pi * i / n_major, 2 * np.pi * j / n_minor
    v = np.stack([(R + r * np.cos(ph)) * np.cos(th), r * np.sin(ph), (R + r * np.cos(ph)) * np.sin(th)], -1).reshape(-1, 3)
    idx = lambda a, b: (a % n_major) * n_minor + (b % n_minor)
    f = np.concatenate([np.stack([idx(i, j), idx(i, j + 1), idx(i + 1, j)], -1).reshape(-1, 3),
                        np.stack([idx(i + 1, j), idx(i, j + 1), idx(i + 1, j + 1)], -1).reshape(-1, 3)])
    return v + np.asarray(centre, np.float64), f.astype(np.int64)


def render_masks(verts, faces, rig, use_principal_point=False):
    """The silhouettes of a mesh over the rig (meshdepth_ref.render; the principal point as rig_cameras): [mask [H,W] u8]."""
    import meshdepth_ref as mr
    out = []
    for i in range(len(rig["shape"])):
        H, W = (int(v) for v in rig["shape"][i])
        intr = np.asarray(rig["intrinsics"][i], np.float64)
        cx, cy = (intr[0, 2], intr[1, 2]) if use_principal_point else (W / 2, H / 2)
        out.append(mr.render(verts, faces, mr.cam16(rig["extrinsics"][i], intr, cx, cy), H, W)[1])
    return out


def concat_rigs(*rigs):
    return {k: np.concatenate([r[k] for r in rigs]) for k in ("intrinsics", "extrinsics", "shape")}


VOXEL, TRUNC = 0.008, 0.02
BOX = (np.full(3, -0.1), np.full(3, 0.1))      # with VOXEL and TRUNC: 4 units per axis, [-0.256, 0.256]^3
FOCAL, DIST = 360.0, 3.0                       # the ring cameras: a voxel's footprint is 0.008 * 360 / 3 = 0.96 pixels
AXIS_VOXEL = (36, 30)                          # the voxel column (x, y index) the axis camera looks along


def ring_rig(n, elevations=(0.35, -0.3)):
    """n cameras of 128 x 96 around the origin at DIST: each sees the whole volume of BOX."""
    return look_at_rig(ring_eyes(n, DIST, elevations), (0.0, 0.0, 0.0), 96, 128, FOCAL)


def edge_rig():
    """The rig of the bit-for-bit tests, 9 cameras, principal points read from the intrinsics:
    0-5  ring cameras, 128 x 96;
    6    67 x 45 at 1.5, looking past the object: the object crosses its right border, much of the volume projects off it;
    7    67 x 45, focal 60, 0.22 in front of the origin inside the volume: voxels behind znear, the object cropped above and below;
    8    128 x 96 with identity rotation on the line through voxel column AXIS_VOXEL, principal point cx = W - 1 = 127: that
         column's voxels have q.x = 0 exactly, so u = 127.0 = W - 1 (x0 = W - 2, a = 1); every voxel right of it is off the image."""
    vol = new_volume(BOX[0], BOX[1], VOXEL, TRUNC)
    crop = look_at_rig([(0.3, 0.2, -1.5)], (0.3, 0.0, 0.0), 45, 67, 170.0)
    near = look_at_rig([(0.0, 0.0, -0.22)], (0.0, 0.0, 0.0), 45, 67, 60.0)
    axis = look_at_rig([(0.0, 0.0, -DIST)], (0.0, 0.0, 0.0), 96, 128, FOCAL)
    E = np.eye(4)
    E[:3, 3] = -np.array([centres(vol, 0)[AXIS_VOXEL[0]], centres(vol, 1)[AXIS_VOXEL[1]], -DIST])
    axis["extrinsics"][0] = E
    axis["intrinsics"][0, 0, 2] = 127.0
    return concat_rigs(ring_rig(6), crop, near, axis)


EDGE_MIN_VIEWS = 8                             # of the edge rig's 9: the voxels two of cameras 6, 7, 8 miss have weight 0


def torus_rig():
    """8 ring cameras and one that looks down the torus' axis (y), through its hole."""
    return concat_rigs(ring_rig(8), look_at_rig([(0.0, DIST, 0.0)], (0.0, 0.0, 0.0), 96, 128, FOCAL))


def sphere_mesh():
    from gaustar_amd import scene
    v, f = scene.icosphere(3, 0.1)
    return np.asarray(v, np.float64), np.asarray(f, np.int64)


def torus_mesh():
    return torus(0.065, 0.03)


RADIUS = 7                                     # >= TRUNC * f / z + 0.5 for every camera of the rigs here that sees the object whole


def carved(verts, faces, rig, min_views, use_principal_point=False, order=None, radius=RADIUS):
    """The restatement's volume of a mesh's silhouettes over a rig in BOX: (vol, touched, masks, d2s)."""
    masks = render_masks(verts, faces, rig, use_principal_point)
    d2s = [mask_distance(m, 128, radius) for m in masks]
    vol = new_volume(BOX[0], BOX[1], VOXEL, TRUNC)
    cams = rig_cameras(rig, d2s, use_principal_point)
    carve(vol, cams if order is None else [cams[i] for i in order])
    touched = finish(vol, min_views)
    return vol, touched, masks, d2s


def dilate(mask, k):
    """A boolean mask grown by k pixels (the (2k + 1)^2 square); nothing grows in from beyond the border."""
    m = np.asarray(mask, bool)
    H, W = m.shape
    p = np.pad(m, k)
    out = np.zeros_like(m)
    for dy in range(2 * k + 1):
        for dx in range(2 * k + 1):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def erode(mask, k):
    """A boolean mask shrunk by k pixels; the border itself does not erode it."""
    return ~dilate(~np.asarray(mask, bool), k)


def mask_check(got, want, k):
    """(pixels of `got` outside `want` grown by k, pixels of `want` shrunk by k that `got` misses): both 0 = passed."""
    a, b = np.asarray(got) > 0, np.asarray(want) > 0
    return int((a & ~dilate(b, k)).sum()), int((erode(b, k) & ~a).sum())
