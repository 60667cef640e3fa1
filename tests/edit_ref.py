"""gaustar_amd.edit (gsr_edit.hip) restated in numpy from the rules of include/gsr.h: the rigid fit's exactly rounded sums and
its host rule, the rigid transform, the SH rotation matrices and their application, the half-space selection, the cut, the
merge and the paint.  Written from the rules, operation by operation; numpy neither contracts a product into a sum nor
reorders one, so where the device follows the same order the bits are the same.  The sums of the fit are the exception: the
device adds in a tree, so they are compared against math.fsum within the bound of a sum of m terms, m 2^-53 sum |term|."""
import math

import numpy as np

from tracking_ref import bary_to_point, dot, point_to_bary

F32, F64 = np.float32, np.float64
SH_C0 = 0.28209479177387814
SH_C1 = 0.4886025119029199
SH_C2 = [1.0925484305920792, -1.0925484305920792, 0.31539156525252005, -1.0925484305920792, 0.5462742152960396]
SH_C3 = [-0.5900435899266435, 2.890611442640554, -0.4570457994644658, 0.3731763325901154, -0.4570457994644658, 1.445305721320277,
         -0.5900435899266435]
BARY = {1: [[1 / 3, 1 / 3, 1 / 3]],
        6: [[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12], [5 / 12, 1 / 6, 5 / 12],
            [5 / 12, 5 / 12, 1 / 6]]}


# ------------------------------------------------------------------------------------------------ rigid fit
def fit_valid(src, dst_t):
    return np.isfinite(src).all(-1) & np.isfinite(dst_t).all(-1)


def fit_centroids(src, dst_t):
    """-> n, abar, bbar, and the bound m 2^-53 sum |term| / n of each centroid coordinate (each side's division adds half an ulp)."""
    ok = fit_valid(src, dst_t)
    n = int(ok.sum())
    a, b = src[ok], dst_t[ok]
    if n == 0:
        return 0, np.full(3, np.nan), np.full(3, np.nan), np.zeros(3), np.zeros(3)
    abar = np.array([math.fsum(a[:, i]) for i in range(3)]) / n
    bbar = np.array([math.fsum(b[:, i]) for i in range(3)]) / n
    tol = lambda x, m: (n * 2.0 ** -53 * np.abs(x).sum(0)) / n + 2.0 ** -52 * np.abs(m)
    return n, abar, bbar, tol(a, abar), tol(b, bbar)


def fit_cross(src, dst_t, abar, bbar):
    """H about the GIVEN centroids (the device's own), each term a rounded product of two rounded differences, summed exactly
    -> H [3,3] and its bound n 2^-53 sum |term|."""
    ok = fit_valid(src, dst_t)
    da, db = src[ok] - abar, dst_t[ok] - bbar
    terms = da[:, :, None] * db[:, None, :]
    H = np.array([[math.fsum(terms[:, i, j]) for j in range(3)] for i in range(3)]).reshape(3, 3)
    return H, int(ok.sum()) * 2.0 ** -53 * np.abs(terms).sum(0)


def rigid_from_sums(sums):
    """Per row {n, abar, bbar, H}: svd, R = Vt^T U^T, the reflection fix on Vt's last row, t = bbar - R abar; ok = n >= 3 and
    S[1] > 1e-12 S[0], NaN otherwise.  -> R, t, n, ok, and which rows took the reflection branch."""
    sums = np.asarray(sums, F64).reshape(-1, 16)
    T = len(sums)
    R, t, ok, flipped = np.full((T, 3, 3), np.nan), np.full((T, 3), np.nan), np.zeros(T, bool), np.zeros(T, bool)
    n = sums[:, 0].astype(np.int64)
    for i in range(T):
        if n[i] < 3 or not np.isfinite(sums[i]).all():
            continue
        U, S, Vt = np.linalg.svd(sums[i, 7:].reshape(3, 3))
        Ri = Vt.T @ U.T
        if np.linalg.det(Ri) < 0:
            Vt[2] = -Vt[2]
            Ri = Vt.T @ U.T
            flipped[i] = True
        if S[1] > 1e-12 * S[0]:
            R[i], t[i], ok[i] = Ri, sums[i, 4:7] - Ri @ sums[i, 1:4], True
    return R, t, n, ok, flipped


def fit_rigid(src, dst):
    """The whole fit in numpy (exact sums): for closed-form checks."""
    src, dst = np.asarray(src, F64), np.asarray(dst, F64)
    dst = dst[None] if dst.ndim == 2 else dst
    sums = np.zeros((len(dst), 16))
    for t, b in enumerate(dst):
        n, abar, bbar, _, _ = fit_centroids(src, b)
        sums[t, 0], sums[t, 1:4], sums[t, 4:7] = n, abar, bbar
        if n:
            sums[t, 7:] = fit_cross(src, b, abar, bbar)[0].reshape(-1)
    return rigid_from_sums(sums)


def rotation(rng):
    """A random rotation matrix from a unit quaternion."""
    q = rng.normal(size=4)
    w, x, y, z = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


# ------------------------------------------------------------------------------------------------ moving a model
def transform_points(x, R, t=None):
    """x [n,3] f32 -> f32: per coordinate ((R0 x + R1 y) + R2 z) [+ t] in f64, rounded once."""
    x, R = np.asarray(x, F32).astype(F64), np.asarray(R, F64)
    out = (R[:, 0] * x[:, 0:1] + R[:, 1] * x[:, 1:2]) + R[:, 2] * x[:, 2:3]
    if t is not None:
        out = out + np.asarray(t, F64)
    return out.astype(F32)


def transform_delta_r(q, R):
    """[n,4] f32 (w, x, y, z): the vector part turned, w as it is."""
    out = np.array(q, F32)
    out[:, 1:] = transform_points(out[:, 1:], R)
    return out


def sh_basis(dirs, levels):
    d = np.asarray(dirs, F64)
    x, y, z = d[:, 0], d[:, 1], d[:, 2]
    xx, yy, zz, xy, yz, xz = x * x, y * y, z * z, x * y, y * z, x * z
    cols = [np.full_like(x, SH_C0),
            -SH_C1 * y, SH_C1 * z, -SH_C1 * x,
            SH_C2[0] * xy, SH_C2[1] * yz, SH_C2[2] * (2.0 * zz - xx - yy), SH_C2[3] * xz, SH_C2[4] * (xx - yy),
            SH_C3[0] * y * (3 * xx - yy), SH_C3[1] * xy * z, SH_C3[2] * y * (4 * zz - xx - yy), SH_C3[3] * z * (2 * zz - 3 * xx - 3 * yy),
            SH_C3[4] * x * (4 * zz - xx - yy), SH_C3[5] * z * (xx - yy), SH_C3[6] * x * (xx - 3 * yy)]
    return np.stack(cols[:levels * levels], axis=1)


def fibonacci_sphere(n=32):
    i = np.arange(n, dtype=F64) + 0.5
    z = 1.0 - 2.0 * i / n
    r = np.sqrt(1.0 - z * z)
    phi = i * (np.pi * (3.0 - np.sqrt(5.0)))
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1)


def sh_rotation_matrices(R, levels):
    d = fibonacci_sphere(32)
    Y0, Y1 = sh_basis(d, levels), sh_basis(d @ np.asarray(R, F64), levels)
    D = np.zeros((levels * levels, levels * levels))
    for l in range(levels):
        o, w = l * l, 2 * l + 1
        D[o:o + w, o:o + w] = np.linalg.lstsq(Y0[:, o:o + w], Y1[:, o:o + w], rcond=None)[0]
    return D


def rotate_sh(rest, D):
    """rest [N, M - 1, 3] f32, D [M,M] -> f32: per band the f64 dot in ascending index order from the first product."""
    rest, D = np.asarray(rest, F32), np.asarray(D, F64)
    M = rest.shape[1] + 1
    x = rest.astype(F64)
    out = np.zeros_like(x)
    l = 1
    while l * l < M:
        o, w = l * l, 2 * l + 1
        for i in range(o, o + w):
            s = D[i, o] * x[:, o - 1]
            for k in range(o + 1, o + w):
                s = s + D[i, k] * x[:, k - 1]
            out[:, i - 1] = s
        l += 1
    return out.astype(F32)


# ------------------------------------------------------------------------------------------------ selecting, cutting, merging
def face_centres(verts, faces):
    v = np.asarray(verts, F32).astype(F64)[np.asarray(faces)]
    return ((v[:, 0] + v[:, 1]) + v[:, 2]) / 3.0


def faces_in_halfspaces(verts, faces, groups):
    c = face_centres(verts, faces)
    sel = np.zeros(len(c), bool)
    for g in groups:
        every = np.ones(len(c), bool)
        for a, b, cc, d in np.asarray(g, F64):
            every &= ((a * c[:, 0] + b * c[:, 1]) + cc * c[:, 2]) + d > 0
        sel |= every
    return sel


def plane_through(centre, normal):
    """(a, b, c, d) with d = -((a cx + b cy) + c cz): the plane's value at `centre` is exactly 0."""
    a, b, c = (float(x) for x in normal)
    return np.array([a, b, c, -((a * centre[0] + b * centre[1]) + c * centre[2])])


def cut(verts, faces, params, keep, G):
    """The kept faces in order, their vertices renumbered in ascending old index; per-Gaussian arrays: G rows per kept face."""
    verts, faces, keep = np.asarray(verts), np.asarray(faces), np.asarray(keep, bool)
    kept = faces[keep]
    used = np.zeros(len(verts), bool)
    used[kept.reshape(-1)] = True
    new_id = np.cumsum(used) - 1
    rows = (np.nonzero(keep)[0][:, None] * G + np.arange(G)).reshape(-1)
    return verts[used], new_id[kept], {k: np.asarray(v)[rows] for k, v in params.items()}


def merge(verts_a, faces_a, params_a, verts_b, faces_b, params_b):
    return (np.concatenate([verts_a, verts_b]), np.concatenate([faces_a, np.asarray(faces_b) + len(verts_a)]),
            {k: np.concatenate([params_a[k], params_b[k]]) for k in params_a})


# ------------------------------------------------------------------------------------------------ painting
def gaussian_centres(verts, faces, G):
    """[F G,3] f64: (b0 v0 + b1 v1) + b2 v2 from the f32 vertices and the f32 barycentric table."""
    v = np.asarray(verts, F32).astype(F64)[np.asarray(faces)]                 # [F,3,3]
    b = np.asarray(BARY[G], F32).astype(F64)                                  # [G,3]
    p = (b[None, :, 0, None] * v[:, None, 0] + b[None, :, 1, None] * v[:, None, 1]) + b[None, :, 2, None] * v[:, None, 2]
    return p.reshape(-1, 3)


def paint(verts, faces, G, scales, dc, anchors, uv, triangles, texture, mode="multiply", bary_slack=0.03, max_dist=0.05,
          shrink_scale=-6.0, alpha_min=50):
    """-> scales [N,2] f32, dc [N,3] f32, n_inside (per triangle), n_painted, n_outside, touched [N] bool (inside a triangle)."""
    p = gaussian_centres(verts, faces, G)
    N = len(p)
    scales, dc = np.array(scales, F32).reshape(N, 2), np.array(dc, F32).reshape(N, 3)
    anchors, uv, tex = np.asarray(anchors, F64), np.asarray(uv, F64), np.asarray(texture, np.uint8)
    tex = tex[:, :, None] if tex.ndim == 2 else tex
    h, w, C = tex.shape
    c0 = F32(SH_C0)
    rgb, have, touched = np.zeros((N, 3), F32), np.zeros(N, bool), np.zeros(N, bool)
    n_inside, n_outside = [], 0
    with np.errstate(all="ignore"):
        for tri_idx in np.asarray(triangles):
            t = anchors[tri_idx]
            nb = point_to_bary(np.broadcast_to(t, (N, 3, 3)), p)
            e, g = t[1] - t[0], t[2] - t[1]
            cr = np.array([e[1] * g[2] - e[2] * g[1], e[2] * g[0] - e[0] * g[2], e[0] * g[1] - e[1] * g[0]])
            nrm = -cr / np.sqrt((cr[0] * cr[0] + cr[1] * cr[1]) + cr[2] * cr[2])
            dist = dot(t[0] - p, np.broadcast_to(nrm, (N, 3)))
            inside = (nb >= -bary_slack).all(-1) & (-max_dist < dist) & (dist < max_dist)
            n_inside.append(int(inside.sum()))
            touched |= inside
            tu = uv[tri_idx]
            u = (nb[:, 0] * tu[0, 0] + nb[:, 1] * tu[1, 0]) + nb[:, 2] * tu[2, 0]
            v = (nb[:, 0] * tu[0, 1] + nb[:, 1] * tu[1, 1]) + nb[:, 2] * tu[2, 1]
            row, col = np.trunc(u * h), np.trunc(v * w)
            within = inside & (row >= 0) & (row < h) & (col >= 0) & (col < w)
            n_outside += int((inside & ~within).sum())
            for i in np.nonzero(within)[0]:
                px = tex[int(row[i]), int(col[i])]
                if mode == "replace" and C == 4 and not int(px[3]) > alpha_min:
                    continue
                if not have[i]:
                    rgb[i] = dc[i] * c0 + F32(0.5)
                    have[i] = True
                if mode == "multiply":
                    rgb[i] = rgb[i] * F32(float(px[0]) / 255.0)
                else:
                    rgb[i] = (px[:3].astype(F64) / 255.0).astype(F32)
    if shrink_scale is not None:
        scales[touched] = F32(shrink_scale)
    dc[have] = (rgb[have] - F32(0.5)) / c0
    return scales, dc, n_inside, int(have.sum()), n_outside, touched
