"""The numpy restatement of the density field (include/gsr.h's gsr_density_eval, gsr_density.hip) and of postprocess_mesh
(gaustar_amd/harness.py): float64 from the f32 inputs, every operation in the stated order, the row's sum by the same tree.
numpy's array arithmetic rounds every operation on its own (no contraction)."""
import numpy as np

ROW = 16          # lanes per query: slot j and slot j + 16 share a lane
MAX_K = 32


def rotation(q):
    """pytorch3d's quaternion_to_matrix with producers.quaternion_to_matrix's expressions, q [...,4] f64 -> nine arrays R[a][b]."""
    r, i, j, k = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    two_s = 2.0 / (((r * r + i * i) + j * j) + k * k)
    return ((1.0 - two_s * (j * j + k * k), two_s * (i * j - k * r), two_s * (i * k + j * r)),
            (two_s * (i * j + k * r), 1.0 - two_s * (i * i + k * k), two_s * (j * k - i * r)),
            (two_s * (i * k - j * r), two_s * (j * k + i * r), 1.0 - two_s * (i * i + j * j)))


def mahalanobis2(x, c, q, s):
    """m of include/gsr.h for f32 arrays that broadcast: x, c [...,3], q [...,4], s [...,3] -> f64, clamped as selects."""
    x, c, q, s = (np.asarray(a, np.float32).astype(np.float64) for a in (x, c, q, s))
    with np.errstate(all="ignore"):
        d0, d1, d2 = x[..., 0] - c[..., 0], x[..., 1] - c[..., 1], x[..., 2] - c[..., 2]
        R = rotation(q)
        w = []
        for a in range(3):
            sa = s[..., a]
            inv = 1.0 / np.where(sa < 1e-8, 1e-8, sa)
            w.append(inv * ((R[0][a] * d0 + R[1][a] * d1) + R[2][a] * d2))
        m = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]
        return np.where(m < 0.0, 0.0, np.where(m > 1e8, 1e8, m))     # (a NaN fails both comparisons and stays)


def terms(x, idx, points, scaling, quaternions, strengths, density_factor=1.0):
    """t [Q,K] f64: (f64(f32 density_factor) f64(strength)) exp(-0.5 m) per slot, +0.0 where idx is -1."""
    idx = np.asarray(idx, np.int64)
    have = idx >= 0
    j = np.where(have, idx, 0)
    x = np.asarray(x, np.float32)
    strengths = np.asarray(strengths, np.float32).reshape(-1)
    m = mahalanobis2(x[:, None, :], np.asarray(points, np.float32)[j], np.asarray(quaternions, np.float32)[j],
                     np.asarray(scaling, np.float32)[j])
    with np.errstate(all="ignore"):
        t = (np.float64(np.float32(density_factor)) * strengths[j].astype(np.float64)) * np.exp(-0.5 * m)
    return np.where(have, t, 0.0)


def row_sum(t):
    """[Q,K] f64, K <= 32 -> [Q] f64: slots beyond K are +0.0; u_j = t_j + t_{j+16}; rounds r = 1, 2, 4, 8 of u_j + u_{j xor r}."""
    Q, K = t.shape
    assert 1 <= K <= MAX_K
    pad = np.zeros((Q, MAX_K))
    pad[:, :K] = t
    with np.errstate(all="ignore"):
        u = pad[:, :ROW] + pad[:, ROW:]
        lanes = np.arange(ROW)
        for r in (1, 2, 4, 8):
            u = u + u[:, lanes ^ r]
    return u[:, 0]


def density(x, idx, points, scaling, quaternions, strengths, density_factor=1.0):
    """-> (density [Q] f32, neighbor_opacities [Q,K] f32)."""
    t = terms(x, idx, points, scaling, quaternions, strengths, density_factor)
    with np.errstate(all="ignore"):
        return row_sum(t).astype(np.float32), t.astype(np.float32)


def ulp_diff(a, b):
    """Per element the distance in f32 steps between two finite or equal values (NaN with NaN, inf with inf: 0)."""
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    same = (np.isnan(a) & np.isnan(b)) | (a == b)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    bad = np.isnan(a) != np.isnan(b)
    return np.where(same, 0, np.where(bad, np.int64(2) ** 40, np.abs(ia - ib)))


# ------------------------------------------------------------------------------------------------ the border clean-up
def peel(faces, iterations):
    """refined_mesh.py:1169-1177 with every face inside at the start: per iteration a face stays iff each of its three
    edges occurs at least twice among the faces still there (np.unique counts) -> (mask [F] bool, kept per iteration)."""
    faces = np.asarray(faces, np.int64)
    mask = np.ones(len(faces), bool)
    kept = []
    for _ in range(iterations):
        f = faces[mask]
        e = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1).reshape(-1, 2)
        e = np.sort(e, axis=1)
        _, inv, cnt = np.unique(e, axis=0, return_inverse=True, return_counts=True)
        inside = (cnt[inv.reshape(-1)].reshape(-1, 3) >= 2).all(1)
        mask[np.nonzero(mask)[0]] = inside
        kept.append(int(mask.sum()))
    return mask, kept


def face_centres(verts, faces):
    v = np.asarray(verts, np.float32)[np.asarray(faces, np.int64)]
    return ((v[:, 0] + v[:, 1]) + v[:, 2]) / np.float32(3)


def postprocess(verts, faces, points, scaling, quaternions, strengths, iterations, threshold, K, knn):
    """-> (face_mask, kept per iteration, restored, densities of the removed centres); knn(q, c, K) -> idx with -1."""
    mask, kept = peel(faces, iterations)
    removed = np.nonzero(~mask)[0]
    restored, dens = 0, np.zeros(0, np.float32)
    if removed.size:
        c = face_centres(verts, faces)[removed]
        dens, _ = density(c, knn(c, points, K), points, scaling, quaternions, strengths)
        back = dens > np.float32(threshold)
        mask[removed] = back
        restored = int(back.sum())
    return mask, kept, restored, dens
