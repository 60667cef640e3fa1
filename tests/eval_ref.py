"""The numpy restatement of gaustar_amd.evaluate (include/gsr.h, "Scoring a result"), operation by operation in float64 --
numpy never contracts a product and a sum -- so that faces, barycentrics, closest points, distances, sample ids, counts and
maxima can be compared with the device bit for bit.  Nothing here mirrors a library: the definitions are the project's own.

    closest(p; a,b,c)   the region test of Ericson 5.1.5 as selects, one reciprocal per pair
    nearest face        the lexicographic minimum of (dist2, face index); one square root, of the winner
    area, weights       gsr_splice_face_areas' statement on f64; w = floor(area 2^(32-e)), max area = mu 2^e, mu in [0.5, 1)
    sample k of n       t_k = k q + min(k, r) + q div 2 over the int64 scan; splitmix64's finaliser for the barycentrics
    distance stats      sum d, sum d d, max, #(d < tau)
    image SSE           (p - g) and its square in f32, widened and summed in f64
"""
import numpy as np

from tracking_ref import bary_to_point, dot

U64 = np.uint64
GOLDEN = U64(0x9E3779B97F4A7C15)


def closest_pairs(p, a, b, c):
    """p, a, b, c [...,3] f64, broadcast against each other -> (dist2 [...], v, w, q [...,3]); u is formed by the caller."""
    p, a, b, c = (np.asarray(x, np.float64) for x in (p, a, b, c))
    with np.errstate(all="ignore"):
        ab, ac, ap, bp, cp = b - a, c - a, p - a, p - b, p - c
        d1, d2, d3, d4, d5, d6 = dot(ab, ap), dot(ac, ap), dot(ab, bp), dot(ac, bp), dot(ab, cp), dot(ac, cp)
        vc, vb, va = d1 * d4 - d3 * d2, d5 * d2 - d1 * d6, d3 * d6 - d5 * d4
        e, g = d4 - d3, d5 - d6
        rA = (d1 <= 0) & (d2 <= 0)
        rB = (d3 >= 0) & (d4 <= d3)
        rAB = (vc <= 0) & (d1 >= 0) & (d3 <= 0)
        rC = (d6 >= 0) & (d5 <= d6)
        rAC = (vb <= 0) & (d2 >= 0) & (d6 <= 0)
        rBC = (va <= 0) & (e >= 0) & (g >= 0)
        zero, one = np.zeros_like(d1), np.ones_like(d1)
        conds = [rA, rB, rAB, rC, rAC, rBC]                      # np.select: the first that holds
        nv = np.select(conds, [zero, one, d1, zero, zero, zero], vb)
        nw = np.select(conds, [zero, zero, zero, one, d2, e], vc)
        den = np.select(conds, [one, one, d1 - d3, one, d2 - d6, e + g], (va + vb) + vc)
        bc = rBC & ~(rA | rB | rAB | rC | rAC)
        r = 1.0 / den
        w = nw * r
        v = np.where(bc, 1.0 - w, nv * r)
        q = a + (ab * v[..., None] + ac * w[..., None])
        d = p - q
        return dot(d, d), v, w, q


def surface_distance(points, verts, faces, block=256):
    """-> (dist [K], face [K] int32, bary [K,3], closest [K,3]); face -1, dist inf, NaN where no face ranks."""
    points, verts = np.asarray(points, np.float64).reshape(-1, 3), np.asarray(verts, np.float64)
    tri = verts[np.asarray(faces, np.int64).reshape(-1, 3)]
    K = len(points)
    face = np.full(K, -1, np.int32)
    dist = np.full(K, np.inf)
    bary = np.full((K, 3), np.nan)
    closest = np.full((K, 3), np.nan)
    for s in range(0, K, block):
        p = points[s:s + block]
        d2, v, w, q = closest_pairs(p[:, None, :], tri[None, :, 0], tri[None, :, 1], tri[None, :, 2])
        key = np.where(np.isnan(d2) | np.isinf(d2), np.inf, d2)
        j = np.argmin(key, axis=1)                               # the lowest index among equals
        rows = np.arange(len(p))
        ok = np.isfinite(d2[rows, j])
        vj, wj = v[rows, j], w[rows, j]
        u = (1.0 - vj) - wj
        u = np.where(u < 0, 0.0, u)
        face[s:s + block] = np.where(ok, j, -1)
        dist[s:s + block] = np.where(ok, np.sqrt(np.where(ok, d2[rows, j], 0.0)), np.inf)
        bary[s:s + block] = np.where(ok[:, None], np.stack([u, vj, wj], -1), np.nan)
        closest[s:s + block] = np.where(ok[:, None], q[rows, j], np.nan)
    return dist, face, bary, closest


def face_areas(verts, faces):
    v = np.asarray(verts, np.float64)
    tri = v[np.asarray(faces, np.int64).reshape(-1, 3)]
    u, w = tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 1]
    cx = u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1]
    cy = u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2]
    cz = u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]
    return 0.5 * np.sqrt((cx * cx + cy * cy) + cz * cz)


def sample_weights(area):
    """int64 [F]; ValueError where no face has a positive, finite area."""
    area = np.asarray(area, np.float64)
    if len(area) == 0:
        raise ValueError("no faces")
    m = area.max()
    if not (np.isfinite(m) and m > 0):
        raise ValueError("no positive, finite area")
    _mu, e = np.frexp(m)                                         # m = mu 2^e, mu in [0.5, 1)
    return np.floor(area * np.ldexp(1.0, 32 - int(e))).astype(np.int64)


def mix64(z):
    z = np.atleast_1d(np.asarray(z, U64))                       # (arrays wrap modulo 2^64 without a warning)
    z = (z ^ (z >> U64(30))) * U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> U64(27))) * U64(0x94D049BB133111EB)
    return z ^ (z >> U64(31))


def sample_ids(weights, n):
    c = np.cumsum(np.asarray(weights, np.int64))
    W = int(c[-1])
    q, r = W // n, W % n
    k = np.arange(n, dtype=np.int64)
    t = k * q + np.minimum(k, r) + q // 2
    return np.searchsorted(c, t, side="right").astype(np.int32)  # the lowest f with c[f] > t


def sample_bary(n, seed):
    k1 = np.arange(1, n + 1, dtype=U64)
    z = mix64(np.full(n, int(seed) & (2 ** 64 - 1), U64) + k1 * GOLDEN)
    s = ((z >> U64(32)).astype(np.float64) + 0.5) * 2.0 ** -32
    t = ((z & U64(0xffffffff)).astype(np.float64) + 0.5) * 2.0 ** -32
    flip = s + t > 1.0
    s, t = np.where(flip, 1.0 - s, s), np.where(flip, 1.0 - t, t)
    return np.stack([(1.0 - s) - t, s, t], -1)


def sample_surface(verts, faces, n, seed=0):
    """-> (face_ids [n] int32, bary [n,3], points [n,3])"""
    verts, faces = np.asarray(verts, np.float64), np.asarray(faces, np.int64).reshape(-1, 3)
    ids = sample_ids(sample_weights(face_areas(verts, faces)), n)
    bary = sample_bary(n, seed)
    return ids, bary, bary_to_point(verts[faces[ids]], bary)


def distance_stats(d, thresholds):
    """-> (sum d, sum d d, max, counts); the sums are numpy's (pairwise), the device's are fixed-order: compare with a bound."""
    d = np.asarray(d, np.float64)
    return float(d.sum()), float((d * d).sum()), float(d.max()) if len(d) else 0.0, [int((d < t).sum()) for t in thresholds]


def image_sse(pred, gt, mask=None, clamp01=False):
    """pred, gt [C,H,W] f32 -> (f64 sum of the f32 squares, count)"""
    p, g = np.asarray(pred, np.float32), np.asarray(gt, np.float32)
    if clamp01:
        p = np.where(p < 0, np.float32(0), np.where(p > 1, np.float32(1), p))
    e = (p - g).astype(np.float32)
    sq = (e * e).astype(np.float32)
    if mask is not None:
        sq = sq[:, np.asarray(mask).astype(bool)]
    return float(sq.astype(np.float64).sum()), int(sq.size)


def psnr(sse, n):
    mse = sse / n
    return np.inf if mse == 0 else 20.0 * np.log10(1.0 / np.sqrt(mse))


# ------------------------------------------------------------------------------------------------ shared cases
TRIANGLE = np.array([[0, 0, 0], [4, 0, 0], [0, 4, 0]], np.float64)
# query, dist2, barycentrics (None: not pinned by the table)
HAND_CASES = [
    ((1, 1, 3), 9, (.5, .25, .25)),     # inside
    ((-1, -1, 2), 6, (1, 0, 0)),        # A
    ((6, -1, 1), 6, (0, 1, 0)),         # B
    ((-1, 6, 1), 6, (0, 0, 1)),         # C
    ((2, -3, 0), 9, (.5, .5, 0)),       # AB
    ((-3, 2, 0), 9, (.5, 0, .5)),       # AC
    ((4, 4, 5), 33, (0, .5, .5)),       # BC
    ((1, 1, 0), 0, (.5, .25, .25)),     # inside, on the face
    ((2, 0, 0), 0, (.5, .5, 0)),        # on an edge
    ((0, 0, 0), 0, (1, 0, 0)),          # on a vertex
]
MIRROR = (np.array([[1, 0, 0], [3, 0, 0], [1, 2, 0], [-1, 0, 0], [-3, 0, 0], [-1, 2, 0]], np.float64),
          np.array([[0, 1, 2], [3, 4, 5]], np.int32), np.array([[0, 1, 2]], np.float64))


def icosphere(level=2):
    """A unit icosphere: 20 4^level faces -> (verts f64, faces int32)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.array(x, np.float64) / np.linalg.norm(x) for x in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(i, j):
            key = (min(i, j), max(i, j))
            if key not in mid:
                x = v[i] + v[j]
                v.append(x / np.linalg.norm(x))
                mid[key] = len(v) - 1
            return mid[key]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.array(v, np.float64), np.array(f, np.int32)


def triangle_soup(F, seed=0):
    rng = np.random.default_rng(seed)
    centre = rng.uniform(-1, 1, size=(F, 1, 3))
    verts = (centre + rng.uniform(-0.3, 0.3, size=(F, 3, 3))).reshape(-1, 3)
    return verts, np.arange(3 * F, dtype=np.int32).reshape(F, 3)
