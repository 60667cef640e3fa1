"""The restatement of the density field and of the border clean-up (tests/density_ref.py) against facts that need no GPU."""
import numpy as np

import density_ref as dr
from gaustar_amd import scene

EPS = 2.0 ** -52


def _one(x, c, q, s, w, factor=1.0):
    d, t = dr.density(np.asarray([x], np.float32), np.zeros((1, 1), np.int64), np.asarray([c], np.float32), np.asarray([s], np.float32),
                      np.asarray([q], np.float32), np.asarray([w], np.float32), factor)
    return d[0], t[0, 0]


def test_one_isotropic_gaussian():
    rng = np.random.default_rng(0)
    for _ in range(50):
        x, c = rng.normal(size=3).astype(np.float32), rng.normal(size=3).astype(np.float32)
        s, w = np.float32(rng.uniform(0.3, 2.0)), np.float32(rng.uniform(0.05, 0.95))
        m = dr.mahalanobis2(x, c, np.float32([1, 0, 0, 0]), np.float32([s, s, s]))
        d = x.astype(np.float64) - c.astype(np.float64)
        want_m = (d * d).sum() / (np.float64(s) * np.float64(s))
        assert abs(m - want_m) <= 8 * EPS * want_m
        got, t = _one(x, c, [1, 0, 0, 0], [s, s, s], w)
        want = np.float64(w) * np.exp(-want_m / 2)
        assert got == t and abs(np.float64(got) - want) <= 2.0 ** -23 * want


def test_equal_scales_make_the_rotation_irrelevant():
    rng = np.random.default_rng(1)
    x, c = rng.normal(size=(200, 3)).astype(np.float32), rng.normal(size=(200, 3)).astype(np.float32)
    q = rng.normal(size=(200, 4)).astype(np.float32)
    s = np.repeat(rng.uniform(0.3, 2.0, (200, 1)), 3, 1).astype(np.float32)
    ident = np.tile(np.float32([1, 0, 0, 0]), (200, 1))
    a, b = dr.mahalanobis2(x, c, q, s), dr.mahalanobis2(x, c, ident, s)
    # the rotation's nine entries, the three dot products and the squares each round: a few tens of 2^-53 relative
    assert np.abs(a - b).max() <= 64 * EPS * np.abs(b).max() and (np.abs(a - b) <= 64 * EPS * b).all()


def test_quaternion_norm_does_not_matter():
    rng = np.random.default_rng(2)
    x, c = rng.normal(size=(200, 3)).astype(np.float32), rng.normal(size=(200, 3)).astype(np.float32)
    s = rng.uniform(0.05, 2.0, (200, 3)).astype(np.float32)
    q = rng.normal(size=(200, 4)).astype(np.float32)
    # powers of two scale every product exactly: bit-equal; any other factor rounds in f32 first, so compare in f64 directly
    assert np.array_equal(dr.mahalanobis2(x, c, q, s), dr.mahalanobis2(x, c, q * np.float32(4), s))
    q64 = q.astype(np.float64)
    R = np.array(dr.rotation(q64)), np.array(dr.rotation(q64 / np.linalg.norm(q64, axis=1, keepdims=True)))
    assert np.abs(R[0] - R[1]).max() <= 16 * EPS


def test_nan_and_clamp_rules():
    one = [1, 0, 0, 0]
    # far away: m is clamped at 1e8 and the term is exactly 0
    assert dr.mahalanobis2(np.float32([1e3, 0, 0]), np.float32([0, 0, 0]), np.float32(one), np.float32([0.01, 1, 1])) == 1e8
    assert _one([1e3, 0, 0], [0, 0, 0], one, [0.01, 1, 1], 0.7) == (0.0, 0.0)
    # a scale of 0 and one below the clamp count as 1e-8
    for s0 in (0.0, 1e-9):
        m = dr.mahalanobis2(np.float32([1e-8, 0, 0]), np.float32([0, 0, 0]), np.float32(one), np.float32([s0, 1, 1]))
        want = (np.float64(np.float32(1e-8)) * (1.0 / 1e-8)) ** 2
        assert m == want
    # NaN goes through the clamp, and through the sum
    assert np.isnan(dr.mahalanobis2(np.float32([np.nan, 0, 0]), np.float32([0, 0, 0]), np.float32(one), np.float32([1, 1, 1])))
    d, t = _one([np.nan, 0, 0], [0, 0, 0], one, [1, 1, 1], 0.5)
    assert np.isnan(d) and np.isnan(t)
    d, t = _one([0, 0, 0], [0, 0, 0], [0, 0, 0, 0], [1, 1, 1], 0.5)      # two_s = 2 / 0 = inf, inf 0 = NaN
    assert np.isnan(d) and np.isnan(t)
    # strength 0, the factor, and an empty slot
    assert _one([0.1, 0, 0], [0, 0, 0], one, [1, 1, 1], 0.0) == (0.0, 0.0)
    a, b = _one([0.1, 0, 0], [0, 0, 0], one, [1, 1, 1], 0.5, 1.0), _one([0.1, 0, 0], [0, 0, 0], one, [1, 1, 1], 0.5, 0.5)
    assert b[0] == np.float32(0.5) * a[0]
    d, t = dr.density(np.zeros((1, 3), np.float32), np.array([[0, -1, -1]]), np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32),
                      np.float32([one]), np.float32([0.25]))
    assert d[0] == np.float32(0.25) and t.tolist() == [[0.25, 0.0, 0.0]]


def test_row_sum_is_the_stated_tree():
    rng = np.random.default_rng(3)
    for K in (1, 15, 16, 17, 32):
        t = rng.uniform(0, 1, (5, K))
        pad = np.zeros((5, 32)); pad[:, :K] = t
        u = pad[:, :16] + pad[:, 16:]
        u = u[:, 0::2] + u[:, 1::2]
        u = u[:, 0::2] + u[:, 1::2]
        u = u[:, 0::2] + u[:, 1::2]
        assert np.array_equal(dr.row_sum(t), u[:, 0] + u[:, 1])


def _strip(n):
    """2 n triangles between two rows of n + 1 vertices."""
    faces = []
    for i in range(n):
        a, b, c, d = i, i + 1, n + 1 + i, n + 2 + i
        faces += [[a, b, c], [b, d, c]]
    return np.array(faces)


def _tube(n, m=3):
    """n segments between n + 1 rings of m vertices, open at both ends: 2 m n triangles, segment s holds faces [2 m s, 2 m (s + 1)),
    per side first the triangle with an edge on ring s, then the one with an edge on ring s + 1."""
    faces = []
    for s in range(n):
        for k in range(m):
            a, b = s * m + k, s * m + (k + 1) % m
            c, d = a + m, b + m
            faces += [[a, b, c], [b, d, c]]
    return np.array(faces)


def test_flat_strip_is_all_border():
    """Every triangle of a flat strip has an edge on one of the two long borders, so by the rule of refined_mesh.py:1173-1177
    (all three edges at least twice) the first peel takes them all, not only the two at the ends."""
    mask, kept = dr.peel(_strip(6), 2)
    assert kept == [0, 0] and not mask.any()


def test_strip_rolled_into_a_tube_loses_its_two_ends_per_peel():
    """The strip whose long borders are closed: a tube of m-gon rings, open only at its ends.  A peel takes, at either end, the m
    triangles with an edge on the end ring; that bares the m triangles between them, which go in the next peel, and then the
    next ring is the end.  So every peel takes 2 m triangles until none remain, and it is the end ones it takes."""
    n, m = 5, 3
    tube = _tube(n, m)
    mask, kept = dr.peel(tube, n + 1)
    assert kept == [max(0, 2 * m * n - 2 * m * (i + 1)) for i in range(n + 1)] and not mask.any()
    gone = np.nonzero(~dr.peel(tube, 1)[0])[0]
    assert sorted(gone) == sorted([2 * k for k in range(m)] + [2 * m * (n - 1) + 2 * k + 1 for k in range(m)])
    mask2 = dr.peel(tube, 2)[0]
    assert not mask2[:2 * m].any() and not mask2[2 * m * (n - 1):].any() and mask2[2 * m:2 * m * (n - 1)].all()


def test_grid_loses_its_outer_ring():
    g = 8
    vid = lambda r, c: r * (g + 1) + c
    grid = np.array([t for r in range(g) for c in range(g) for t in ([vid(r, c), vid(r, c + 1), vid(r + 1, c)],
                                                                       [vid(r, c + 1), vid(r + 1, c + 1), vid(r + 1, c)])])
    mask, kept = dr.peel(grid, 3)
    # 4 g border edges, one triangle each, but for the two corner triangles that hold two of them
    assert kept[0] == len(grid) - (4 * g - 2) and kept[0] > kept[1] > kept[2] > 0


def test_entry_points_validate_without_gpu(hip_lib):
    """gsr_density_pack / gsr_density_eval: argument checks come before any device work."""
    import ctypes
    null = None
    assert hip_lib.gsr_density_queries_per_wave() == 4
    assert hip_lib.gsr_density_queries_per_workgroup() % hip_lib.gsr_density_queries_per_wave() == 0
    buf = (ctypes.c_float * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    assert hip_lib.gsr_density_eval(0, 0, 16, *([null] * 3), 1.0, *([null] * 4)) == 0           # Q == 0: a no-op
    assert hip_lib.gsr_density_pack(0, *([null] * 6)) == 0
    for K in (0, 33, -1):
        assert hip_lib.gsr_density_eval(4, 8, K, p, p, p, 1.0, p, null, p, null) != 0 and b"K must be" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_density_eval(4, 0, 16, p, p, p, 1.0, p, null, p, null) != 0 and b"at least one" in hip_lib.gsr_last_error()
    for miss in (3, 4, 5, 7, 9):                                                                  # x, idx, records, density, err
        args = [4, 8, 16, p, p, p, 1.0, p, null, p, null]
        args[miss] = null
        assert hip_lib.gsr_density_eval(*args) != 0 and b"null" in hip_lib.gsr_last_error(), miss
    assert hip_lib.gsr_density_eval(-1, 8, 16, p, p, p, 1.0, p, null, p, null) != 0 and b"negative" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_density_pack(8, null, p, p, p, p, null) != 0 and b"null" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_density_pack(-1, p, p, p, p, p, null) != 0 and b"negative" in hip_lib.gsr_last_error()
    off = ctypes.c_void_p(p.value + 4)
    assert hip_lib.gsr_density_pack(8, off, p, p, p, p, null) != 0 and b"aligned" in hip_lib.gsr_last_error()


def test_closed_icosphere_loses_nothing():
    v, f = scene.icosphere(2)
    mask, kept = dr.peel(f, 5)
    assert mask.all() and kept == [len(f)] * 5
