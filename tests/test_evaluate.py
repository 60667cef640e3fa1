"""tests/eval_ref.py, the numpy restatement of gaustar_amd.evaluate, pinned on cases whose answers are known by hand, and the
host side of the module (no GPU): what tests/test_gpu_evaluate.py compares the device with is right in itself."""
import numpy as np
import pytest

import eval_ref as ref
from gaustar_amd import evaluate


def _d2(points, verts, faces):
    dist, face, bary, closest = ref.surface_distance(points, verts, faces)
    return dist * dist, face, bary, closest


# ---------------------------------------------------------------------------------------------------- 1 closest point
def test_one_triangle_every_region():
    """(0,0,0), (4,0,0), (0,4,0): a query per region and three on the face itself.  Every denominator is a power of two, so
    x (1 / y) is x / y and the squared distances are exact integers."""
    faces = np.array([[0, 1, 2]])
    for p, want_d2, want_bary in ref.HAND_CASES:
        d2, v, w, q = ref.closest_pairs(np.array(p, float), *ref.TRIANGLE)
        assert d2 == want_d2, (p, d2)
        dist, face, bary, closest = ref.surface_distance([p], ref.TRIANGLE, faces)
        assert face[0] == 0 and dist[0] == np.sqrt(want_d2)
        assert tuple(bary[0]) == want_bary, (p, bary[0])
        assert np.array_equal(closest[0], np.array(want_bary) @ ref.TRIANGLE)
        assert np.array_equal(closest[0], q)


def test_mirror_tie_takes_the_lower_index():
    verts, faces, p = ref.MIRROR
    for f in (faces, faces[::-1]):
        d2, face, _b, _q = _d2(p, verts, f)
        both = ref.closest_pairs(p[0], verts[f[:, 0]], verts[f[:, 1]], verts[f[:, 2]])[0]
        assert tuple(both) == (5.0, 5.0)
        assert face[0] == 0 and ref.surface_distance(p, verts, f)[0][0] == np.sqrt(5.0)


def test_degenerate_faces_are_segments_and_points():
    line = np.array([[0, 0, 0], [1, 0, 0], [2, 0, 0]], float)
    d2, v, w, q = ref.closest_pairs(np.array([.5, 1, 0]), *line)
    assert d2 == 1.0 and tuple(q) == (.5, 0, 0)
    point = np.array([[1, 2, 3]] * 3, float)
    d2, v, w, q = ref.closest_pairs(np.array([1., 2, 5]), *point)
    assert d2 == 4.0 and tuple(q) == (1, 2, 3)
    dist, face, bary, _ = ref.surface_distance([[1., 2, 5]], point, [[0, 1, 2]])
    assert dist[0] == 2.0 and face[0] == 0 and bary[0].sum() == 1.0


def test_nan_ranks_nothing():
    dist, face, bary, closest = ref.surface_distance([[np.nan, 0, 0], [0, 0, 1]], ref.TRIANGLE, [[0, 1, 2]])
    assert face[0] == -1 and dist[0] == np.inf and np.isnan(bary[0]).all() and np.isnan(closest[0]).all()
    assert face[1] == 0 and dist[1] == 1.0


def test_exact_distance_against_a_barycentric_lattice():
    """40 random triangles, 200 random queries: the minimum over the lattice of barycentrics i / n, j / n (n = 60) can only be
    at or above the exact distance, and by no more than the lattice's spacing, (longest edge) / n: the closest point lies in a
    lattice cell, whose corners are within that of it."""
    rng = np.random.default_rng(7)
    n = 60
    tri = rng.uniform(-1, 1, size=(40, 3, 3))
    pts = rng.uniform(-1.5, 1.5, size=(200, 3))
    verts, faces = tri.reshape(-1, 3), np.arange(120).reshape(40, 3)
    exact = ref.surface_distance(pts, verts, faces)[0]
    i, j = np.meshgrid(np.arange(n + 1), np.arange(n + 1), indexing="ij")
    keep = i + j <= n
    b = np.stack([(n - i - j)[keep], i[keep], j[keep]], -1) / n                # [L,3]
    lattice = np.einsum("lk,fkc->flc", b, tri)                                # [40,L,3]
    grid = np.sqrt(((pts[:, None, None, :] - lattice[None]) ** 2).sum(-1)).min(axis=(1, 2))
    edges = np.linalg.norm(tri - np.roll(tri, 1, axis=1), axis=-1).max()
    excess = grid - exact
    print("largest excess", excess.max(), "bound", edges / n)
    assert (excess >= -1e-12).all() and (excess <= edges / n).all()


def test_bary_and_closest_agree():
    """u + v + w is 1 to rounding, all >= 0, and bary_to_point of them is the closest point to rounding."""
    verts, faces = ref.triangle_soup(50, seed=3)
    pts = np.random.default_rng(4).uniform(-1.5, 1.5, size=(300, 3))
    dist, face, bary, closest = ref.surface_distance(pts, verts, faces)
    assert (bary >= 0).all() and np.abs(bary.sum(-1) - 1).max() < 1e-15
    again = ref.bary_to_point(verts[faces[face]], bary)
    assert np.abs(again - closest).max() < 1e-14
    assert np.allclose(np.linalg.norm(pts - closest, axis=-1), dist, rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------------- 2 sampler
TWO = (np.array([[0, 0, 0], [1, 0, 0], [0, 2, 0], [3, 0, 0], [0, 2, 0], [0, 0, 0], [5, 5, 5], [5, 5, 5], [5, 5, 5]], float),
       np.array([[0, 1, 2], [6, 7, 8], [3, 4, 5]]))      # areas 1, 0, 3


@pytest.mark.parametrize("n", (1, 2, 7, 1000))
def test_sampler_gives_each_face_its_share(n):
    verts, faces = TWO
    assert tuple(ref.face_areas(verts, faces)) == (1.0, 0.0, 3.0)
    ids, bary, points = ref.sample_surface(verts, faces, n, seed=0)
    assert ids.dtype == np.int32 and (np.diff(ids) >= 0).all()
    assert (ids != 1).all()                                                   # no area, no sample
    assert int((ids == 0).sum()) in (n // 4, -(-n // 4))
    assert (bary >= 0).all() and (bary.sum(-1) == 1.0).all()
    ids2, bary2, points2 = ref.sample_surface(verts, faces, n, seed=1)
    assert np.array_equal(ids, ids2) and not np.array_equal(points, points2)
    # a sample lies on its face: bary_to_point of weights that are >= 0 and sum to 1
    assert np.array_equal(points, ref.bary_to_point(verts[faces[ids]], bary))


def test_sampler_weights_and_errors():
    w = ref.sample_weights(np.array([3.0, 1.5, 0.0, 1e-300]))
    assert w.dtype == np.int64 and tuple(w) == (3 << 30, 3 << 29, 0, 0) and 2 ** 31 <= w.max() < 2 ** 32
    for bad in ([0.0, 0.0], [np.inf, 1.0], [np.nan], []):
        with pytest.raises(ValueError):
            ref.sample_weights(np.array(bad))
    # splitmix64: the first output for seed 0 is a published value
    assert int(ref.mix64(ref.GOLDEN)[0]) == 0xE220A8397B1DCDAF


# ---------------------------------------------------------------------------------------------------- 3 statistics, images
def test_stats_and_sse_restatements():
    s, s2, mx, counts = ref.distance_stats([0.25, 0.5, 1.0], [0.25, 0.5, 2.0])
    assert (s, s2, mx, counts) == (1.75, 1.3125, 1.0, [0, 1, 3])
    gt = np.zeros((3, 2, 2), np.float32)
    sse, n = ref.image_sse(gt + 0.5, gt)
    assert (sse, n) == (3.0, 12) and ref.psnr(sse, n) == 20 * np.log10(2.0)
    assert ref.psnr(0.0, 12) == np.inf
    sse, n = ref.image_sse(gt + 2.0, gt, clamp01=True)
    assert (sse, n) == (12.0, 12)
    sse, n = ref.image_sse(gt - 1.0, gt, mask=np.array([[1, 0], [0, 0]]), clamp01=False)
    assert (sse, n) == (3.0, 3)


# ---------------------------------------------------------------------------------------------------- 4 the module's host side
def test_module_surface():
    for name in ("surface_distance", "sample_surface", "mesh_distance", "image_metrics", "evaluate_views", "score_frame"):
        assert callable(getattr(evaluate, name)) and name in evaluate.__all__
    assert evaluate.SurfaceHit._fields == ("dist", "face", "bary", "closest")
    assert evaluate.SurfaceSamples._fields == ("face_ids", "bary", "points")
    assert evaluate.ImageMetrics._fields == ("psnr", "ssim", "mse", "n")
    assert evaluate.ViewMetrics._fields == ("psnr", "ssim", "mean_psnr", "mean_ssim")
    assert evaluate._psnr(0.25) == 20 * np.log10(2.0) and evaluate._psnr(0.0) == float("inf")
    import gaustar_amd
    assert "`evaluate`" in gaustar_amd.__doc__
    import inspect
    from gaustar_amd import tracking
    assert inspect.signature(tracking.bind_points).parameters["exact"].default is False


def test_library_exports_the_entries(hip_lib):
    from gaustar_amd import build
    assert "gsr_eval.hip" in build.SOURCES
    assert hip_lib.gsr_eval_queries() == 16 and hip_lib.gsr_eval_tile() == 512 and hip_lib.gsr_eval_max_thresholds() == 8
    assert hip_lib.gsr_eval_workspace_bytes() >= 4 * 8 * 2048
    null = None
    assert hip_lib.gsr_eval_closest(4, null, null, 4, 0, *([null] * 7), null) != 0 and b"no faces" in hip_lib.gsr_last_error()
    assert hip_lib.gsr_eval_closest(0, null, null, 0, 0, *([null] * 7), null) == 0
    assert hip_lib.gsr_eval_distance_stats(4, null, 9, *([null] * 3), null) != 0
    assert hip_lib.gsr_eval_image_sse(0, 4, 4, null, 0, 0, 0, null, 0, 0, 0, null, 0, null, null, null) != 0
    assert hip_lib.gsr_eval_sample(4, 0, 0, *([null] * 3), 0, *([null] * 4), null) != 0 and b"no faces" in hip_lib.gsr_last_error()
