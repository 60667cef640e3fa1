"""GPU: the kernels behind a capped grid and the shared fixed-order reduction (gsr_reduce.h) at the shapes of tests/
beyond_caps.py, where the grid-stride loops take a second and a third trip, tree_total's lanes add more than one partial,
md_big_kernel's waves take a second work item and hull_row_kernel has an interior segment -- against the restatements the
suite already compares them with at small shapes, and with the tolerances it derives there.  Nothing is excluded: what the
comparisons presuppose of the cases is asserted on the restatements alone by tests/test_beyond_caps.py."""
import functools

import numpy as np
import pytest
import torch

import beyond_caps as bc
import edit_ref
import eval_ref
import hull_ref
import splice_ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _bits(t):
    return t.cpu().numpy().tobytes() if torch.is_tensor(t) else np.ascontiguousarray(t).tobytes()


# ---------------------------------------------------------------------------------------------- image SSE
@pytest.mark.parametrize("name", list(bc.sse_shapes()))
def test_image_sse_past_one_partial_per_lane_and_past_one_trip(name):
    """|mse n - sse| <= n 2^-52 sse (a sum of n non-negative doubles in any order), n exact, two calls the same bits."""
    from gaustar_amd import evaluate as ev
    pred, gt = bc.sse_pair(name)
    tp, tg = _t(pred), _t(gt)
    launch = bc.reduce_launch(pred.size)
    for clamp in (False, True):
        im, again = ev.image_metrics(tp, tg, clamp=clamp), ev.image_metrics(tp, tg, clamp=clamp)
        sse, count = eval_ref.image_sse(pred, gt, clamp01=clamp)
        dev = abs(im.mse * count - sse) / sse
        print(f"[beyond_caps] sse {name} {pred.shape} clamp={clamp}: {launch.workgroups} workgroups, {launch.trips} trips, "
              f"relative deviation {dev:.3e} (bound {count * 2.0 ** -52:.3e})")
        assert im.n == count == pred.size
        assert abs(im.mse * count - sse) <= count * 2.0 ** -52 * sse
        assert abs(im.psnr - eval_ref.psnr(sse, count)) <= 1e-9
        assert (im.mse, im.n, im.psnr) == (again.mse, again.n, again.psnr)


def test_image_sse_masked_and_from_a_permuted_view():
    from gaustar_amd import evaluate as ev
    pred, gt = bc.sse_pair(bc.MASKED)
    mask = bc.sse_mask()
    tp, tg = _t(pred), _t(gt)
    for m in (_t(mask), _t(mask.astype(np.uint8))):
        im, again = ev.image_metrics(tp, tg, mask=m), ev.image_metrics(tp, tg, mask=m)
        sse, count = eval_ref.image_sse(pred, gt, mask=mask, clamp01=True)
        print(f"[beyond_caps] sse masked: n {im.n}, relative deviation {abs(im.mse * count - sse) / sse:.3e} (bound {count * 2.0 ** -52:.3e})")
        assert im.n == count == 3 * int(mask.sum()) and im.ssim is None
        assert abs(im.mse * count - sse) <= count * 2.0 ** -52 * sse
        assert (im.mse, im.n) == (again.mse, again.n)
    hp, hg = bc.sse_hwc()
    vp, vg = _t(hp).permute(2, 0, 1), _t(hg).permute(2, 0, 1)
    assert not vp.is_contiguous() and vp.stride(2) == 3 and tuple(vp.shape) == pred.shape
    for clamp in (False, True):
        a, b = ev.image_metrics(tp, tg, clamp=clamp), ev.image_metrics(vp, vg, clamp=clamp)
        assert a.mse == b.mse and a.n == b.n == pred.size           # other index arithmetic, the same summation order
    a, b = ev.image_metrics(tp, tg, mask=_t(mask)), ev.image_metrics(vp, vg, mask=_t(mask))
    assert a.mse == b.mse and a.n == b.n


# ---------------------------------------------------------------------------------------------- distance statistics
@pytest.mark.parametrize("n", bc.stats_sizes())
def test_distance_stats_past_one_partial_per_lane_and_past_one_trip(n):
    from gaustar_amd import evaluate as ev
    verts, faces, other = bc.stats_meshes()
    taus = bc.STATS_THRESHOLDS
    md, ab, ba = ev.mesh_distance((_t(verts), _t(faces)), (_t(other), _t(faces)), n_samples=n, thresholds=taus, seed=bc.STATS_SEED,
                                  return_samples=True)
    assert md.n_samples == n and tuple(ab.dist.shape) == tuple(ba.dist.shape) == (n,)
    launch = bc.reduce_launch(n)
    for what, got, hit in (("a_to_b", md.a_to_b, ab), ("b_to_a", md.b_to_a, ba)):
        d = hit.dist.cpu().numpy()
        s, s2, mx, counts = eval_ref.distance_stats(d, taus)
        print(f"[beyond_caps] stats n={n} {what}: {launch.workgroups} workgroups, {launch.trips} trips, mean deviation "
              f"{abs(got.mean - s / n) / (s / n):.3e}, mean_sq {abs(got.mean_sq - s2 / n) / (s2 / n):.3e} (bound {n * 2.0 ** -52:.3e})")
        assert abs(got.mean - s / n) <= n * 2.0 ** -52 * (s / n)
        assert abs(got.mean_sq - s2 / n) <= n * 2.0 ** -52 * (s2 / n)
        assert got.max == mx and list(got.counts) == counts
        assert 0 < counts[0] < counts[1] < counts[2] <= n
    assert md.chamfer == md.a_to_b.mean + md.b_to_a.mean


# ---------------------------------------------------------------------------------------------- the plain mean
@pytest.mark.parametrize("n", bc.mean_sizes())
def test_mean_past_one_partial_per_lane_and_past_two_trips(n):
    from gaustar_amd import regions
    x = bc.mean_vector(n)
    tx = _t(x)
    a, b = regions._mean_f64(tx), regions._mean_f64(tx)
    assert _bits(a) == _bits(b)
    want = splice_ref.exact_mean(x)
    dev = abs(float(a.cpu()) - want) / want
    launch = bc.reduce_launch(n)
    print(f"[beyond_caps] mean of {n}: {launch.workgroups} workgroups, {launch.trips} trips, last trip {launch.last_trip}, "
          f"relative deviation {dev:.3e} (bound {n * 2.0 ** -53:.3e})")
    assert dev <= n * 2.0 ** -53


# ---------------------------------------------------------------------------------------------- the rigid fit's sums
@functools.lru_cache(maxsize=None)
def _fit_reference(K):
    """Per frame: edit_ref.fit_centroids (exactly rounded sums and their bounds), computed once."""
    src, dst, _, _ = bc.fit_anchors(K)
    return [edit_ref.fit_centroids(src, dst[t]) for t in range(bc.FIT_FRAMES)]


@pytest.mark.parametrize("K", bc.fit_sizes())
def test_fit_sums_past_one_partial_per_lane_and_past_one_trip(K):
    """What tests/test_gpu_edit.py's test_fit_sums asserts, at K = 66 000 and 524 801.  The sums' bounds at the larger K are
    some 5e-11 on a centroid and 3e-5 on the entries of H, which are about 5e5: 1e-9 on the rotation and the translation holds."""
    from gaustar_amd import edit
    src, dst, Rs, ts = bc.fit_anchors(K)
    T = bc.FIT_FRAMES
    sums = edit.fit_sums(src, dst)
    assert sums.is_cuda and tuple(sums.shape) == (T, 16) and sums.dtype == torch.float64
    again = edit.fit_sums(_t(src), _t(dst))
    assert _bits(sums) == _bits(again)
    got = sums.cpu().numpy()
    launch = bc.reduce_launch(K)
    for t in range(T):
        n, abar, bbar, tol_a, tol_b = _fit_reference(K)[t]
        assert got[t, 0] == n == K - 2
        err_a, err_b = np.abs(got[t, 1:4] - abar), np.abs(got[t, 4:7] - bbar)
        H, tol_h = edit_ref.fit_cross(src, dst[t], got[t, 1:4], got[t, 4:7])
        err_h = np.abs(got[t, 7:].reshape(3, 3) - H)
        print(f"[beyond_caps] fit K={K} t={t}: {launch.workgroups} workgroups, {launch.trips} trips, n={n}, centroid err/tol "
              f"{np.max(err_a / tol_a):.3f} {np.max(err_b / tol_b):.3f}, H err/tol {np.max(err_h / tol_h):.3f} "
              f"(tol {tol_a.max():.1e}, {tol_h.max():.1e})")
        assert (err_a <= tol_a).all() and (err_b <= tol_b).all() and (err_h <= tol_h).all()
    fit = edit.fit_rigid(src, dst)
    R, tr, n, ok, _ = edit_ref.rigid_from_sums(got)
    assert _bits(fit.R) == _bits(R) and _bits(fit.t) == _bits(tr) and np.array_equal(fit.n, n) and np.array_equal(fit.ok, ok) and ok.all()
    for i in range(T):
        print(f"[beyond_caps] fit K={K} t={i}: |R - planted| {np.abs(fit.R[i] - Rs[i]).max():.2e}, |t - planted| {np.abs(fit.t[i] - ts[i]).max():.2e}")
        assert np.abs(fit.R[i] - Rs[i]).max() < 1e-9 and np.abs(fit.t[i] - ts[i]).max() < 1e-9


# ---------------------------------------------------------------------------------------------- rectify
@pytest.mark.parametrize("which", ["dword", "byte"])
def test_rectify_past_the_grid_cap(which):
    """Byte for byte the restatement, from an aligned dst (whole dwords, quads of pixels) and from one a byte off alignment
    (byte stores, single pixels): each of the two runs the path whose second trip the case is there for, and the other one at
    fewer trips."""
    from gaustar_amd import dataprep
    case = bc.rectify_case(which)
    h, w, c = case.h, case.w, case.c
    src, want = bc.rectify_source(which), bc.rectify_want(which)
    aligned_src = _t(src)
    aligned_out = torch.full((h, w, c), 0xAA, dtype=torch.uint8, device=DEV)
    assert aligned_src.data_ptr() % 16 == 0 and aligned_out.data_ptr() % 16 == 0
    a = dataprep.rectify_image(aligned_src, case.intr, case.dist, case.border, out=aligned_out)
    assert a.data_ptr() == aligned_out.data_ptr()
    n = h * w * c
    pool_src = torch.zeros(n + 1, dtype=torch.uint8, device=DEV)
    pool_out = torch.full((n + 17,), 0xAA, dtype=torch.uint8, device=DEV)
    off_src, off_out = pool_src[1:].view(h, w, c), pool_out[1:n + 1].view(h, w, c)
    off_src.copy_(aligned_src)
    assert off_src.data_ptr() % 16 == 1 and off_out.data_ptr() % 16 == 1
    b = dataprep.rectify_image(off_src, case.intr, case.dist, case.border, out=off_out)
    assert b.data_ptr() == off_out.data_ptr()
    assert int(pool_out[0]) == 0xAA and bool((pool_out[n + 1:] == 0xAA).all())          # nothing before, nothing past the end
    ga, gb = a.cpu().numpy(), b.cpu().numpy()
    print(f"[beyond_caps] rectify {which} {h}x{w}x{c}: launch {bc.rectify_launch(case)}, {int((ga != want).sum())} bytes of the aligned "
          f"run differ, {int((gb != want).sum())} of the unaligned run")
    assert np.array_equal(ga, want) and np.array_equal(gb, want) and torch.equal(a, b)


# ---------------------------------------------------------------------------------------------- mesh depth
def _render(case, **kw):
    from gaustar_amd import mesh_depth
    cam = case.cam
    extr = np.eye(4)
    extr[:3, :3], extr[:3, 3] = cam[:9].reshape(3, 3), cam[9:12]
    intr = np.array([[cam[12], 0, cam[14]], [0, cam[13], cam[15]], [0, 0, 1.0]])
    view = mesh_depth.mesh_depth_view(case.verts, case.faces, extr, intr, case.H, case.W, principal_point=(cam[14], cam[15]),
                                      return_faces=True, **kw)
    return view.depth.cpu().numpy(), view.mask.cpu().numpy(), view.face.cpu().numpy(), int(view.n_clipped.cpu())


def _same_render(got, want, what):
    wrong = int((got[2] != want[2]).sum())
    print(f"[beyond_caps] mesh depth {what}: {wrong} pixels show another face, n_clipped {got[3]}")
    assert got[0].dtype == np.float32 and got[0].shape == want[0].shape
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[1], want[1]) and got[3] == want[3]
    assert got[0].view(np.uint32).tobytes() == want[0].view(np.uint32).tobytes()


@pytest.mark.parametrize("small_max", [1, None], ids=["every_face_listed", "default"])
def test_mesh_depth_wall_with_more_mid_faces_than_waves(small_max):
    wall = bc.depth_wall()
    kw = {} if small_max is None else {"small_max": small_max}
    items = bc.big_items(wall, 1 if small_max is not None else bc.caps()["MD_SMALL_MAX"])
    _same_render(_render(wall, **kw), bc.depth_want("wall"), f"wall small_max={small_max}: (mid, huge, items) = {items} on {bc.big_waves()} waves")


@pytest.mark.parametrize("small_max", [None, 10 ** 9], ids=["default", "no_face_listed"])
def test_mesh_depth_fan_with_more_slices_than_waves(small_max):
    fan, _cols = bc.depth_fan()
    kw = {} if small_max is None else {"small_max": small_max}
    items = bc.big_items(fan, bc.caps()["MD_SMALL_MAX"] if small_max is None else small_max)
    _same_render(_render(fan, **kw), bc.depth_want("fan"), f"fan small_max={small_max}: (mid, huge, items) = {items} on {bc.big_waves()} waves")


# ---------------------------------------------------------------------------------------------- hull distance
@pytest.mark.parametrize("radius", bc.HULL_RADII)
def test_hull_distance_with_an_interior_segment(radius):
    """Three segments a row, runs across both boundaries, a row whose halos hold nothing, distances beyond the cap; from
    contiguous input and from a column-strided view.  (In this mask a pixel near a boundary is at most three rows from a run or
    from the quiet row, so the column pass decides most of what is compared there: what the halos hold is the next test's.)"""
    from gaustar_amd import hull
    m = bc.hull_mask()
    want = hull_ref.mask_distance(m, 128, radius)
    got = hull.mask_distance(np.array(m), 128, radius)
    assert got.dtype == torch.int16 and tuple(got.shape) == m.shape
    wide = _t(np.repeat(m, 2, axis=1))
    view = wide[:, ::2]
    assert not view.is_contiguous()
    strided = hull.mask_distance(view, 128, radius)
    print(f"[beyond_caps] hull {m.shape} R={radius}: {int((got.cpu().numpy() != want).sum())} pixels differ, "
          f"{int((strided.cpu().numpy() != want).sum())} from the strided view")
    assert np.array_equal(got.cpu().numpy(), want) and np.array_equal(strided.cpu().numpy(), want)


@pytest.mark.parametrize("name", list(bc.hull_halo_masks()))
def test_hull_distance_reads_both_words_of_both_halos(name):
    """Masks of three rows alike, whose distances near the segment boundaries are decided by pixels of the neighbouring segment
    (tests/test_beyond_caps.py shows that a halo of 0 or of 64 columns gets them wrong)."""
    from gaustar_amd import hull
    m = bc.hull_halo_masks()[name]
    want = hull_ref.mask_distance(m, 128, 127)
    got = hull.mask_distance(np.array(m), 128, 127).cpu().numpy()
    print(f"[beyond_caps] hull halo {name} {m.shape}: {int((got != want).sum())} pixels differ")
    assert np.array_equal(got, want)
