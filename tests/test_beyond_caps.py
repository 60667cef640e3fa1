"""CPU: the cases of tests/beyond_caps.py cross the caps they are there for -- so that a moved cap fails HERE instead of silently
losing the coverage -- and the conditions the GPU tests rely on hold for the restatements alone, so that tests/
test_gpu_beyond_caps.py excludes nothing."""
import numpy as np

import beyond_caps as bc
import hull_ref


def test_caps_are_the_ones_the_shapes_were_derived_for():
    c = bc.caps()
    msg = "tests/beyond_caps.py derives its shapes from this cap: they move with it -- look at what they became"
    assert (c["RED_BLOCK"], c["RED_MAX_WGS"]) == (256, 2048), msg
    assert (c["PREP_BLOCK"], c["PREP_MAX_BLOCKS"]) == (256, 4096), msg
    assert (c["MD_BLOCK"], c["MD_BIG_BLOCKS"], c["MD_SLICES"], c["MD_MID_MAX"]) == (256, 2048, 64, 4096), msg
    assert (c["HD_LANE_PX"], c["HD_HALO"]) == (16, 128), msg
    assert c["PR_G"] == 4, msg
    assert bc.one_partial_per_lane() == 65536 and bc.one_trip() == 524288 and bc.rectify_trip() == 1048576
    assert bc.big_waves() == 8192 and bc.hull_segment() == 1024


def test_reduction_cases_cross_their_caps():
    c = bc.caps()
    block, cap = c["RED_BLOCK"], c["RED_MAX_WGS"]
    shapes = bc.sse_shapes()
    assert list(shapes.values()) == [(3, 150, 150), (3, 419, 418), (1, 1025, 1024)]
    n = {k: int(np.prod(s)) for k, s in shapes.items()}
    a, b, d = (bc.reduce_launch(n[k]) for k in ("partials", "one_trip", "two_trips"))
    assert (a.workgroups, a.trips, a.partials_per_lane) == (264, 1, 2) and block < a.workgroups < cap
    assert (b.workgroups, b.trips, b.last_trip) == (cap, 2, 1138) and b.last_trip % block != 0
    assert (d.workgroups, d.trips, d.last_trip) == (cap, 3, 1024)
    assert b.partials_per_lane == d.partials_per_lane == cap // block
    pred, gt = bc.sse_pair(bc.MASKED)
    assert pred.dtype == gt.dtype == np.float32 and pred.min() < 0 and pred.max() > 1 and 0 <= gt.min() and gt.max() <= 1
    m = bc.sse_mask()
    assert m.shape == shapes[bc.MASKED][1:] and m[:, 0].all() and not m[:, 1].any() and 0 < m.sum() < m.size
    hp, hg = bc.sse_hwc()
    assert hp.shape == shapes[bc.MASKED][1:] + (3,) and np.array_equal(hp.transpose(2, 0, 1), pred) and np.array_equal(hg.transpose(2, 0, 1), gt)
    # plain vectors
    assert bc.mean_sizes() == (65537, 524289, 1100003)
    l0, l1, l2 = (bc.reduce_launch(k) for k in bc.mean_sizes())
    assert (l0.workgroups, l0.partials_per_lane) == (block + 1, 2) and l0.trips == 1
    assert (l1.workgroups, l1.trips, l1.last_trip) == (cap, 2, 1)
    assert (l2.workgroups, l2.trips) == (cap, 3) and l2.last_trip % block != 0
    assert all((bc.mean_vector(k) > 0).all() and len(bc.mean_vector(k)) == k for k in bc.mean_sizes())
    # distance statistics
    assert bc.stats_sizes() == (70001, 600001)
    s0, s1 = (bc.reduce_launch(k) for k in bc.stats_sizes())
    assert block < s0.workgroups < cap and s0.partials_per_lane == 2 and (s1.workgroups, s1.trips) == (cap, 2)
    assert len(bc.stats_meshes()[1]) == 320
    # rigid fit
    assert bc.fit_sizes() == (66000, 524801)
    f0, f1 = (bc.reduce_launch(k) for k in bc.fit_sizes())
    assert block < f0.workgroups < cap and f0.partials_per_lane == 2
    assert (f1.workgroups, f1.trips, f1.last_trip) == (cap, 2, 2 * block + 1)
    for K in bc.fit_sizes():
        src, dst, Rs, ts = bc.fit_anchors(K)
        assert dst.shape == (bc.FIT_FRAMES, K, 3) and np.isnan(dst[-1, K // 2]).all() and np.isnan(dst[0, K - 1, 1]) and np.isnan(src[1, 2])
        assert int(np.isnan(src).sum()) == 1 and int(np.isnan(dst).sum()) == 4
    # the regularisers' groups of PR_G Gaussians
    sizes = bc.param_reg_sizes()
    assert sizes == ((100_003, 60_001), (491_520, 300_001), (2_097_157, 1_300_003))
    p0, p1, p2 = (bc.param_reg_launch(N) for N, _ in sizes)
    assert p0.workgroups == 98 and p1.workgroups == 480 and p1.partials_per_lane == 2
    assert (p2.workgroups, p2.trips, p2.last_trip) == (cap, 2, 2) and sizes[2][0] % c["PR_G"] == 1     # the last group holds one
    assert all(M < N and M % c["PR_G"] != 0 for N, M in sizes)


def test_planted_rigid_motions_are_recovered_from_exact_sums():
    """What the GPU test asks of fit_rigid (rotation and translation within 1e-9 of the planted ones) holds for the planted data
    with exactly rounded sums: the anchors are an exact rigid motion up to one rounding per coordinate."""
    import edit_ref
    K = bc.fit_sizes()[0]
    src, dst, Rs, ts = bc.fit_anchors(K)
    R, t, n, ok, _ = edit_ref.fit_rigid(src, dst)
    assert ok.all() and n.tolist() == [K - 2, K - 2]
    for i in range(bc.FIT_FRAMES):
        print(f"K={K} frame {i}: |R - planted| {np.abs(R[i] - Rs[i]).max():.2e}, |t - planted| {np.abs(t[i] - ts[i]).max():.2e}")
        assert np.abs(R[i] - Rs[i]).max() < 1e-12 and np.abs(t[i] - ts[i]).max() < 1e-12


def test_rectify_cases_cross_the_grid_cap_and_show_border_and_image():
    c = bc.caps()
    dword, byte = bc.rectify_case("dword"), bc.rectify_case("byte")
    assert (dword.h, dword.w, dword.c) == (2049, 2048, 1) and (byte.h, byte.w, byte.c) == (1025, 1024, 3)
    assert dword.dist is not None and any(dword.dist) and byte.dist is None and byte.unaligned and not dword.unaligned
    assert bc.rectify_launch(dword) == (c["PREP_MAX_BLOCKS"], 2, dword.w // 4)      # 1 049 088 quads: one row into the second trip
    assert bc.rectify_launch(byte) == (c["PREP_MAX_BLOCKS"], 2, byte.w)
    assert dword.cam4[2] != dword.w / 2 and dword.cam4[2] % 1 != 0                 # the fractional shift
    for which, case in (("dword", dword), ("byte", byte)):
        want = bc.rectify_want(which)
        border = (want == np.asarray(case.border, np.uint8)).all(-1)
        second = border[-1]                                                        # the last row is the second trip
        print(f"rectify {which}: {border.mean():.3f} of the pixels are border, {second.mean():.3f} of the second trip's")
        assert border.any() and not border.all() and border.mean() < 0.9 and border[0, 0] and border[0, -1]
        assert not second.all() and (~second).sum() > case.w // 2
        src = bc.rectify_source(which)
        assert src.shape == (case.h, case.w, case.c) and len(np.unique(src)) == 256


def test_depth_wall_lists_more_mid_faces_than_the_grid_has_waves():
    c = bc.caps()
    wall = bc.depth_wall()
    assert len(wall.faces) >= 8200 and len(wall.faces) == 2 * wall_cells_product()
    n = bc.pixel_ranges(wall)
    assert n.min() >= 2 and n.max() <= c["MD_MID_MAX"], (n.min(), n.max())
    n_mid, n_huge, items = bc.big_items(wall, small_max=1)
    assert n_mid == len(wall.faces) > bc.big_waves() and n_huge == 0 and items - bc.big_waves() == len(wall.faces) - bc.big_waves()
    assert bc.big_items(wall, small_max=c["MD_SMALL_MAX"]) == (0, 0, 0)           # at the default every face is walked in place
    depth, mask, face, n_clipped = bc.depth_want("wall")
    assert n_clipped == 0 and np.array_equal(np.unique(face[face >= 0]), np.arange(len(wall.faces)))
    assert (mask == 0).any() and len(np.unique(depth[mask > 0])) > 1000


def wall_cells_product():
    rows, cols = bc.wall_cells()
    return rows * cols


def test_depth_fan_has_more_slices_than_the_grid_has_waves():
    c = bc.caps()
    fan, cols = bc.depth_fan()
    assert len(fan.faces) == bc.fan_faces() == 140 and len(set(cols.tolist())) == len(cols) and (np.diff(cols) < 0).any()
    n = bc.pixel_ranges(fan)
    assert (n == fan.H * fan.W).all() and fan.H * fan.W > c["MD_MID_MAX"] and fan.H >= c["MD_SLICES"]
    n_mid, n_huge, items = bc.big_items(fan, small_max=c["MD_SMALL_MAX"])
    assert (n_mid, n_huge) == (0, 140) and items == 140 * c["MD_SLICES"] and items - bc.big_waves() == bc.FAN_EXTRA * c["MD_SLICES"]
    assert bc.big_items(fan, small_max=10 ** 9) == (0, 0, 0)
    depth, mask, face, n_clipped = bc.depth_want("fan")
    assert n_clipped == 0 and (mask == 255).all()
    assert np.array_equal(np.unique(face), np.arange(140))
    assert (face[:, cols] == np.arange(140)).all()                               # each face is the nearest at its own column


def test_hull_mask_shows_the_runs_the_cap_and_the_quiet_row():
    c = bc.caps()
    m = bc.hull_mask()
    seg, halo = bc.hull_segment(), c["HD_HALO"]
    assert m.shape == (5, 2200) and bc.hull_width() > 2 * seg + halo and c["HD_MAX_R"] == max(bc.HULL_RADII) == halo - 1
    assert -(-m.shape[1] // seg) == 3                                            # segments per row: one of them interior
    inside = m >= 128
    run = np.zeros(m.shape[1], bool)
    run[bc.HULL_RUN[0]:bc.HULL_RUN[1]] = True
    assert inside[2, run].all() and bc.HULL_RUN[1] - bc.HULL_RUN[0] == 400
    for b in bc.hull_boundaries():
        assert not inside[bc.HULL_QUIET_ROW, b - halo:b + halo].any()
        for r in set(range(bc.HULL_ROWS)) - {bc.HULL_QUIET_ROW}:
            assert inside[r, b - 9:b + 6].all() and not inside[r, b + 6] and inside[r, b - 1] and inside[r, b]
    sparse = inside.copy()
    sparse[2, run] = False
    for b in bc.hull_boundaries():
        sparse[:, b - 9:b + 6] = False
    assert 20 < sparse.sum() < 150 and sparse[:, :seg].any() and sparse[:, seg:2 * seg].any()
    assert sparse[:, seg - halo:seg].any() and sparse[:, seg:seg + halo].any() and sparse[:, 2 * seg - halo:2 * seg].any()   # in the halos
    for R in bc.HULL_RADII:
        d2 = hull_ref.mask_distance(m, 128, R).astype(np.int64)
        assert (np.abs(d2) <= R * R).all() and (d2 != 0).all()
        for b in bc.hull_boundaries():
            for side in (d2[:, max(b - seg, 0):b], d2[:, b:min(b + seg, m.shape[1])]):
                assert (side == -R * R).any() and (side > 0).any()                 # the cap and the run, on either side
                if R > 1:
                    assert ((side > 0) & (side < R * R)).any() and ((side < 0) & (side > -R * R)).any()
                else:
                    assert (side == R * R).any()
        if R == 127:
            assert (d2[2, 200:400] > 0).all() and (d2[2, 200:400] <= 4).all() and (d2[bc.HULL_QUIET_ROW, seg - 2:seg + 2] == -1).all()
            for lo, hi in bc.hull_empty_zones():
                assert (d2[:, lo:hi] == -R * R).any()


def test_hull_halo_masks_depend_on_both_words_of_both_halos():
    """Restated with a halo of 0 columns (near_*) or of 64 (far_*), the distance of these masks is wrong on the side of each
    boundary the case is there for: a kernel that dropped or misplaced a halo word would not pass them."""
    R, halo = 127, bc.caps()["HD_HALO"]
    masks = bc.hull_halo_masks()
    assert len(masks) == 8
    for name, m in masks.items():
        want = hull_ref.mask_distance(m, 128, R)
        assert m.shape == (3, bc.hull_width()) and (m[0] == m[1]).all() and (m[0] == m[2]).all()
        assert np.array_equal(bc.hull_with_halo_of(m, R, halo), want)            # the whole halo: the restatement itself
        case = name.replace("_inverted", "")
        seen = 0 if case.startswith("near") else 64
        wrong = bc.hull_with_halo_of(m, R, seen) != want
        for b, (a, c) in zip(bc.hull_boundaries(), bc.HULL_HALO_CASES[case]):
            left, right = int(wrong[:, b - halo:b].sum()), int(wrong[:, b:b + halo].sum())
            reach = min(abs(a - c) // 2, R - min(a, c)) - 1                      # pixels per row that look across the boundary
            print(f"hull {name} at {b}: with a halo of {seen} columns {left} pixels are wrong before it, {right} after it")
            assert (left, right) == ((3 * reach, 0) if a > c else (0, 3 * (reach + 1))), (name, b, reach)
            sign = 1 if name.endswith("_inverted") else -1
            assert (want[:, b - 1] == sign * min(a - 1, c + 1) ** 2).all() and (want[:, b] == sign * min(a, c) ** 2).all()
