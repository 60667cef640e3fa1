"""The scenes of test_gpu_plan_lifecycle.py (plan_scenes.py) do what the GPU tests lean on -- shown here on the CPU oracle's
tile ranges, so that a failure on the GPU is the library's and not the scene's."""
import numpy as np

import plan_scenes as S

PART_FROM = 1024        # gsr_internal.h: the exact path may blend longer lists in parts, and bit equality with a planned view ends
PLAN_MAX_LIST = 2048    # gsr_internal.h: a planned list is sorted inside the forward blend


def _block(counts):
    """-> (first row, last row, first column, last column) of the tiles that hold anything."""
    ys, xs = np.nonzero(counts)
    return int(ys.min()), int(ys.max()), int(xs.min()), int(xs.max())


def test_corner_clusters_land_on_small_blocks_with_empty_tiles_between_them():
    """Case 3: each corner's instances fall into at most 3 x 3 tiles, and any two corners' blocks are at least three tiles apart in
    rows or in columns -- so a tile of one block, and each of its eight neighbours, is empty in every other corner's view: capacity 0
    in that view's plan at any slack level (gsr_plan.h plan_capacity), and the next corner's view must outgrow it.  (The library's
    lists are the oracle's or shorter, plan_scenes.tile_lists: empty tiles stay empty, short lists stay short.)"""
    cam = S.camera()
    assert (cam.W, cam.H) == (128, 128)
    blocks = []
    for visit in range(len(S.CORNERS)):
        counts, R = S.tile_lists(S.corner_cluster(visit), cam)
        r0, r1, c0, c1 = _block(counts)
        assert r1 - r0 <= 2 and c1 - c0 <= 2, (visit, r0, r1, c0, c1)
        assert 500 <= counts.max() <= S.CORNER_P < PART_FROM and 1000 <= R <= 1300, (visit, int(counts.max()), R)
        # (the longest list doubled -- slack level 3 -- stays a plannable, unsplit list: the plan each view leaves is VALID)
        assert 2 * int(counts.max()) + 63 < 1792
        blocks.append((r0, r1, c0, c1))
    for i, a in enumerate(blocks):
        for b in blocks[i + 1:]:
            rows_apart = max(a[0] - b[1], b[0] - a[1])
            cols_apart = max(a[2] - b[3], b[2] - a[3])
            assert max(rows_apart, cols_apart) >= 3, (a, b)
    # every visit's corner differs from the corner of the visit before, and from those 3, 5, 9 and 17 visits before: the distances
    # between the views that try a plan under the back-off's pauses of 0, 2, 4, 8 and 16 views
    for gap in (1, 3, 5, 9, 17):
        assert gap % len(S.CORNERS) != 0


def test_unplannable_scene_has_a_list_above_the_planned_sort_and_its_cut_is_plannable():
    gs, cam = S.unplannable()
    assert (cam.W, cam.H) == (64, 64) and gs.P == S.UNPLANNABLE_P
    counts, _ = S.tile_lists(gs, cam)
    assert counts.max() > PLAN_MAX_LIST - 16, int(counts.max())
    # A lower bound has to hold for the library's own lists, which keep only the instances that can reach alpha 1/255 in their
    # tile: every Gaussian does, in each of the four centre tiles -- at the tile's pixel next to the image centre its alpha
    # (forward.cu's: opacity * exp(-(a dx^2 + c dy^2) / 2 - b dx dy)) is at least twice 1/255, a margin no float rounding eats.
    st = S.oracle_state(gs, cam)
    assert (st["radii"] > 0).all()
    for px in (31.0, 32.0):
        for py in (31.0, 32.0):
            dx, dy = st["means2D"][:, 0] - px, st["means2D"][:, 1] - py
            con = st["conic_opacity"].astype(np.float64)
            alpha = con[:, 3] * np.exp(-0.5 * (con[:, 0] * dx * dx + con[:, 2] * dy * dy) - con[:, 1] * dx * dy)
            assert alpha.min() > 2.0 / 255.0, (px, py, float(alpha.min()))
    assert (counts[1:3, 1:3] == S.UNPLANNABLE_P).all()
    small = S.cut(gs, S.CUT_P)
    assert small.P == S.CUT_P and np.array_equal(small.means3D, gs.means3D[:S.CUT_P])
    counts, R = S.tile_lists(small, cam)
    assert 0 < counts.max() < PART_FROM and R > 0, int(counts.max())


def test_static_cloud_keeps_every_list_short_from_every_camera():
    """Cases 1, 2, 5 and 6: the cloud through the rings of 2, 4 and 6 cameras."""
    gs = S.cloud()
    for n in (2, 4, 6):
        for k, cam in enumerate(S.ring(n)):
            counts, R = S.tile_lists(gs, cam)
            assert 0 < counts.max() < PART_FROM and R > 0, (n, k, int(counts.max()))
            assert (counts == 0).sum() > 0      # (some tiles are light: the plan's bulk-filled tail is exercised too)


def test_soak_scene_keeps_every_list_short_and_moves_as_described():
    soak = S.Soak()
    seen = set()
    for frame in range(S.SOAK_FRAMES):
        order = [soak.camera_of(frame, it) for it in range(S.SOAK_ITERS)]
        assert order[:4] == order[4:8] == order[8:] and len(set(order)) == 4      # four cameras, three visits each, in turn
        seen.update(order)
        for it in (0, S.SOAK_ITERS - 1):
            means, scales = soak.gaussians(frame, it)
            counts, R = S.tile_lists(soak.gs, soak.cams[soak.camera_of(frame, it)], means, scales)
            assert 0 < counts.max() < PART_FROM and R > 0, (frame, it, int(counts.max()))
        step = np.linalg.norm(soak.offset(frame, 1) - soak.offset(frame, 0)) / soak.PIXEL
        assert 0.2 < step < 0.5, step                                            # a fraction of a pixel per iteration
        if frame:
            jump = np.linalg.norm(soak.offset(frame, 0) - soak.offset(frame - 1, S.SOAK_ITERS)) / soak.PIXEL
            assert 2.0 < jump < 4.0, jump                                        # a few pixels at a frame boundary
            assert 0.985 < soak.scale_factor(frame) / soak.scale_factor(frame - 1) < 1.015
        assert np.linalg.norm(soak.offset(frame, 0)) / soak.PIXEL < 16.0         # the cloud stays in view
    assert seen == set(range(S.SOAK_CAMERAS))
    assert any(set(a) & set(b) for a, b in zip(soak.orders, soak.orders[1:]))     # plans are carried across frame boundaries
