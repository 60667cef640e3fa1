"""Scenes of the planned-view lifecycle tests (test_gpu_plan_lifecycle.py), as plain numpy: the GPU tests render them, and
test_plan_lifecycle_scenes.py proves on the CPU oracle that they do what those tests lean on (list lengths, where the
instances fall) -- so a failure on the GPU is the library's and not the scene's.  Everything is seeded; nothing here needs a GPU."""
import math

import numpy as np

from gaustar_amd import scene

W = H = 128                       # 64 tiles; the unplannable case: 64 x 64 = 16 tiles, the smallest image a plan exists for
EYE_DISTANCE = 4.0
SMALL = (0.01, 0.03)              # scale_range of every scene here
BOX = ((-1.2, 1.2), (-1.2, 1.2), (-0.5, 0.5))
CORNERS = ((-1.1, -1.1), (1.1, 1.1), (-1.1, 1.1), (1.1, -1.1))   # case 3: where the cluster goes, visit by visit
CORNER_P = 600
UNPLANNABLE_P, CUT_P = 2200, 800
SOAK_P, SOAK_CAMERAS, SOAK_FRAMES, SOAK_ITERS, SOAK_VISITS = 1500, 8, 40, 12, 3
BG = np.zeros(3, np.float32)


def camera(azimuth=0.0, elevation=0.0, w=W, h=H):
    """The base camera -- eye (0, 0, -4) looking at the origin -- with its eye turned about the origin."""
    ce = math.cos(elevation)
    eye = (-EYE_DISTANCE * math.sin(azimuth) * ce, EYE_DISTANCE * math.sin(elevation), -EYE_DISTANCE * math.cos(azimuth) * ce)
    return scene.look_at_camera(eye, (0.0, 0.0, 0.0), w, h, fovx=0.9, znear=0.01)


def ring(n):
    """n cameras around the origin, every other one a little above / below the equator."""
    return [camera(2.0 * math.pi * k / n, 0.3 * (k % 3 - 1)) for k in range(n)]


def cloud(P=1000, seed=11):
    """The static scene of the eviction, hint and stream cases."""
    return scene.random_gaussians(P, np.random.default_rng(seed), box=BOX, scale_range=SMALL)


def corner_cluster(visit, seed=23):
    """Case 3: a compact cluster of 600 Gaussians in the image corner of `visit` (the same Gaussians, moved)."""
    cx, cy = CORNERS[visit % len(CORNERS)]
    return scene.random_gaussians(CORNER_P, np.random.default_rng(seed), box=((cx - 0.2, cx + 0.2), (cy - 0.2, cy + 0.2), (-0.2, 0.2)),
                                  scale_range=SMALL)


def unplannable(seed=31):
    """Case 4: 2 200 small Gaussians within a third of a pixel of the centre of a 64 x 64 image -- the corner that four tiles
    share, so each of the four holds them all: lists above PLAN_MAX_LIST - 16 = 2 032.  -> (Gaussians, camera)"""
    gs = scene.random_gaussians(UNPLANNABLE_P, np.random.default_rng(seed), box=((-0.02, 0.02), (-0.02, 0.02), (-0.2, 0.2)),
                                scale_range=SMALL)
    return gs, camera(w=64, h=64)


def cut(gs, n):
    """The first n Gaussians of gs."""
    return scene.GaussianSet(means3D=gs.means3D[:n].copy(), opacities=gs.opacities[:n].copy(), scales=gs.scales[:n].copy(),
                             rotations=gs.rotations[:n].copy(), colors_precomp=gs.colors_precomp[:n].copy())


class Soak:
    """Case 7, the windowed refinement loop in miniature: SOAK_FRAMES frames of SOAK_ITERS iterations.  A frame works on four of the
    eight cameras -- the head of a seeded permutation drawn per frame -- three visits each, in turn (the reference's loop visits a
    camera three times per frame); the Gaussians drift by a third of a pixel per iteration, jump by three pixels at a frame
    boundary (the next frame's mesh), and their scales grow or shrink by a per cent per frame.  Drift and jump turn from frame to
    frame, so the cloud stays in view."""
    PIXEL = 2.0 * EYE_DISTANCE * math.tan(0.45) / W     # world units per pixel at the origin's depth, ~0.03

    def __init__(self, seed=41):
        self.gs = scene.random_gaussians(SOAK_P, np.random.default_rng(seed), box=BOX, scale_range=SMALL)
        self.cams = ring(SOAK_CAMERAS)
        self.rng = np.random.default_rng(seed + 1)
        self.orders = [self.rng.permutation(SOAK_CAMERAS)[:SOAK_ITERS // SOAK_VISITS] for _ in range(SOAK_FRAMES)]

    def camera_of(self, frame, it):
        order = self.orders[frame]
        return int(order[it % len(order)])

    def offset(self, frame, it):
        off = np.zeros(3)
        for f in range(frame + 1):
            steps = SOAK_ITERS if f < frame else it
            off[:2] += steps * self.PIXEL / 3.0 * np.array([math.cos(1.1 * f), math.sin(1.1 * f)])
            if f > 0:
                off[:2] += 3.0 * self.PIXEL * np.array([math.cos(2.4 * f), math.sin(2.4 * f)])
        return off

    def scale_factor(self, frame):
        up = frame % 20 if frame % 20 <= 10 else 20 - frame % 20      # ten frames up, ten down
        return 1.01 ** up

    def gaussians(self, frame, it):
        """-> (means3D, scales) of iteration `it` of `frame`, float32."""
        return ((self.gs.means3D.astype(np.float64) + self.offset(frame, it)).astype(np.float32),
                (self.gs.scales.astype(np.float64) * self.scale_factor(frame)).astype(np.float32))


def oracle_state(gs, cam, means3D=None, scales=None):
    """The CPU oracle's forward of gs through cam (oracle.forward's dict)."""
    from oracle import oracle
    return oracle.forward(gs.means3D if means3D is None else means3D, gs.opacities, cam.viewmatrix, cam.projmatrix, cam.campos, cam.W,
                          cam.H, cam.tanfovx, cam.tanfovy, BG, colors_precomp=gs.colors_precomp,
                          scales=gs.scales if scales is None else scales, rotations=gs.rotations)


def tile_lists(gs, cam, means3D=None, scales=None):
    """The oracle's per-tile lists: -> (their lengths as a [tiles_y, tiles_x] array, R).  These are the REFERENCE's lists, every
    tile of a splat's bounding square; the library drops the instances that cannot reach alpha 1/255 in their tile
    (gsr_preprocess.hip), so its lists are these or shorter -- an upper bound carries over, a lower bound does not."""
    from oracle import oracle
    st = oracle_state(gs, cam, means3D, scales)
    gx, gy = oracle.tile_grid(cam.W, cam.H)
    r = st["ranges"].astype(np.int64)
    return (r[:, 1] - r[:, 0]).reshape(gy, gx), int(st["num_rendered"])
