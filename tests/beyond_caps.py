"""Cases that run the capped grids and the shared fixed-order reduction PAST their caps, shared by tests/test_beyond_caps.py
(CPU) and tests/test_gpu_beyond_caps.py (GPU).  TEST INFRASTRUCTURE ONLY, numpy only.

The suite pins most kernels at the smallest shapes that reach every branch.  One kind of branch needs a large shape: the second
trip of a grid-stride loop behind a capped grid, the second partial per lane of gsr_reduce.h's tree_total, the wrap of
md_big_kernel's fixed grid of waves, an interior segment of hull_row_kernel.  Every shape below is derived from the caps as the
sources state them (caps()), through the named helpers, so that a moved cap moves the shapes with it; tests/test_beyond_caps.py
asserts today's values and that each case still crosses its cap in the way its name says.

    gsr_reduce.h      an element pass of ceil(n / RED_BLOCK) workgroups, at most RED_MAX_WGS, each lane striding by the grid's
                      size; one partial per workgroup; tree_total's RED_BLOCK lanes add the partials i, i + RED_BLOCK, ...
    gsr_prep.hip      prep_rectify_kernel: at most PREP_MAX_BLOCKS workgroups of PREP_BLOCK lanes over quads of four pixels (dst
                      4-byte aligned) or over pixels (unaligned dst)
    gsr_meshdepth.hip md_big_kernel: MD_BIG_BLOCKS * MD_BLOCK / 64 waves over n_huge * MD_SLICES + n_mid work items
    gsr_hull.hip      hull_row_kernel: one wave per 64 * HD_LANE_PX pixels of a row, HD_HALO pixels of halo on either side
    gsr_param_reg.hip a lane takes PR_G Gaussians; the groups are gsr_reduce.h's elements"""
import collections
import functools
import math
import os
import re

import numpy as np

import meshdepth_ref
import prep_ref
from conftest import ROOT

CSRC = os.path.join(ROOT, "gaustar_amd", "csrc")
CAP_SOURCES = collections.OrderedDict([
    ("gsr_reduce.h", ("RED_BLOCK", "RED_MAX_WGS")),
    ("gsr_prep.hip", ("PREP_BLOCK", "PREP_MAX_BLOCKS")),
    ("gsr_meshdepth.hip", ("MD_BLOCK", "MD_BIG_BLOCKS", "MD_SLICES", "MD_MID_MAX", "MD_SMALL_MAX")),
    ("gsr_hull.hip", ("HD_LANE_PX", "HD_HALO", "HD_MAX_R")),
    ("gsr_param_reg.hip", ("PR_G",)),
])


@functools.lru_cache(maxsize=None)
def caps():
    """name -> value of every `constexpr int NAME = <digits>;` listed in CAP_SOURCES, read from the sources."""
    out = {}
    for fname, names in CAP_SOURCES.items():
        with open(os.path.join(CSRC, fname)) as fh:
            src = fh.read()
        for name in names:
            m = re.findall(r"constexpr int %s = (\d+);" % name, src)
            assert len(m) == 1, f"{fname} no longer states {name} as `constexpr int {name} = <n>;`"
            out[name] = int(m[0])
    return out


# ---------------------------------------------------------------------------------------------- gsr_reduce.h
def one_partial_per_lane():
    """Elements whose workgroups' partials give tree_total's every lane exactly one: beyond it a lane adds a second."""
    return caps()["RED_BLOCK"] ** 2


def one_trip():
    """Elements the capped grid covers in one trip: beyond it the element pass loops."""
    return caps()["RED_BLOCK"] * caps()["RED_MAX_WGS"]


Launch = collections.namedtuple("Launch", "workgroups trips last_trip partials_per_lane")


def _launch(items, block, max_wgs):
    wgs = min(-(-items // block), max_wgs)
    per_trip = wgs * block
    trips = -(-items // per_trip)
    return wgs, trips, items - (trips - 1) * per_trip


def reduce_launch(n):
    """Of an element pass over n elements: the workgroups launched, the trips of the busiest lane, the elements the last trip
    holds, and the partials tree_total's lane 0 adds."""
    wgs, trips, last = _launch(n, caps()["RED_BLOCK"], caps()["RED_MAX_WGS"])
    return Launch(wgs, trips, last, -(-wgs // caps()["RED_BLOCK"]))


def sse_shapes():
    """name -> [C,H,W] of the image pairs.
    partials   3 s s with s three past the largest square under one_partial_per_lane / 3: a few lanes add a second partial
    one_trip   3 (w + 1) w with 3 w w just under one_trip: one full trip and a ragged second one
    two_trips  1 (w + 1) w with w w = 2 one_trip: two full trips and one more row"""
    s = math.isqrt(one_partial_per_lane() // 3) + 3
    w = math.isqrt(one_trip() // 3)
    w2 = math.isqrt(2 * one_trip())
    return collections.OrderedDict([("partials", (3, s, s)), ("one_trip", (3, w + 1, w)), ("two_trips", (1, w2 + 1, w2))])


MASKED = "one_trip"        # the shape that is also compared under a mask and from a permuted view


@functools.lru_cache(maxsize=None)
def sse_pair(name):
    """(pred, gt) f32 [C,H,W]: the value ranges of tests/test_gpu_evaluate.py's _pair (pred leaves [0, 1] on both sides)."""
    shape = sse_shapes()[name]
    rng = np.random.default_rng(7000 + sum(shape))
    return rng.uniform(-0.2, 1.2, size=shape).astype(np.float32), rng.uniform(0, 1, size=shape).astype(np.float32)


def sse_mask(name=MASKED):
    """[H,W] bool: every second column."""
    _, h, w = sse_shapes()[name]
    m = np.zeros((h, w), bool)
    m[:, ::2] = True
    return m


def sse_hwc(name=MASKED):
    """The pair stored [H,W,C]: permuted back to [C,H,W] it is a non-contiguous view of the same values."""
    pred, gt = sse_pair(name)
    return np.ascontiguousarray(pred.transpose(1, 2, 0)), np.ascontiguousarray(gt.transpose(1, 2, 0))


RAGGED_TAIL = 200 * 256 + 227          # a third trip that ends inside a workgroup (whatever RED_BLOCK is, it is no multiple)


def mean_sizes():
    """Lengths of the plain f64 vectors: one element into the second partial, one into the second trip, a ragged third trip."""
    return one_partial_per_lane() + 1, one_trip() + 1, 2 * one_trip() + RAGGED_TAIL


@functools.lru_cache(maxsize=None)
def mean_vector(n):
    """[n] f64 positive values over three decades."""
    return np.exp(np.random.default_rng(n).uniform(-3.0, 3.0, size=n))


def stats_sizes():
    """n_samples of the distance statistics: into the second partial per lane, and into the second trip."""
    return one_partial_per_lane() + 4465, one_trip() + 75713


STATS_THRESHOLDS = (0.004, 0.01, 0.03)
STATS_SEED = 9


def stats_meshes():
    """The 320-face sphere pair of tests/test_gpu_evaluate.py's test_means_maxima_and_counts_against_numpy."""
    import eval_ref
    verts, faces = eval_ref.icosphere(2)
    other = verts * np.array([1.02, 0.97, 1.0]) + np.array([0.004, 0.0, -0.003])
    return verts, faces, other


def fit_sizes():
    """K of the rigid fit: a few workgroups past one partial per lane; two workgroups and one anchor into the second trip."""
    return one_partial_per_lane() + 464, one_trip() + 2 * caps()["RED_BLOCK"] + 1


FIT_FRAMES = 2


@functools.lru_cache(maxsize=None)
def fit_anchors(K, T=FIT_FRAMES):
    """(src [K,3], dst [T,K,3], Rs, ts): dst[t] = Rs[t] src + ts[t] with the lost points tests/test_gpu_edit.py's test_fit_sums
    plants: a NaN row in the last frame, a single NaN coordinate in frame 0 and one in src."""
    import edit_ref
    rng = np.random.default_rng(100 * K + T)
    src = rng.normal(size=(K, 3))
    Rs, ts = [edit_ref.rotation(rng) for _ in range(T)], rng.normal(size=(T, 3))
    dst = np.stack([src @ R.T + t for R, t in zip(Rs, ts)])
    dst[T - 1, K // 2] = np.nan
    dst[0, K - 1, 1] = np.nan
    src[1, 2] = np.nan
    return src, dst, Rs, ts


def param_reg_sizes():
    """(N, M) of the Gaussian-parameter regularisers: the size the suite had, config C's 491 520 Gaussians, and two groups of
    PR_G into the second trip, the last of them holding one Gaussian."""
    g = caps()["PR_G"]
    return (100_003, 60_001), (491_520, 300_001), (g * (one_trip() + 2) - (g - 1), 1_300_003)


def param_reg_launch(N):
    return reduce_launch(-(-N // caps()["PR_G"]))


# ---------------------------------------------------------------------------------------------- gsr_prep.hip
BORDER = (7, 200, 33, 129)
DIST = (-0.2, 0.05, 1e-3, -2e-3, 0.01)
SHIFT = (3.25, -2.5)
RectCase = collections.namedtuple("RectCase", "h w c intr dist cam4 border unaligned")


def rectify_trip():
    """Work items (quads of four pixels, or pixels) one trip of prep_rectify_kernel's capped grid covers."""
    return caps()["PREP_BLOCK"] * caps()["PREP_MAX_BLOCKS"]


def rectify_case(which):
    """dword: (w + 1) w 1 with w w / 4 = rectify_trip(): one row of quads into the second trip; the distorted path.
    byte:  (w + 1) w 3 with w w = rectify_trip(), dst one byte off alignment: one row of pixels into the second trip; the
           fractional shift.
    The cameras are built as tests/test_gpu_prep.py's _case builds them (the principal point SHIFT off the centre).  The
    distorted camera's focal length is w / 2.8, a normalised half-width of 1.4: rad = 1 + r2 (k1 + r2 (k2 + r2 k3)) stays
    below 1 up to r2 = 2.6, so the middle of every edge -- the last row, which is the second trip, with it -- samples the
    source, while the corners (r2 = 3.9) sample the border.  (_case's focal of 60 pixels, made for 128 columns, would leave a
    disc of 100 pixels in the middle and nothing but border in the second trip.)"""
    if which == "dword":
        w = math.isqrt(4 * rectify_trip())
        h, c, dist, f, unaligned = w + 1, 1, DIST, w / 2.8, False
    else:
        w = math.isqrt(rectify_trip())
        h, c, dist, f, unaligned = w + 1, 3, None, 500.0, True
    dx, dy = SHIFT
    intr = np.array([[f, 0.0, w / 2 + dx], [0.0, f, h / 2 + dy], [0.0, 0.0, 1.0]])
    return RectCase(h, w, c, intr, dist, (f, f, w / 2 + dx, h / 2 + dy), BORDER[:c], unaligned)


def rectify_launch(case):
    """(workgroups, trips, work items of the last trip) of the launch gsr_prep.hip's launch_rectify makes."""
    n = case.h * case.w
    items = n if case.unaligned else (n + 3) // 4
    return _launch(items, caps()["PREP_BLOCK"], caps()["PREP_MAX_BLOCKS"])


@functools.lru_cache(maxsize=None)
def rectify_source(which):
    k = rectify_case(which)
    return prep_ref.hash_image(k.h + k.c, k.h, k.w, k.c)


@functools.lru_cache(maxsize=None)
def rectify_want(which):
    """prep_ref.rectify of the case, computed once and left unchanged."""
    k = rectify_case(which)
    out = prep_ref.rectify(rectify_source(which), k.cam4, k.dist, k.border)
    out.setflags(write=False)
    return out


# ---------------------------------------------------------------------------------------------- gsr_meshdepth.hip
def big_waves():
    return caps()["MD_BIG_BLOCKS"] * (caps()["MD_BLOCK"] // 64)


def pinhole(f):
    """cam16 of the camera at the origin that looks down +z, principal point (0, 0): image coordinates are f X / Z."""
    return np.array([1, 0, 0, 0, 1, 0, 0, 0, 1, 0, 0, 0, f, f, 0, 0], np.float64)


def _lift(cam, px, py, z):
    """World points that project to pixel (px, py) at depth z."""
    f = cam[12]
    return np.stack([(px - cam[14]) / f * z, (py - cam[15]) / f * z, z], -1)


MeshCase = collections.namedtuple("MeshCase", "verts faces cam H W")
WALL_CELL = 3                # pixels per cell side: a triangle's range is 3 x 3 pixels


def wall_cells():
    """(rows, cols) of the wall's cells, two triangles each: more triangles than md_big_kernel has waves."""
    rows = math.isqrt(big_waves() // 2)
    return rows, rows + 1


@functools.lru_cache(maxsize=None)
def depth_wall():
    """A bumpy wall of 2 rows cols triangles facing the camera.  The vertices sit at pixels (3 i - 0.5, 3 j - 0.5), so every
    triangle's range is 3 x 3 pixel centres, three of them strictly inside it: under small_max = 1 every triangle is a mid face,
    and every triangle wins a pixel (the surface is a height field: no other triangle covers its interior)."""
    rows, cols = wall_cells()
    cam = pinhole(1024.0)
    rng = np.random.default_rng(31)
    j, i = np.mgrid[0:rows + 1, 0:cols + 1]
    z = 2.0 + rng.uniform(-0.2, 0.2, size=i.shape)
    verts = _lift(cam, WALL_CELL * i - 0.5, WALL_CELL * j - 0.5, z).reshape(-1, 3)
    vid = lambda jj, ii: (jj * (cols + 1) + ii).reshape(-1)
    jj, ii = np.mgrid[0:rows, 0:cols]
    lower = np.stack([vid(jj, ii), vid(jj, ii + 1), vid(jj + 1, ii)], -1)
    upper = np.stack([vid(jj, ii + 1), vid(jj + 1, ii + 1), vid(jj + 1, ii)], -1)
    faces = np.stack([lower, upper], 1).reshape(-1, 3).astype(np.int64)
    return MeshCase(verts, faces, cam, WALL_CELL * rows + 2, WALL_CELL * cols + 5)     # (a margin no face reaches)


FAN_H, FAN_W = 96, 320
FAN_EXTRA = 12


def fan_faces():
    """Huge faces whose MD_SLICES items each exceed md_big_kernel's waves by FAN_EXTRA faces' worth."""
    return big_waves() // caps()["MD_SLICES"] + FAN_EXTRA


@functools.lru_cache(maxsize=None)
def depth_fan():
    """fan_faces() triangles, each over the whole FAN_H x FAN_W image (and past it), in a shuffled order.  A plane's inverse depth
    is affine in the image; face k's is the tangent of the strictly convex g(c) = 0.3 + 1e-6 (c - W / 2)^2 at its own column
    c_k = 20 + 2 k, constant along a column.  The largest tangent at column c_k is face k's, by g''/2 (c_k - c_j)^2 >= 4e-6 of
    0.3: some 200 f32 steps of the depth, so every face is the nearest in its own band of columns."""
    n = fan_faces()
    cam = pinhole(512.0)
    first = 20
    step = (FAN_W - 2 * first) // n
    assert step >= 2, "the image is too narrow for the fan's bands"
    cols = first + step * np.random.default_rng(32).permutation(n)
    a = 1e-6
    corners = np.array([[-200.0, -50.0], [520.0, -50.0], [160.0, 300.0]])      # holds [0, W - 1] x [0, H - 1] with a margin
    verts = []
    for ck in cols:
        iz = (0.3 + a * (ck - FAN_W / 2) ** 2) + 2 * a * (ck - FAN_W / 2) * (corners[:, 0] - ck)
        assert (iz > 0.01).all()
        verts.append(_lift(cam, corners[:, 0], corners[:, 1], 1.0 / iz))
    return MeshCase(np.concatenate(verts), np.arange(3 * n, dtype=np.int64).reshape(n, 3), cam, FAN_H, FAN_W), cols


def pixel_ranges(case, znear=0.01):
    """[F] int64: the pixels in each face's range by the rules of gsr_meshdepth.hip (0: the face is skipped), restated from
    tests/meshdepth_ref.py's render: what md_face_kernel compares with small_max and MD_MID_MAX."""
    X, Y, Z = meshdepth_ref.project(case.cam, case.verts)
    out = np.zeros(len(case.faces), np.int64)
    for f, tri in enumerate(case.faces):
        x, y, z = X[tri], Y[tri], Z[tri]
        if (z <= znear).any():
            continue
        area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
        if area == 0.0 or not np.isfinite(area):
            continue
        c_lo, c_hi = max(np.ceil(x.min()), 0.0), min(np.floor(x.max()), float(case.W - 1))
        r_lo, r_hi = max(np.ceil(y.min()), 0.0), min(np.floor(y.max()), float(case.H - 1))
        if c_lo <= c_hi and r_lo <= r_hi:
            out[f] = (int(c_hi) - int(c_lo) + 1) * (int(r_hi) - int(r_lo) + 1)
    return out


def big_items(case, small_max):
    """(n_mid, n_huge, work items of md_big_kernel) for the case under small_max."""
    n = pixel_ranges(case)
    listed = n > small_max
    n_mid, n_huge = int((listed & (n <= caps()["MD_MID_MAX"])).sum()), int((n > max(small_max, caps()["MD_MID_MAX"])).sum())
    return n_mid, n_huge, n_huge * caps()["MD_SLICES"] + n_mid


@functools.lru_cache(maxsize=None)
def depth_want(which):
    """meshdepth_ref.render of the wall / the fan, computed once."""
    case = depth_wall() if which == "wall" else depth_fan()[0]
    return meshdepth_ref.render(case.verts, case.faces, case.cam, case.H, case.W)


# ---------------------------------------------------------------------------------------------- gsr_hull.hip
HULL_ROWS, HULL_QUIET_ROW = 5, 3
HULL_RADII = (1, 127)
HULL_RUN = (100, 500)        # one run of 400 inside pixels in row 2: distances along the row beyond the cap


def hull_segment():
    return 64 * caps()["HD_LANE_PX"]


def hull_width():
    """Two whole segments and a third wider than a halo: the second segment's halos are real pixels of its two neighbours."""
    return 2 * hull_segment() + caps()["HD_HALO"] + 24


def hull_boundaries():
    return hull_segment(), 2 * hull_segment()


def hull_empty_zones():
    """Column ranges without an inside pixel in any row, each wider than two radii (or running to the image's end, 127 past
    the last inside pixel): their middles are capped at R = 127.  One on either side of each segment boundary, more than a halo away from it
    (but for the last, the short third segment), so that the halos hold sparse pixels too."""
    seg, w = hull_segment(), hull_width()
    return (seg - 464, seg - 184), (seg + 180, seg + 460), (2 * seg - 460, 2 * seg - 180), (2 * seg + 6, w)


@functools.lru_cache(maxsize=None)
def hull_mask():
    """[5, hull_width()] uint8: sparse random inside pixels; a run of inside pixels across each segment boundary (columns
    b - 9 .. b + 5) in every row but HULL_QUIET_ROW, which has no inside pixel within a halo of either boundary, so what its
    halos carry is "nothing found"; HULL_RUN; and hull_empty_zones()."""
    w, halo = hull_width(), caps()["HD_HALO"]
    rng = np.random.default_rng(5)
    m = (rng.random((HULL_ROWS, w)) < 0.01).astype(np.uint8) * 255
    for lo, hi in hull_empty_zones():
        m[:, lo:hi] = 0
    for b in hull_boundaries():
        m[:, b - 9:b + 6] = 255
        m[HULL_QUIET_ROW, b - halo:b + halo] = 0
    m[2, HULL_RUN[0]:HULL_RUN[1]] = 255
    m.setflags(write=False)
    return m


# In hull_mask() a pixel near a boundary is never more than three rows from the quiet row or from a run, so the column pass
# hides most of what the row pass read from a halo.  The masks below have three rows alike -- the squared distance of a pixel
# is then the square of its distance along the row -- and are there for what the halos HOLD.  Around a boundary b the only
# inside pixels are one at b - a and one at b + c: for a > c the pixels less than (a - c) / 2 before b find the one at b + c,
# in the right halo of their segment; for c > a those less than (c - a) / 2 after b find the one at b - a, in the left halo.
#   near  offsets 20 and 48: the halo's first word (up to 64 columns away)
#   far   offsets 70 and 210: the second word (64 .. 127 columns away)
# each looking right at the first boundary and left at the second (_a) and the other way round (_b), and each also inverted,
# where it is the inside pixels that look for outside ones (the kernel keeps a word array per kind).
HULL_HALO_CASES = collections.OrderedDict([("near_a", ((48, 20), (20, 48))), ("near_b", ((20, 48), (48, 20))),
                                           ("far_a", ((210, 70), (70, 210))), ("far_b", ((70, 210), (210, 70)))])
HULL_CLEARED = 220           # columns on either side of a boundary that hold nothing but the two pixels


@functools.lru_cache(maxsize=None)
def hull_halo_masks():
    """name -> [3, hull_width()] uint8, for R = 127: sparse random pixels, and HULL_HALO_CASES around the boundaries."""
    w = hull_width()
    out = collections.OrderedDict()
    for k, (name, offsets) in enumerate(HULL_HALO_CASES.items()):
        row = (np.random.default_rng(60 + k).random(w) < 0.03).astype(np.uint8) * 255
        for b, (a, c) in zip(hull_boundaries(), offsets):
            row[b - HULL_CLEARED:b + HULL_CLEARED] = 0
            row[b - a] = 255
            if b + c < w:
                row[b + c] = 255
        out[name] = np.repeat(row[None], 3, axis=0)
        out[name + "_inverted"] = 255 - out[name]
    for m in out.values():
        m.setflags(write=False)
    return out


def hull_with_halo_of(mask, radius, k):
    """hull_ref.mask_distance as a row pass would give it that saw only k columns beyond its own segment: each segment
    restated alone with k columns of its neighbours, then cropped.  k >= radius is the restatement itself."""
    import hull_ref
    seg, w = hull_segment(), mask.shape[1]
    parts = []
    for a in range(0, w, seg):
        lo, hi = max(a - k, 0), min(a + seg + k, w)
        parts.append(hull_ref.mask_distance(np.ascontiguousarray(mask[:, lo:hi]), 128, radius)[:, a - lo:a - lo + min(seg, w - a)])
    return np.concatenate(parts, axis=1)
