"""The backward blend (gsr_blend_bwd.hip) at the edges of a trip, of a chunk and of its one-chunk path, through the public
rasterizer API against the C oracle under tests/parity.py's tolerances, no outliers.

One wave of the kernel serves a (64-entry unit of a tile's list, 8x8 block) pair.  It KEEPS the unit's instances some pixel of the
block replays, evaluates them four per trip and sub-block, in chunks of at most 32, and flushes a chunk's moment table with
atomics.  What a wave does therefore hangs on how many instances its block keeps: 1, 4 | 5 (one trip | two), 31, 32 | 33 (one
chunk | two: the flush hands the table back clean, the lists are reset, the records fetched again), 63, 64 (every lane of the
unit), and on the unit's place in the list (units behind the first start from the forward's snapshot).

Scenes are hand-placed, not random: splats 0.6 px wide (sigma^2 = 0.36 + the 0.3 of the low-pass filter), opacity 0.3, centred
on pixel centres or half-way between two: alpha >= 1/255 out to 2.39 px, and the squared distances such centres make to pixel
centres (.., 4.25, 5 | 6.25, 8, ..) stay clear of that radius, so which (pixel, splat) pairs pass the reference's test does not
hang on rounding.  Before a scene is used, `_kept` counts on the CPU, from the oracle's state alone (the reference's pair test,
list positions below the pixel's n_contrib), how many instances the block in question keeps, and asserts both the count and that
no pair comes within a factor e^0.2 of the threshold (the forward's candidate words carry a margin of e^0.022).  In a one-tile
image every splat covers its own centre pixel, so the library's list is the oracle's and the counts are the kernel's."""
import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

F32 = np.float32
KS = [1, 4, 5, 31, 32, 33, 63, 64]


# ---------------------------------------------------------------- scenes
def _cam(W, H):
    from gaustar_amd import scene
    return scene.look_at_camera((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), W, H, focal_px=200.0)


def _place(cam, u, v):
    """Splats centred on pixel coordinates (u[i], v[i]), list order = index (depth grows with it)."""
    u, v = np.asarray(u, np.float64), np.asarray(v, np.float64)
    n = len(u)
    z = 3.0 + 1e-3 * np.arange(n)
    f = cam.W / (2.0 * cam.tanfovx)
    pv = np.stack([(u - 0.5 * (cam.W - 1)) * z / f, (v - 0.5 * (cam.H - 1)) * z / f, z, np.ones(n)], axis=1)
    world = (pv @ np.linalg.inv(np.asarray(cam.viewmatrix, np.float64)))[:, :3]      # (row vectors: view = world @ viewmatrix)
    s = 0.6 * z / f
    scales = np.stack([s, s, 0.3 * s], axis=1)                                          # (not a sphere: rotations get a gradient)
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
    return dict(means3D=world.astype(F32), opacities=np.full((n, 1), 0.3, F32), scales=scales.astype(F32), rotations=rot.astype(F32))


def _scene_k(k):
    """16x16, a list of 64: k splats on the first k pixels of block 0 (row-major) at k list positions scattered over the unit, the
    other 64 - k on the 4x4 pixels (10..13, 10..13) of block 3, 3 px and more from block 0."""
    pos = np.sort(np.random.default_rng(100 + k).choice(64, k, replace=False))
    u, v = np.zeros(64), np.zeros(64)
    u[pos], v[pos] = np.arange(k) % 8, np.arange(k) // 8
    rest = np.setdiff1d(np.arange(64), pos)
    u[rest], v[rest] = 10 + np.arange(len(rest)) % 4, 10 + (np.arange(len(rest)) // 4) % 4
    return 16, 16, u, v, [((0, 0, 0), k)]


def _scene_long(n):
    """16x16, a list of n > 64 entries, all on block 0's pixels in turn: every unit is kept whole, the last keeps the remainder."""
    i = np.arange(n)
    return 16, 16, i % 8, (i // 8) % 8, [((0, un, 0), min(64, n - 64 * un)) for un in range((n + 63) // 64)]


def _scene_shared():
    """16x16, 40 splats half-way between the columns 7 and 8, five to a row: blocks 0 and 1 keep all 40 -- two chunks in each of
    the two waves, both flushing into the same 40 Gaussians."""
    i = np.arange(40)
    return 16, 16, np.full(40, 7.5), (i % 8).astype(np.float64), [((0, 0, 0), 40), ((0, 0, 1), 40)]


def _scene_17x9():
    """17x9: tile 0's lower blocks have their row 8 only, tile 1 its column 16 only.  Five splats on (0..4, 8): block 2 of tile 0
    keeps five (two trips on one pixel row); 33 on (16, 0..8) in turn: block 0 of tile 1 keeps 33 (two chunks on one column)."""
    i = np.arange(33)
    u = np.concatenate([np.arange(5), np.full(33, 16)])
    v = np.concatenate([np.full(5, 8), i % 9])
    return 17, 9, u, v, [((0, 0, 2), 5), ((1, 0, 0), 33)]


def _scene_33x31():
    """33x31 (3 x 2 tiles): the corner tile 5 has column 32 only, rows 16..30.  33 splats on (32, 16..21) in turn: its block 0
    keeps 33; five on (32, 26..30), 3 px and more from those and from block 0: its block 2 keeps five."""
    i = np.arange(33)
    u = np.full(38, 32)
    v = np.concatenate([16 + i % 6, 26 + np.arange(5)])
    return 33, 31, u, v, [((5, 0, 0), 33), ((5, 0, 2), 5)]


# ---------------------------------------------------------------- the oracle: kept counts and reference, once per (scene, C)
def _kept(st, W, H, tile, unit, blk):
    """Gaussian ids block `blk` of (tile, unit) keeps, by the reference's pair test on the oracle's state."""
    gx = (W + 15) // 16
    ty, tx = divmod(tile, gx)
    a, b = (int(x) for x in st["ranges"][tile])
    ids = st["point_list"][a:b][64 * unit:64 * unit + 64].astype(np.int64)
    ys, xs = ty * 16 + (blk >> 1) * 8 + np.arange(8), tx * 16 + (blk & 1) * 8 + np.arange(8)
    ys, xs = ys[ys < H], xs[xs < W]
    assert len(ids) and len(ys) and len(xs)
    Y, X = np.meshgrid(ys, xs, indexing="ij")
    m, co = st["means2D"][ids].astype(np.float64), st["conic_opacity"][ids].astype(np.float64)
    dx, dy = m[:, 0, None, None] - X, m[:, 1, None, None] - Y
    power = -0.5 * (co[:, 0, None, None] * dx * dx + co[:, 2, None, None] * dy * dy) - co[:, 1, None, None] * dx * dy
    ln_a = np.log(255.0 * co[:, 3, None, None]) + power                      # ln(255 alpha)
    assert np.abs(ln_a).min() >= 0.2, f"a pair within e^{np.abs(ln_a).min():.3f} of alpha = 1/255: rebuild the scene"
    replayed = (64 * unit + np.arange(len(ids)))[:, None, None] < st["n_contrib"][Y, X].astype(np.int64)[None]
    return ids[((ln_a >= 0.0) & (power <= 0.0) & replayed).any(axis=(1, 2))]


_CASES = {}


def _case(name, build, C):
    """(kw, dL_dpix, reference) of a scene for C channels; the oracle renders three channels per pass, so channels 3.. are a second
    pass over the same geometry: geometry gradients add up, colour gradients split (four channels: the fourth rides in channel
    0 of the second pass)."""
    if (name, C) in _CASES:
        return _CASES[(name, C)]
    W, H, u, v, want = build()
    cam = _cam(W, H)
    g = _place(cam, u, v)
    P = len(u)
    rng = np.random.default_rng(7)
    cols, bg = rng.uniform(0.0, 1.0, size=(P, C)).astype(F32), rng.uniform(0.0, 1.0, size=C).astype(F32)
    dpix = rng.normal(size=(C, H, W)).astype(F32)
    kw = dict(means3D=g["means3D"], opacities=g["opacities"], view=cam.viewmatrix, proj=cam.projmatrix, campos=cam.campos, W=W, H=H,
              tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg, shs=None, colors_precomp=cols, scales=g["scales"],
              rotations=g["rotations"], cov3D_precomp=None, sh_degree=0, scale_modifier=1.0)
    st, ga = parity.run_oracle(dict(kw, bg=bg[:3], colors_precomp=np.ascontiguousarray(cols[:, :3])), np.ascontiguousarray(dpix[:3]))
    for (tile, unit, blk), k in want:
        got = _kept(st, W, H, tile, unit, blk)
        assert len(got) == k, f"{name}: block {blk} of tile {tile}, unit {unit} keeps {len(got)} instances, not {k}: rebuild the scene"
    if name == "shared":
        assert np.array_equal(np.sort(_kept(st, W, H, 0, 0, 0)), np.sort(_kept(st, W, H, 0, 0, 1)))
    ref = {k_: np.asarray(ga[k_], np.float64) for k_ in parity.GRAD_KEYS}
    color = st["color"].copy()
    if C > 3:
        if C == 4:
            c2, bg2, d2 = np.repeat(cols[:, 3:4], 3, axis=1), np.repeat(bg[3:4], 3), np.concatenate([dpix[3:4], 0 * dpix[:2]])
        else:
            c2, bg2, d2 = cols[:, 3:6], bg[3:6], dpix[3:6]
        st2, gb = parity.run_oracle(dict(kw, bg=bg2, colors_precomp=np.ascontiguousarray(c2)), np.ascontiguousarray(d2))
        for k_ in parity.GRAD_KEYS:
            if k_ != "dL_dcolors":
                ref[k_] = ref[k_] + np.asarray(gb[k_], np.float64)
        ref["dL_dcolors"] = np.concatenate([ref["dL_dcolors"], np.asarray(gb["dL_dcolors"], np.float64)[:, :C - 3]], axis=1)
        color = np.concatenate([color, st2["color"][:C - 3]])
    _CASES[(name, C)] = (kw, dpix, dict(color=color, radii=st["radii"].copy(), grads=ref))
    return _CASES[(name, C)]


def _run(name, build, C):
    kw, dpix, ref = _case(name, build, C)
    hip = parity.run_hip(kw, dpix)
    assert hip["color"].shape == ref["color"].shape and hip["dL_dcolors"].shape == (len(kw["means3D"]), C)
    parity.compare_hip_to(hip, ref["color"], ref["radii"], ref["grads"], what=f"{name} C={C}")


# ---------------------------------------------------------------- the cases
@pytest.mark.parametrize("C", [3, 4, 6])
@pytest.mark.parametrize("k", KS)
def test_block_keeps_k_of_a_unit(k, C):
    _run(f"k={k}", lambda: _scene_k(k), C)


@pytest.mark.parametrize("C", [3, 6])
@pytest.mark.parametrize("k", [33, 64])
def test_block_keeps_k_flags_ignored(k, C, monkeypatch):
    """The same scenes with the forward's live flags ignored: every (unit, block) wave runs, none leaves early."""
    monkeypatch.setenv("GSR_BWD_LIVE", "0")
    _run(f"k={k}", lambda: _scene_k(k), C)


@pytest.mark.parametrize("C", [3, 4, 6])
@pytest.mark.parametrize("n", [65, 129])
def test_second_and_third_unit(n, C):
    _run(f"list of {n}", lambda: _scene_long(n), C)


@pytest.mark.parametrize("C", [3, 4, 6])
def test_two_chunks_in_two_waves_on_the_same_gaussians(C):
    _run("shared", _scene_shared, C)


@pytest.mark.parametrize("C", [3, 4, 6])
@pytest.mark.parametrize("size", ["17x9", "33x31"])
def test_partial_blocks(size, C):
    _run(size, _scene_17x9 if size == "17x9" else _scene_33x31, C)
