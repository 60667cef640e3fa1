"""The forward blend's per-(unit, 8x8 block) live flags (gsr_blend_fwd.hip -> the unit table's live bits, read back through
gsr_debug_export_units) and the backward blend that leaves on them (gsr_blend_bwd.hip, GSR_BWD_LIVE).  A flag may say live for a wave without work; it may never say dead for a wave
with a live pair -- that wave's gradient contributions would be lost.

Images are 48 x 40: 3 x 3 tiles, the bottom row clipped after its upper blocks (blocks 2 and 3 of those tiles lie outside the
image and never blend anything).  Constructed scenes put Gaussians wider than the image over the middle tile (pixels 16..31 in x
and y), so every tile holds the same list and the flags are known by construction; the random scene is checked between two
integer-exact bounds read from the forward's own state.  Gradients of every case are compared with the C oracle under
tests/parity.py, without outliers, with the flags used and ignored.

Expectations come from the construction, the formats and the oracle, never from the kernels:
  * wall splats: opacity 0.99, 200 px wide, centred half a pixel off every pixel centre, so alpha = 0.99 G lies in [0.978, 0.98999]
    over the image: (1 - alpha)^2 stays above 1e-4 by 0.1 % (a hundred times the rounding of 1 - alpha) and (1 - alpha)^3 is ten
    times below it: every pixel blends two of them and stops at the third;
  * thin splats: opacity 0.0041, 400 px wide: alpha stays 4 % above 1/255 and 2 048 of them leave T = 2.2e-4 > 1e-4: a pixel
    blends every one of them."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity

pytestmark = pytest.mark.gpu

F32 = np.float32
W, H = 48, 40
GX, GY = 3, 3
MID = 4                     # tile (1, 1)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dscales", "dL_drotations"]
HIP_ORDER = ["dL_dmeans2D", "dL_dcolors", "dL_dopacity", "dL_dmeans3D", "dL_dcov3D", "dL_dsh", "dL_dscales", "dL_drotations"]


# ---------------------------------------------------------------- scenes
def _cam():
    from gaustar_amd import scene
    return scene.look_at_camera((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), W, H, focal_px=200.0)


def _place(cam, u, v, z, sx, sy, opacity):
    """Axis-aligned Gaussians centred on pixel (u, v) at view depth z, (sx, sy) pixels wide -> dict of float32 arrays."""
    u, v, z, sx, sy, opacity = (np.atleast_1d(np.asarray(a, np.float64)) for a in (u, v, z, sx, sy, opacity))
    n = len(z)
    u, v, sx, sy, opacity = (np.broadcast_to(a, (n,)) for a in (u, v, sx, sy, opacity))
    f = cam.W / (2.0 * cam.tanfovx)
    pv = np.stack([(u - 0.5 * (cam.W - 1)) * z / f, (v - 0.5 * (cam.H - 1)) * z / f, z, np.ones(n)], axis=1)
    world = (pv @ np.linalg.inv(np.asarray(cam.viewmatrix, np.float64)))[:, :3]      # (row vectors: view = world @ viewmatrix)
    scales = np.stack([sx * z / f, sy * z / f, 0.15 * (sx + sy) * z / f], axis=1)      # (not a sphere: rotations get a gradient)
    rot = np.tile(np.array([1.0, 0.0, 0.0, 0.0]), (n, 1))
    return dict(means3D=world.astype(F32), opacities=opacity.reshape(n, 1).astype(F32), scales=scales.astype(F32), rotations=rot.astype(F32))


def _cat(*parts):
    return {k: np.concatenate([p[k] for p in parts]) for k in parts[0]}


def _wall(cam, count, z0, half):
    """`count` opaque splats in front: over the whole middle tile, or (half) over its left blocks only -- 20 px wide about x = 19.5:
    alpha >= 0.96 for x <= 23 (stops at the third), alpha <= 0.84 at x = 31 (T = 4e-3 behind the three)."""
    return _place(cam, 19.5 if half else 23.5, 23.5, z0 + 1e-3 * np.arange(count), 20.0 if half else 200.0, 100.0 if half else 200.0, 0.99)


def _thin(cam, count, z0):
    return _place(cam, 23.5, 23.5, z0 + 1e-3 * np.arange(count), 400.0, 400.0, 0.0041)


def _walled(n, half=False, front=0):
    """A list of n entries per tile: `front` thin splats, up to three wall splats, thin splats behind."""
    cam = _cam()
    nw = min(3, n - front)
    parts = [_thin(cam, front, 3.0)] if front else []
    parts.append(_wall(cam, nw, 3.5, half))
    if n - front - nw > 0:
        parts.append(_thin(cam, n - front - nw, 4.0))
    return _cat(*parts)


def _random_scene(P=2000, seed=20):
    """Mixed: the left half of the image dense with nearly opaque splats (pixels saturate early, whole blocks go dead in the rear
    units), the right half faint (pixels blend to the end of their lists)."""
    cam = _cam()
    rng = np.random.default_rng(seed)
    u = rng.uniform(-4, W + 4, size=P)
    op = np.where(rng.uniform(size=P) < np.where(u < 26, 0.35, 0.05), rng.uniform(0.7, 0.99, size=P), rng.uniform(0.01, 0.1, size=P))
    s = rng.uniform(0.5, 4.0, size=(2, P))
    g = _place(cam, u, rng.uniform(-4, H + 4, size=P), rng.uniform(3.0, 5.0, size=P), s[0], s[1], op)
    q = rng.normal(size=(P, 4))
    g["rotations"] = (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(F32)
    return g


def _dress(g, C, seed=3):
    """colours [P, C], background [C] and dL_dpix [C, H, W] for a scene."""
    rng = np.random.default_rng(seed)
    P = len(g["means3D"])
    return dict(g, colors=rng.uniform(0.0, 1.0, size=(P, C)).astype(F32)), rng.uniform(0.0, 1.0, size=C).astype(F32), \
        rng.normal(size=(C, H, W)).astype(F32)


# ---------------------------------------------------------------- one view through the binding-level functions
def _view(g, bg, dpix, use_plan=False, fill=None, lives=("1", "0")):
    """Forward, the state it left behind, and one backward per value of GSR_BWD_LIVE.  fill: byte the binning buffer holds before."""
    import torch
    from gaustar_amd import _lib, rasterizer as rz
    lib = _lib.load()
    dev = torch.device("cuda:0")
    cam = _cam()
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x, F32)).to(dev)
    ps = {k: t(v) for k, v in g.items()}
    view, proj, campos, bg_t = t(cam.viewmatrix), t(cam.projmatrix), t(cam.campos), t(bg)
    e = torch.Tensor([])
    orig, filled = rz._view_buffers, []
    if fill is not None:
        def with_fill(*a):
            out = orig(*a)
            out[4].fill_(fill)
            filled.append(out[4].data_ptr())
            return out
        rz._view_buffers = with_fill
    before = dict(rz.PLAN_STATS)
    box = []
    try:
        R, color, radii, geom, binning, img, _maxc, nseg = rz.rasterize_gaussians_native(
            bg_t, ps["means3D"], ps["colors"], ps["opacities"], ps["scales"], ps["rotations"], 1.0, e, view, proj, cam.tanfovx,
            cam.tanfovy, H, W, e, 0, campos, False, False, need_backward=True, scratch_box=box, use_plan=use_plan)
    finally:
        rz._view_buffers = orig
    if fill is not None:
        assert filled == [binning.data_ptr()], "the view did not render into the buffer that was filled"
    P = len(g["means3D"])
    U = max(nseg, 1)
    i32 = dict(dtype=torch.int32, device=dev)
    fT, nc, rg = torch.zeros(H, W, device=dev), torch.zeros(H, W, **i32), torch.zeros(GX * GY, 2, **i32)
    info, live = torch.zeros(U, 4, **i32), torch.full((U, 4), 77, dtype=torch.uint8, device=dev)
    masks = torch.zeros(U, 4, 64, dtype=torch.int64, device=dev)
    p_ = lambda x: x.data_ptr()
    torch.cuda.synchronize(dev)
    _lib.check(lib.gsr_debug_export(P, R, U, W, H, p_(geom), None, p_(img), None, None, None, None, p_(rg), None, p_(fT), p_(nc), None), "export")
    _lib.check(lib.gsr_debug_export_masks(R, U, p_(binning), p_(masks), None), "export masks")
    _lib.check(lib.gsr_debug_export_units(R, U, p_(binning), p_(info), p_(live), None), "export units")
    torch.cuda.synchronize(dev)
    out = dict(color=color.cpu().numpy(), radii=radii.cpu().numpy(), final_T=fT.cpu().numpy(), n_contrib=nc.cpu().numpy().astype(np.int64),
               ranges=rg.cpu().numpy().astype(np.int64), info=info.cpu().numpy().astype(np.int64), live=live.cpu().numpy(),
               masks=masks.cpu().numpy().view(np.uint64), U=nseg, stats={k: rz.PLAN_STATS[k] - before[k] for k in before}, grads={})
    old = os.environ.get("GSR_BWD_LIVE")
    try:
        for i, lv in enumerate(lives):
            os.environ["GSR_BWD_LIVE"] = lv
            gr = rz.rasterize_gaussians_backward_native(bg_t, ps["means3D"], radii, ps["colors"], ps["scales"], ps["rotations"], 1.0, e, view,
                                                        proj, cam.tanfovx, cam.tanfovy, t(dpix), e, 0, campos, geom, R, binning, img, False,
                                                        num_segments=nseg, zeroed_scratch=box[0] if (box and i == 0) else None)
            torch.cuda.synchronize(dev)
            out["grads"][lv] = {k: v.cpu().numpy() for k, v in zip(HIP_ORDER, gr) if v is not None}
    finally:
        if old is None:
            os.environ.pop("GSR_BWD_LIVE", None)
        else:
            os.environ["GSR_BWD_LIVE"] = old
    return out


# ---------------------------------------------------------------- the oracle, once per scene
_ORACLE = {}


def _oracle(name, g, bg, dpix):
    """C oracle (three channels per pass): channels 3.. are a second pass over the same geometry -- geometry gradients add up, the
    colour gradients split (four channels: the scalar target rides in channel 0 of the second pass)."""
    if name in _ORACLE:
        return _ORACLE[name]
    cam = _cam()
    C = len(bg)

    def one(cols, bg3, d3):
        kw = dict(means3D=g["means3D"], opacities=g["opacities"], view=cam.viewmatrix, proj=cam.projmatrix, campos=cam.campos, W=W, H=H,
                  tanfovx=cam.tanfovx, tanfovy=cam.tanfovy, bg=bg3, shs=None, colors_precomp=cols, scales=g["scales"],
                  rotations=g["rotations"], cov3D_precomp=None, sh_degree=0, scale_modifier=1.0)
        return parity.run_oracle(kw, d3)

    st, ga = one(g["colors"][:, :3], bg[:3], dpix[:3])
    ref = dict(color=st["color"].copy(), radii=st["radii"].copy(), n_contrib=st["n_contrib"].astype(np.int64),
               **{k: np.asarray(ga[k], np.float64) for k in KEYS})
    if C > 3:
        if C == 4:
            cols, bg3, d3 = np.repeat(g["colors"][:, 3:4], 3, axis=1), np.repeat(bg[3:4], 3), np.concatenate([dpix[3:4], 0 * dpix[:2]])
        else:
            cols, bg3, d3 = g["colors"][:, 3:6], bg[3:6], dpix[3:6]
        st2, gb = one(np.ascontiguousarray(cols), bg3, np.ascontiguousarray(d3))
        for k in KEYS:
            if k != "dL_dcolors":
                ref[k] = ref[k] + np.asarray(gb[k], np.float64)
        ref["dL_dcolors"] = np.concatenate([ref["dL_dcolors"], np.asarray(gb["dL_dcolors"], np.float64)[:, :C - 3]], axis=1)
        ref["color"] = np.concatenate([ref["color"], st2["color"][:C - 3]])
    _ORACLE[name] = ref
    return ref


def _check_against_oracle(r, ref, what, same_lists=False):
    """same_lists: every Gaussian is wider than the image, so the library's tile test drops nothing and list positions are the
    oracle's -- n_contrib must then be the oracle's too (no pair on the other side of a threshold)."""
    assert np.array_equal(r["radii"], ref["radii"]), what
    if same_lists:
        assert np.array_equal(r["n_contrib"], ref["n_contrib"]), f"{what}: n_contrib differs from the oracle's in {(r['n_contrib'] != ref['n_contrib']).sum()} pixels"
    parity.check_image(r["color"], ref["color"], f"{what} color")
    for lv, gr in r["grads"].items():
        for k in KEYS:
            parity.check_grad(gr[k], ref[k].reshape(gr[k].shape), f"{what} GSR_BWD_LIVE={lv} {k}")


# ---------------------------------------------------------------- what the flags must be
def _block_pixels(tile, blk):
    """Image coordinates (ys, xs) of the block's pixels that lie inside the image, lane order."""
    ty, tx = divmod(tile, GX)
    ys = ty * 16 + (blk >> 1) * 8 + np.arange(64) // 8
    xs = tx * 16 + (blk & 1) * 8 + np.arange(64) % 8
    ok = (ys < H) & (xs < W)
    return ys, xs, ok


def _tile_units(r, tile):
    """(first unit, units the backward launches for the tile, entries) from the unit table."""
    info = r["info"][:r["U"]]
    first, end = r["ranges"][tile]
    rows = np.nonzero((info[:, 0] == tile) & (info[:, 1] == first) & (info[:, 2] == end - first))[0]
    rows = rows[info[rows, 3] == rows.min()] if len(rows) else rows       # (rows another view left behind name another first unit)
    if len(rows) == 0:
        return 0, 0, 0
    assert np.array_equal(rows, rows.min() + np.arange(len(rows)))
    return int(rows.min()), len(rows), int(end - first)


def _flags_of(r, tile):
    u0, nu, _ = _tile_units(r, tile)
    return r["live"][u0:u0 + nu].astype(np.int64)       # [unit of the tile][block]


def _inside_blocks(tile):
    return np.array([int(_block_pixels(tile, b)[2].any()) for b in range(4)])


def _sandwich(r, what, upper=True):
    """Integer-exact bounds on every flag of the view.  Upper (views whose flags are exact): a unit flagged live has a candidate bit
    below some pixel's n_contrib (`kept`, as bench.py::issue_statistics counts it).  Lower: the unit of a pixel's last contributor
    is live for its block."""
    n_live = n_kept = n_units = 0
    for tile in range(GX * GY):
        u0, nu, n = _tile_units(r, tile)
        fl = _flags_of(r, tile)
        assert set(np.unique(fl)) <= {0, 1}, f"{what}: tile {tile} has flag bytes {np.unique(fl)} (stale memory?)"
        for blk in range(4):
            ys, xs, ok = _block_pixels(tile, blk)
            nc = np.where(ok, r["n_contrib"][np.minimum(ys, H - 1), np.minimum(xs, W - 1)], 0)
            for u in range(nu):
                n_units += 1
                lim = np.clip(nc - 64 * u, 0, 64)
                below = np.where(lim >= 64, np.uint64(0xFFFFFFFFFFFFFFFF), (np.uint64(1) << lim.astype(np.uint64)) - np.uint64(1))
                if fl[u, blk]:
                    n_live += 1
                    kept = 64 * u < n and bool(((r["masks"][u0 + u, blk] & below) != 0).any())
                    if not upper:
                        n_kept += int(kept)
                        continue
                    assert kept, f"{what}: tile {tile} unit {u} block {blk} is flagged live without a candidate below any pixel's n_contrib"
                    n_kept += 1
            for u in np.unique((nc[nc > 0] - 1) >> 6):
                assert fl[u, blk] == 1, f"{what}: tile {tile} block {blk}: unit {u} holds a pixel's last contributor and is flagged dead"
    print(f"[live] {what}: (unit, block) pairs {n_units}, flagged live {n_live}, of those kept {n_kept}, dead {n_units - n_live}")
    return n_units, n_live


def _case(name, g3, C, exact=True, same_lists=True):
    g, bg, dpix = _dress(g3, C)
    r = _view(g, bg, dpix)
    _check_against_oracle(r, _oracle(name, g, bg, dpix), name, same_lists)
    r["counts"] = _sandwich(r, name, upper=exact)      # ((unit, block) pairs of the view, flagged live)
    return r


# ---------------------------------------------------------------- (a), (b): walls
@pytest.mark.parametrize("k,rr,front,C", [(0, 1, 0, 3), (1, 0, 0, 4), (1, 1, 0, 6), (3, 0, 0, 3), (1, 1, 70, 3)])
def test_opaque_wall_in_front(k, rr, front, C):
    n = front + 3 + 64 * k + rr
    r = _case(f"wall k={k} r={rr} front={front} C={C}", _walled(n, front=front), C)
    # every pixel blends the thin splats in front and then two wall splats -- one, where the thin ones have taken T to 0.75 already
    last = front + (2 if front == 0 else 1)
    stop = (last - 1) >> 6
    assert np.isin(r["n_contrib"], [last, last + 1] if front else [last]).all() and (stop == (last >> 6))
    for tile in range(GX * GY):
        fl = _flags_of(r, tile)
        assert fl.shape == ((n + 63) // 64, 4)
        want = np.outer(np.arange(len(fl)) <= stop, _inside_blocks(tile)).astype(np.int64)
        assert np.array_equal(fl, want), f"tile {tile}: flags {fl.T.tolist()} instead of {want.T.tolist()}"


@pytest.mark.parametrize("k,rr,C", [(0, 1, 3), (1, 0, 6), (1, 1, 4), (3, 0, 3)])
def test_half_covered_wall(k, rr, C):
    n = 3 + 64 * k + rr
    r = _case(f"half wall k={k} r={rr} C={C}", _walled(n, half=True), C)
    fl = _flags_of(r, MID)
    nc = r["n_contrib"][16:32, 16:32]
    assert (nc[:, :8] == 2).all() and (nc[:, 12:] == n).all()       # left blocks stop in the wall, columns 28.. blend everything
    want = np.ones((len(fl), 4), np.int64)
    want[1:, 0] = want[1:, 2] = 0
    assert np.array_equal(fl, want), f"flags {fl.T.tolist()} instead of {want.T.tolist()}"


# ---------------------------------------------------------------- (c), (d): list lengths; long and split lists
def _length_case(n, walled, C=3):
    r = _case(f"length {n} {'wall' if walled else 'thin'}", _walled(n) if walled else _thin(_cam(), n, 4.0), C, exact=n <= 2048)
    assert (r["n_contrib"] == (2 if walled and n > 2 else n)).all()      # (the wall stops every pixel at its third splat)
    for tile in range(GX * GY):
        fl = _flags_of(r, tile)
        units = (n + 63) // 64
        assert fl.shape == (units, 4)
        if n > 2048:
            want = np.ones((units, 4), np.int64)                      # no exact word: live throughout, blocks outside the image included
        elif walled:
            want = np.outer(np.arange(units) == 0, _inside_blocks(tile)).astype(np.int64)
        else:
            want = np.outer(np.ones(units, np.int64), _inside_blocks(tile))      # every pixel blends every entry: bit 31 at 2 048
        assert np.array_equal(fl, want), f"n = {n}, tile {tile}: flags {fl.T.tolist()} instead of {want.T.tolist()}"
    return r


@pytest.mark.parametrize("walled", [False, True])
@pytest.mark.parametrize("n", [1, 63, 64, 65])
def test_list_length_boundaries(n, walled):
    _length_case(n, walled)


def test_2049_entries_blended_in_parts_is_all_live():
    """In process a nine-tile view of 2 049 entries per tile SPLITS (above SPLIT_FROM and more than 1/256 of the view), so this is a
    second case of parts; the one-word limit itself is tested unsplit, in the child process below."""
    _length_case(2049, False)


def test_tile_blended_in_parts_is_all_live():
    """1 800 entries on every tile of a nine-tile view: above SPLIT_FROM (1 792) and more than 1/256 of the view's instances, so the
    view splits and every list above PART_FROM (1 024) is blended in parts (gsr_internal.h).  The wall in front would make all
    rear units dead; in parts nobody can tell."""
    n = 1800
    r = _case("parts 1800 wall", _walled(n), 3, exact=False)
    assert (r["n_contrib"] == 2).all()
    for tile in range(GX * GY):
        assert np.array_equal(_flags_of(r, tile), np.ones(((n + 63) // 64, 4), np.int64)), tile


def test_more_parts_than_one_launch_holds_is_all_live():
    """3 600 entries on each of nine tiles = 72 parts: above the 64 the forward blends inside one launch (gsr_blend_fwd.hip
    PARTS_IN_LAUNCH), so the parts run as a launch of their own and the tiles' workgroups combine them (MODE 1 + MODE 0)."""
    n = 3600
    r = _case("parts 3600 wall", _walled(n), 3, exact=False)
    assert (r["n_contrib"] == 2).all()
    for tile in range(GX * GY):
        assert np.array_equal(_flags_of(r, tile), np.ones(((n + 63) // 64, 4), np.int64)), tile


_CHILD = """
import os, sys, numpy as np
sys.path.insert(0, {tests!r}); sys.path.insert(0, {root!r})
import test_gpu_bwd_live as t
for n in (2047, 2048, 2049):
    for walled in (False, True):
        t._length_case(n, walled)
print("CHILD-OK")
"""


def test_list_lengths_2047_2048_2049_unsplit():
    """In a nine-tile image a list of 2 047 entries is more than 1/256 of the view, so the view would split (above).  Full-size
    views hold such lists unsplit (config C: up to 2 060 entries of 800 k); here GSR_SPLIT_FROM, which the library reads once per
    process, raises the threshold -- hence the child process.  2 047 and 2 048 carry exact flags (2 048 uses bit 31 of the pixels'
    word); 2 049 has a 33rd unit and no exact word: all live, with the thin list (position 2 048 would alias bit 0 and unit 32 come
    out dead) and behind the wall (every rear unit would come out dead), n_contrib and gradients as the oracle's."""
    env = dict(os.environ, GSR_SPLIT_FROM="1000000")
    code = _CHILD.format(tests=os.path.join(ROOT, "tests"), root=ROOT)
    p = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    print(p.stdout[-4000:])
    assert p.returncode == 0 and "CHILD-OK" in p.stdout, p.stdout[-3000:] + p.stderr[-3000:]


# ---------------------------------------------------------------- random scene: sandwich, gradients, stale memory, planned views
@pytest.mark.parametrize("C", [3, 4, 6])
def test_random_scene(C):
    r = _case(f"random C={C}", _random_scene(), C, same_lists=False)
    n_units, n_live = r["counts"]
    assert 0 < n_live < n_units
    assert (r["final_T"] < 1e-3).any() and (r["final_T"] > 0.1).any()      # some pixels saturate, some do not


def test_stale_memory():
    g, bg, dpix = _dress(_random_scene(), 3)
    _view(g, bg, dpix, lives=())                 # (sizes the binning buffer the later views get)
    a = _view(g, bg, dpix, fill=0xFF)
    b = _view(g, bg, dpix, fill=0x00)
    ref = _oracle("random C=3", g, bg, dpix)
    for r, what in ((a, "over 0xFF"), (b, "over 0x00")):
        _sandwich(r, what)
        _check_against_oracle(r, ref, what)
    assert a["U"] == b["U"] and np.array_equal(a["live"][:a["U"]], b["live"][:b["U"]])
    for k in ("color", "final_T", "n_contrib", "radii"):
        assert np.array_equal(a[k], b[k]), k


def test_planned_views():
    from gaustar_amd import rasterizer as rz
    full = _random_scene()
    P = len(full["means3D"])
    gf, bg, dpix = _dress(full, 3)
    gs = {k: v[:P - P // 4] for k, v in gf.items()}
    rz.drop_plans()
    try:
        first = _view(gf, bg, dpix, use_plan=None)
        second = _view(gf, bg, dpix, use_plan=None)
        third = _view(gs, bg, dpix, use_plan=None)
        exact_full, exact_fewer = _view(gf, bg, dpix), _view(gs, bg, dpix)
    finally:
        rz.drop_plans()
    assert first["stats"]["planned"] == 0 and second["stats"] == {"planned": 1, "exact": 0, "misfit": 0} and third["stats"] == second["stats"], \
        (first["stats"], second["stats"], third["stats"])
    for r, ex, g, what in ((second, exact_full, gf, "planned"), (third, exact_fewer, gs, "planned, fewer Gaussians")):
        for k in ("color", "final_T", "n_contrib", "radii"):
            assert np.array_equal(r[k], ex[k]), f"{what}: {k} differs from the exact path"
        _check_against_oracle(r, _oracle("random C=3" if g is gf else "random fewer", g, bg, dpix), what)
        _sandwich(r, what)
        # units past a list's end (the bucket's slack): dead for every block
        slack = np.zeros(r["U"], bool)
        for tile in range(GX * GY):
            u0, nu, n = _tile_units(r, tile)
            slack[u0:u0 + nu] = 64 * np.arange(nu) >= n
        assert (r["live"][:r["U"]][slack] == 0).all(), f"{what}: a slack unit is flagged live"
        print(f"[live] {what}: {int(slack.sum())} slack units of {r['U']}")
        if g is gs:
            assert slack.any()
