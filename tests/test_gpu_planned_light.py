"""Light tiles of a planned view (gsr_plan.h: capacity 0 -- empty in the plan's source view with eight empty neighbours; they
stand last in the plan's launch order and the planned forward blend fills them many to a workgroup, gsr_blend_fwd.hip).  Every
case renders tiny scenes and compares the planned render with the same scene rendered with use_plan=False: image, final_T,
n_contrib and radii bit for bit, gradients to the order of the backward's float atomics (test_gpu_planned.py's tolerance)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

LT = 16   # light tiles per workgroup (gsr_blend_fwd.hip GSR_FWD_LIGHT_TILES)
F32 = np.float32


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, F32)).to(dev)


def _camera(W, H, shift=0.0):
    """Looks down +z from 4 units away; `shift` moves the eye sideways by a hair: another camera (another plan), same picture."""
    from gaustar_amd import scene
    return scene.look_at_camera((shift, 0.0, -4.0), (shift, 0.0, 0.0), W, H, focal_px=200.0)


def _cluster(cam, box, n, seed, sigma_px=1.0, opacity=(0.2, 0.9), depth=(3.5, 4.5), sort_by_depth=False):
    """n Gaussians whose centres project into the pixel box (x0, y0, x1, y1) of `cam`, about sigma_px pixels wide."""
    from gaustar_amd import scene
    rng = np.random.default_rng(seed)
    f = cam.W / (2.0 * cam.tanfovx)
    z = rng.uniform(depth[0], depth[1], size=n)
    if sort_by_depth:
        z = np.sort(z)
    u = rng.uniform(box[0], box[2], size=n)
    v = rng.uniform(box[1], box[3], size=n)
    pv = np.stack([(u - 0.5 * (cam.W - 1)) * z / f, (v - 0.5 * (cam.H - 1)) * z / f, z, np.ones(n)], axis=1)
    world = (pv @ np.linalg.inv(np.asarray(cam.viewmatrix, np.float64)))[:, :3]     # (row vectors: view = world @ viewmatrix)
    s = (sigma_px * z / f)[:, None] * rng.uniform(0.7, 1.3, size=(n, 3))
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    op = rng.uniform(opacity[0], opacity[1], size=(n, 1))
    col = rng.uniform(0.0, 1.0, size=(n, 3))
    return scene.GaussianSet(means3D=world.astype(F32), opacities=op.astype(F32), scales=s.astype(F32), rotations=q.astype(F32),
                             colors_precomp=col.astype(F32))


def _inputs(dev, gs, cam, channels=3):
    ps = dict(means3D=_t(gs.means3D, dev), opacities=_t(gs.opacities, dev), colors=_t(gs.colors_precomp, dev),
              scales=_t(gs.scales, dev), rotations=_t(gs.rotations, dev))
    if channels == 4:
        ps["colors"] = torch.cat([ps["colors"], ps["means3D"][:, 2:3].abs()], dim=1).contiguous()
    cam_t = dict(view=_t(cam.viewmatrix, dev), proj=_t(cam.projmatrix, dev), campos=_t(cam.campos, dev))
    bg_t = _t(np.array([0.25, -0.0, 0.75, 0.5][:channels], F32), dev)      # (a negative zero: C + T bg must stay what it was)
    dpix = torch.randn(channels, cam.H, cam.W, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    return ps, cam_t, bg_t, dpix


def _view(dev, ps, cam_t, bg_t, cam, dpix=None, use_plan=None, need_backward=True):
    """One forward (+ backward) through the binding-level functions -> everything the view left behind."""
    from gaustar_amd import _lib, rasterizer as rz
    lib = _lib.load()
    e = torch.Tensor([])
    before = dict(rz.PLAN_STATS)
    box = []
    out = rz.rasterize_gaussians_native(bg_t, ps["means3D"], ps["colors"], ps["opacities"], ps["scales"], ps["rotations"], 1.0, e,
                                        cam_t["view"], cam_t["proj"], cam.tanfovx, cam.tanfovy, cam.H, cam.W, e, 0, cam_t["campos"],
                                        False, False, need_backward=need_backward, scratch_box=box, use_plan=use_plan)
    R, color, radii, geom, binning, img, _maxc, nseg = out
    delta = {k: rz.PLAN_STATS[k] - before[k] for k in before}
    P = int(ps["means3D"].shape[0])
    fT = torch.full((cam.H, cam.W), -1.0, device=dev)
    nc = torch.full((cam.H, cam.W), -1, dtype=torch.int32, device=dev)
    rg = torch.full((_tiles(cam), 2), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize(dev)
    p_ = lambda x: x.data_ptr()
    _lib.check(lib.gsr_debug_export(P, R, max(nseg, 1), cam.W, cam.H, p_(geom), None, p_(img), None, None, None, None, p_(rg), None,
                                    p_(fT), p_(nc), None), "gsr_debug_export")
    grads = None
    if dpix is not None:
        grads = rz.rasterize_gaussians_backward_native(bg_t, ps["means3D"], radii, ps["colors"], ps["scales"], ps["rotations"], 1.0, e,
                                                       cam_t["view"], cam_t["proj"], cam.tanfovx, cam.tanfovy, dpix, e, 0,
                                                       cam_t["campos"], geom, R, binning, img, False, num_segments=nseg,
                                                       zeroed_scratch=box[0] if box else None)
    torch.cuda.synchronize(dev)
    # (tile_counts: the image state's {first, first + count} per tile -- a plan's buckets lie elsewhere, the counts are the view's)
    return dict(color=color.clone(), radii=radii.clone(), final_T=fT, n_contrib=nc, tile_counts=rg[:, 1] - rg[:, 0], grads=grads,
                stats=delta)


def _same(got, want, what, gtol=2e-5):
    for k in ("color", "final_T", "n_contrib", "radii", "tile_counts"):
        assert torch.equal(got[k], want[k]), f"{what}: {k} differs in {int((got[k] != want[k]).sum())} places"
    if want["grads"] is not None and got["grads"] is not None:
        for i, (ga, gb) in enumerate(zip(got["grads"], want["grads"])):
            if ga is None or ga.numel() == 0:
                assert gb is None or gb.numel() == 0
                continue
            scale = float(gb.abs().max())
            err = float((ga - gb).abs().max())
            assert err <= gtol * scale + 1e-30, f"{what}: gradient {i} differs by {err} of max {scale}"


def _plans():
    from gaustar_amd import rasterizer as rz
    return [p.pi for p in rz._PLANS.values()]


def _light(pi):
    """Light tiles of the plan in use (include/gsr.h: gsr_plan_info::reserved1[1])."""
    return int(pi.reserved1[1])


def _tiles(cam):
    return ((cam.W + 15) // 16) * ((cam.H + 15) // 16)


def test_partial_last_group_and_clipped_edge_tiles():
    """200 x 120 = 13 x 8 tiles, the right and bottom ones clipped; a few hundred Gaussians over about three tiles in a corner,
    so that the light tiles do not fill their last workgroup.  Exact, planned, planned."""
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    cam = _camera(200, 120)
    gs = _cluster(cam, (4, 4, 40, 24), 300, seed=1)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam)
    rz.drop_plans()
    exact = _view(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False)
    assert int((exact["n_contrib"] > 0).sum()) > 100 and exact["stats"] == {"planned": 0, "exact": 0, "misfit": 0}
    first = _view(dev, ps, cam_t, bg_t, cam, dpix)
    assert first["stats"]["planned"] == 0
    _same(first, exact, "first view (exact, leaves the plan)")
    for i in range(3):
        r = _view(dev, ps, cam_t, bg_t, cam, dpix)
        assert r["stats"] == {"planned": 1, "exact": 0, "misfit": 0}, (i, r["stats"])
        _same(r, exact, f"planned view {i}")
        (pi,) = _plans()
        n_light = _light(pi)
        assert 0 < n_light < _tiles(cam) - 3 and n_light % LT != 0, n_light
        assert n_light == int(pi.reserved1[0]) or pi.pending != 0   # (the arriving plan's count: same scene, same count)


@pytest.mark.parametrize("case", ["every_tile_occupied", "one_tile_in_the_middle", "one_tile_image"])
def test_extremes(case):
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    if case == "every_tile_occupied":
        cam = _camera(96, 64)
        gs = _cluster(cam, (0, 0, 95, 63), 600, seed=2, sigma_px=2.0)
    elif case == "one_tile_in_the_middle":
        cam = _camera(200, 120)
        gs = _cluster(cam, (101, 53, 106, 58), 40, seed=3, sigma_px=0.5)       # tile (6, 3) = pixels 96..111 x 48..63
    else:
        cam = _camera(16, 16)
        gs = _cluster(cam, (2, 2, 13, 13), 50, seed=4)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam)
    rz.drop_plans()
    exact = _view(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False)
    runs = [_view(dev, ps, cam_t, bg_t, cam, dpix) for _ in range(4)]
    for i, r in enumerate(runs):
        _same(r, exact, f"{case}, view {i}")
    assert runs[0]["stats"]["planned"] == 0 and runs[-1]["stats"] == {"planned": 1, "exact": 0, "misfit": 0}, [r["stats"] for r in runs]
    (pi,) = _plans()
    T = _tiles(cam)
    if case == "one_tile_in_the_middle":
        nc = exact["n_contrib"].cpu().numpy()
        ys, xs = np.nonzero(nc)
        assert xs.min() >= 96 and xs.max() < 112 and ys.min() >= 48 and ys.max() < 64       # one occupied tile ...
        assert _light(pi) == T - 9                                                           # ... and its eight neighbours
    else:
        assert _light(pi) == 0


def test_misfit_that_dirtied_light_tiles_is_cleaned_up():
    """A view that does not fit its plan because the Gaussians moved onto tiles the plan holds light has claimed on those tiles'
    cursors.  It must be caught and rendered the exact way, and the planned views that follow on the stream -- of cameras whose
    plans hold that region under load, and of one whose plan holds it light -- must find every cursor they claim on zero."""
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    cams_a = [_camera(200, 120), _camera(200, 120, shift=2e-3)]     # (a fresh camera per round: misfits in a row pause a camera's planning)
    cam_b, cam_c = _camera(200, 120, shift=1e-3), _camera(200, 120, shift=-1e-3)
    here = _cluster(cams_a[0], (4, 4, 40, 24), 300, seed=1)             # top left
    there = _cluster(cams_a[0], (150, 90, 190, 110), 300, seed=1)       # bottom right: light under a plan of `here`
    in_b, in_c = _inputs(dev, there, cam_b), _inputs(dev, here, cam_c)
    rz.drop_plans()
    exact_of = lambda inp, cam: _view(dev, inp[0], inp[1], inp[2], cam, inp[3], use_plan=False)
    ex_b, ex_c = exact_of(in_b, cam_b), exact_of(in_c, cam_c)

    def planned(inp, cam, want, what, expect=None):
        r = _view(dev, inp[0], inp[1], inp[2], cam, inp[3])
        _same(r, want, what)
        if expect is not None:
            assert {k: r["stats"][k] for k in expect} == expect, (what, r["stats"])
        return r

    fits = {"planned": 1, "exact": 0, "misfit": 0}
    for inp, cam, want in ((in_b, cam_b, ex_b), (in_c, cam_c, ex_c)):
        for i in range(3):
            planned(inp, cam, want, "warm-up", fits if i == 2 else None)
    for round_, cam_a in enumerate(cams_a):
        in_a, moved = _inputs(dev, here, cam_a), _inputs(dev, there, cam_a)
        ex_a, ex_moved = exact_of(in_a, cam_a), exact_of(moved, cam_a)
        for i in range(3):
            planned(in_a, cam_a, ex_a, f"round {round_}: camera A plans the first scene", fits if i == 2 else None)
        planned(moved, cam_a, ex_moved, f"round {round_}: the scene moved onto light tiles", {"planned": 0, "misfit": 1})
        if round_ == 1:   # first a view whose plan holds the dirtied region LIGHT: its light workgroups hand those cursors back
            planned(in_c, cam_c, ex_c, "camera C behind the misfit", fits)
        planned(in_b, cam_b, ex_b, f"round {round_}: camera B behind the misfit", fits)
        planned(in_b, cam_b, ex_b, f"round {round_}: camera B, second view", fits)


def test_two_image_sizes_alternate_on_one_stream():
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    big, small = _camera(200, 120), _camera(96, 64)
    in_big = _inputs(dev, _cluster(big, (4, 4, 40, 24), 300, seed=1), big)
    in_small = _inputs(dev, _cluster(small, (50, 30, 90, 60), 200, seed=5), small)
    rz.drop_plans()
    ex_big = _view(dev, in_big[0], in_big[1], in_big[2], big, in_big[3], use_plan=False)
    ex_small = _view(dev, in_small[0], in_small[1], in_small[2], small, in_small[3], use_plan=False)
    n_planned = 0
    for i in range(12):
        big_turn = (i % 3) != 2          # big, big, small, big, big, small, ...
        inp, cam, want = (in_big, big, ex_big) if big_turn else (in_small, small, ex_small)
        r = _view(dev, inp[0], inp[1], inp[2], cam, inp[3])
        _same(r, want, f"alternating sizes, view {i}")
        assert r["stats"]["misfit"] == 0, (i, r["stats"])
        n_planned += r["stats"]["planned"]
    assert n_planned >= 6, n_planned
    assert len(_plans()) == 2 and all(_light(pi) > 0 for pi in _plans())


@pytest.mark.parametrize("replan", ["1", "0"])
@pytest.mark.parametrize("channels,need_backward", [(3, False), (4, True)])
def test_forward_only_and_four_channels(monkeypatch, replan, channels, need_backward):
    from gaustar_amd import rasterizer as rz
    monkeypatch.setenv("GSR_REPLAN", replan)
    dev = torch.device("cuda:0")
    cam = _camera(200, 120)
    gs = _cluster(cam, (60, 70, 100, 100), 300, seed=6)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam, channels)
    if not need_backward:
        dpix = None
    rz.drop_plans()
    exact = _view(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False, need_backward=need_backward)
    runs = [_view(dev, ps, cam_t, bg_t, cam, dpix, need_backward=need_backward) for _ in range(5)]
    for i, r in enumerate(runs):
        _same(r, exact, f"C = {channels}, backward {need_backward}, GSR_REPLAN={replan}, view {i}")
    assert [r["stats"]["planned"] for r in runs[2:]] == [1, 1, 1], [r["stats"] for r in runs]
    assert all(0 < _light(pi) < _tiles(cam) for pi in _plans())


def test_plan_whose_light_count_is_garbage_is_not_adopted():
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    cam = _camera(200, 120)
    gs = _cluster(cam, (4, 4, 40, 24), 300, seed=1)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam)
    rz.drop_plans()
    exact = _view(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False)
    first = _view(dev, ps, cam_t, bg_t, cam, dpix)
    (pi,) = _plans()
    assert first["stats"]["planned"] == 0 and pi.state == 0 and pi.pending != 0 and pi.arrived == pi.pending   # its plan has landed
    assert 0 < pi.reserved1[0] < _tiles(cam)
    pi.reserved1[0] = _tiles(cam) + 1
    second = _view(dev, ps, cam_t, bg_t, cam, dpix)
    assert second["stats"] == {"planned": 0, "exact": 1, "misfit": 0} and pi.state == 0, (second["stats"], pi.state)
    _same(second, exact, "view behind a header that is no plan")
    third = _view(dev, ps, cam_t, bg_t, cam, dpix)                # (the exact view left a plan of its own)
    assert third["stats"]["planned"] == 1 and 0 < _light(pi) < _tiles(cam)
    _same(third, exact, "view by the plan that replaced it")
