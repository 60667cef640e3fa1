"""Planned binning (include/gsr.h: gsr_forward_planned; gsr_internal.h "planned binning") against the exact path
(scan + scatter = what replaces DGR/cuda_rasterizer/rasterizer_impl.cu:277-317) on the same inputs: a camera's first view
renders the exact way and leaves a plan, its next views are binned by the plan -- no tile-offset scan, no scatter pass --
and must give the SAME images, radii and last-contributor maps bit for bit, gradients to the order of the backward's float
atomics.  A view that outgrew its plan (the Gaussians moved) must be caught before anything is blended, rendered the exact
way by the same call, and re-planned."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _t(x, dev):
    return torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)


def _scene(name, view):
    from gaustar_amd import scene
    gs, cams, bg = {"C": scene.config_C, "B": scene.config_B}[name]()
    return gs, cams[view], bg


def _render(dev, ps, cam_t, bg_t, cam, dpix=None, use_plan=None, channels=3, need_backward=True):
    """-> (image, radii, n_contrib-free outputs, grads or None, planned?) through the binding-level functions."""
    from gaustar_amd import rasterizer as rz
    e = torch.Tensor([])
    before = dict(rz.PLAN_STATS)
    box = []
    out = rz.rasterize_gaussians_native(bg_t, ps["means3D"], ps["colors"], ps["opacities"], ps["scales"], ps["rotations"], 1.0, e,
                                        cam_t["view"], cam_t["proj"], cam.tanfovx, cam.tanfovy, cam.H, cam.W, e, 0, cam_t["campos"],
                                        False, False, need_backward=need_backward, scratch_box=box, use_plan=use_plan)
    R, color, radii, geom, binning, img, _maxc, nseg = out
    after = dict(rz.PLAN_STATS)
    delta = {k: after[k] - before[k] for k in after}
    grads = None
    if dpix is not None:
        grads = rz.rasterize_gaussians_backward_native(bg_t, ps["means3D"], radii, ps["colors"], ps["scales"], ps["rotations"], 1.0, e,
                                                       cam_t["view"], cam_t["proj"], cam.tanfovx, cam.tanfovy, dpix, e, 0,
                                                       cam_t["campos"], geom, R, binning, img, False, num_segments=nseg,
                                                       zeroed_scratch=box[0] if box else None)
    torch.cuda.synchronize(dev)
    return color.clone(), radii.clone(), grads, delta, (R, nseg)


def _check_same(a, b, what, gtol=2e-5):
    assert torch.equal(a[0], b[0]), f"{what}: images differ, max {float((a[0] - b[0]).abs().max())}"
    assert torch.equal(a[1], b[1]), f"{what}: radii differ"
    if a[2] is not None:
        for i, (ga, gb) in enumerate(zip(a[2], b[2])):
            if ga is None or ga.numel() == 0:
                assert gb is None or gb.numel() == 0
                continue
            scale = float(gb.abs().max())
            err = float((ga - gb).abs().max())
            assert err <= gtol * scale + 1e-30, f"{what}: gradient {i} differs by {err} of max {scale}"


def _inputs(dev, gs, cam, bg, channels=3):
    ps = dict(means3D=_t(gs.means3D, dev), opacities=_t(gs.opacities, dev), colors=_t(gs.colors_precomp, dev),
              scales=_t(gs.scales, dev), rotations=_t(gs.rotations, dev))
    if channels == 4:
        ps["colors"] = torch.cat([ps["colors"], ps["means3D"][:, 2:3].abs()], dim=1).contiguous()
    cam_t = dict(view=_t(cam.viewmatrix, dev), proj=_t(cam.projmatrix, dev), campos=_t(cam.campos, dev))
    bg_t = _t(bg, dev) if channels == 3 else torch.cat([_t(bg, dev), torch.ones(1, device=dev)])
    dpix = torch.randn(channels, cam.H, cam.W, device=dev, generator=torch.Generator(device=dev).manual_seed(5))
    return ps, cam_t, bg_t, dpix


@pytest.mark.parametrize("view,channels", [(0, 3), (90, 3), (37, 4)])
def test_planned_view_equals_exact_view_config_c(view, channels):
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    gs, cam, bg = _scene("C", view)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam, bg, channels)
    rz.drop_plans()
    exact = _render(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False)
    assert exact[3] == {"planned": 0, "exact": 0, "misfit": 0}
    first = _render(dev, ps, cam_t, bg_t, cam, dpix)            # no plan yet: exact, leaves one (and the binning hint grows)
    assert first[3]["planned"] == 0 and first[3]["exact"] == 1
    _check_same(first, exact, "first view (exact, plans)")
    got = [_render(dev, ps, cam_t, bg_t, cam, dpix) for _ in range(3)]
    if not any(g[3]["planned"] for g in got):
        # the only legitimate reason: this view's longest list leaves no room for slack below the in-kernel sort's 2 048 entries
        assert exact[4][0] > 0
        pytest.skip("view is not plannable (longest list too close to 2 048 entries)")
    assert got[-1][3] == {"planned": 1, "exact": 0, "misfit": 0}
    assert got[-1][4][0] >= exact[4][0] and got[-1][4][1] >= exact[4][1]   # capacities, not counts
    for g in got:
        _check_same(g, exact, f"planned view {view}")
    # forward-only renders of the camera keep a plan of their own (the first one leaves it)
    fwd_only = [_render(dev, ps, cam_t, bg_t, cam, None, need_backward=False) for _ in range(2)]
    assert fwd_only[0][3]["planned"] == 0 and fwd_only[1][3]["planned"] == 1
    assert torch.equal(fwd_only[0][0], exact[0]) and torch.equal(fwd_only[1][0], exact[0])


def test_view_that_outgrew_its_plan_falls_back_and_replans():
    """Same camera, the Gaussians blown up by 1.6x and shifted after the plan was made: buckets overflow, the call must notice
    (misfit), render the exact way and leave a new plan that the next call uses; every result equals the exact path's."""
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    gs, cam, bg = _scene("C", 13)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam, bg)
    rz.drop_plans()
    _render(dev, ps, cam_t, bg_t, cam, dpix)
    _render(dev, ps, cam_t, bg_t, cam, dpix)      # (binning hint has room for the plan's capacities from here on)
    a = _render(dev, ps, cam_t, bg_t, cam, dpix)
    if not a[3]["planned"]:
        pytest.skip("view is not plannable")
    moved = dict(ps)
    moved["scales"] = (ps["scales"] * 1.6).contiguous()
    moved["means3D"] = (ps["means3D"] + torch.tensor([0.03, -0.02, 0.0], device=dev)).contiguous()
    exact = _render(dev, moved, cam_t, bg_t, cam, dpix, use_plan=False)
    b = _render(dev, moved, cam_t, bg_t, cam, dpix)
    assert b[3]["planned"] == 0 and b[3]["misfit"] == 1, b[3]
    _check_same(b, exact, "view that outgrew its plan")
    c = [_render(dev, moved, cam_t, bg_t, cam, dpix) for _ in range(2)]
    assert c[-1][3]["planned"] == 1 or exact[4][0] == 0, c[-1][3]
    for r in c:
        _check_same(r, exact, "re-planned view")
    # and back: the original scene under the moved scene's plan (fewer instances everywhere: it simply fits)
    d = _render(dev, ps, cam_t, bg_t, cam, dpix)
    _check_same(d, a, "original scene under the larger plan")


def test_drifting_scene_stays_planned():
    """Round 6: a planned view re-plans from its own tile counts (the plan job rides in every forward blend, gsr_plan.h), so a
    camera's plan is one visit old.  The Gaussians drift and grow a little between ALL visits of the camera -- far more in total
    than any one plan's slack --: every view after the second must be binned by a plan without a misfit, and equal the exact
    path's result for the same inputs."""
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    gs, cam, bg = _scene("C", 21)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam, bg)
    rz.drop_plans()
    seen = {"planned": 0, "exact": 0, "misfit": 0}
    steps = 10
    for i in range(steps):
        moved = dict(ps)
        moved["scales"] = (ps["scales"] * (1.0 + 0.015 * i)).contiguous()       # +13 % at the end: every list grows
        moved["means3D"] = (ps["means3D"] + torch.tensor([0.002 * i, -0.0015 * i, 0.0], device=dev)).contiguous()   # ~2 px per visit
        exact = _render(dev, moved, cam_t, bg_t, cam, dpix, use_plan=False)
        r = _render(dev, moved, cam_t, bg_t, cam, dpix)
        _check_same(r, exact, f"drifting scene, visit {i}")
        if i >= 2:
            for k in seen:
                seen[k] += r[3][k]
    if seen["planned"] == 0 and seen["misfit"] == 0:
        pytest.skip("view is not plannable")
    print(f"[planned] drifting scene: {seen}")
    # (visits 0 and 1 are exact: the first has no binning-size hint, the second leaves the first plan; visit 2 may still be exact
    # while the hint grows to the plan's capacities)
    assert seen["misfit"] <= 1 and seen["planned"] >= steps - 4, seen


def test_planned_views_of_two_image_sizes_alternate_on_one_stream():
    """The library's two cursor blocks are handed back zeroed tile by tile by the view that follows (gsr_api.hip Counters):
    views of a 1080p camera and of a small camera alternating on one stream must each find the block they claim on clean --
    every result equals the exact path's."""
    from gaustar_amd import rasterizer as rz, scene
    dev = torch.device("cuda:0")
    gs, cam, bg = _scene("C", 5)
    small = scene.look_at_camera((0.5, 1.6, 3.0), scene.SUBJECT_CENTER, 325, 243, focal_px=260.0)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam, bg)
    _ps, small_t, _bg, dpix_s = _inputs(dev, gs, small, bg)
    rz.drop_plans()
    ex_big = _render(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False)
    ex_small = _render(dev, ps, small_t, bg_t, small, dpix_s, use_plan=False)
    planned = 0
    for i in range(10):
        big_turn = (i % 3) != 2          # big, big, small, big, big, small, ...
        r = _render(dev, ps, cam_t if big_turn else small_t, bg_t, cam if big_turn else small, dpix if big_turn else dpix_s)
        _check_same(r, ex_big if big_turn else ex_small, f"alternating sizes, view {i}", gtol=1e-4)
        assert r[3]["misfit"] == 0, (i, r[3])
        planned += r[3]["planned"]
    assert planned >= 4, planned


def test_plans_of_many_cameras_and_small_scene():
    """A sweep over 24 cameras of the rig, three epochs: epoch 0 exact, epochs 1-2 planned wherever a plan is valid; images
    equal to the exact path's in every epoch."""
    from gaustar_amd import rasterizer as rz, scene
    dev = torch.device("cuda:0")
    gs, cams, bg = scene.config_C()
    ps = dict(means3D=_t(gs.means3D, dev), opacities=_t(gs.opacities, dev), colors=_t(gs.colors_precomp, dev),
              scales=_t(gs.scales, dev), rotations=_t(gs.rotations, dev))
    bg_t = _t(bg, dev)
    views = list(range(0, 160, 7))
    cam_ts = {v: dict(view=_t(cams[v].viewmatrix, dev), proj=_t(cams[v].projmatrix, dev), campos=_t(cams[v].campos, dev)) for v in views}
    rz.drop_plans()
    ref = {v: _render(dev, ps, cam_ts[v], bg_t, cams[v], None, use_plan=False, need_backward=False)[0] for v in views}
    planned = 0
    for epoch in range(3):
        for v in views:
            r = _render(dev, ps, cam_ts[v], bg_t, cams[v], None, need_backward=False)
            assert torch.equal(r[0], ref[v]), (epoch, v)
            if epoch == 0:
                assert r[3]["planned"] == 0
            planned += r[3]["planned"]
            assert r[3]["misfit"] == 0
    assert planned >= len(views), planned     # most cameras of the rig are plannable, each for two epochs


def test_giant_splats_under_a_plan_do_not_corrupt_anything():
    """Config C under use_solid_surface-like scales (sugar_model.py:1230-1232; bench.py's C_solid): a few splats cover thousands
    of tiles, workgroups run out of table slots and record space.  Round 5 found the planned preprocess acting on records it
    had never written for instances without a table slot (a wild store); every such view must come out as the exact path's."""
    from gaustar_amd import rasterizer as rz, scene
    dev = torch.device("cuda:0")
    gs, cams, bg = scene.config_C()
    cam = cams[0]
    sc = np.array(gs.scales, dtype=np.float32, copy=True)
    sc[:, 1:] *= np.exp(np.random.default_rng(7).normal(0.0, 1.0, size=(gs.P, 1))).astype(np.float32)
    sc[:, 1:] = np.maximum(sc[:, 1:].mean(), sc[:, 1:])
    gs.scales = sc
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam, bg)
    rz.drop_plans()
    exact = _render(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False)
    # (a giant splat's gradient is a float-atomic sum over tens of thousands of pixels: two runs of the SAME path differ by the
    # order of those additions -- that spread, measured here, is the yardstick; images and radii must be equal outright)
    # (tests/devtools/stress_giant.py: 150 exact renders spread up to 1.5e-2 of the largest scale gradient; one pair of runs as the
    # yardstick let the test fail once in five runs of the whole suite -- four pairs, and a wider factor)
    noise = 0.0
    for _ in range(4):
        again = _render(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False)
        noise = max(noise, max(float((ga - gb).abs().max() / gb.abs().max()) for ga, gb in zip(again[2], exact[2]) if ga is not None and ga.numel()))
    seen = {"planned": 0, "exact": 0, "misfit": 0}
    for _ in range(6):
        r = _render(dev, ps, cam_t, bg_t, cam, dpix)
        for k in seen:
            seen[k] += r[3][k]
        _check_same(r, exact, "giant splats", gtol=max(2e-5, 16.0 * noise))
    assert seen["planned"] + seen["misfit"] >= 1, seen    # a plan was tried at least once


@pytest.mark.parametrize("name", ["sh3_random", "cov3d_precomp", "mesh_sphere", "edge_cases", "depth_color_bg10"])
def test_golden_cases_under_a_plan(name):
    """The golden cases of tests/golden (outputs of the reference's own kernels) rendered three times with the same camera
    tensors: the third render is binned by the plan the first left (where the case is plannable) and must still match the
    golden image / radii / gradients as strictly as the first -- in-kernel SH, precomputed covariances, edge cases included."""
    import parity
    from gaustar_amd import rasterizer as rz
    kw, d = parity.load_golden(name)
    rz.drop_plans()
    dev = torch.device("cuda:0")
    t = lambda x: None if x is None else torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(dev)
    e = torch.Tensor([])
    opt = lambda k: t(kw[k]) if kw.get(k) is not None else e
    fixed = dict(bg=t(kw["bg"]), view=t(kw["view"]), proj=t(kw["proj"]), campos=t(kw["campos"]))
    args = dict(means3D=t(kw["means3D"]), colors=opt("colors_precomp"), op=t(kw["opacities"]), scales=opt("scales"), rot=opt("rotations"),
                cov=opt("cov3D_precomp"), shs=opt("shs"))
    dpix = t(d["in_dL_dpix"])
    outs, planned = [], 0
    for _ in range(4):
        before = dict(rz.PLAN_STATS)
        o = rz.rasterize_gaussians_native(fixed["bg"], args["means3D"], args["colors"], args["op"], args["scales"], args["rot"],
                                          kw["scale_modifier"], args["cov"], fixed["view"], fixed["proj"], kw["tanfovx"], kw["tanfovy"],
                                          kw["H"], kw["W"], args["shs"], kw["sh_degree"], fixed["campos"], False, False)
        g = rz.rasterize_gaussians_backward_native(fixed["bg"], args["means3D"], o[2], args["colors"], args["scales"], args["rot"],
                                                   kw["scale_modifier"], args["cov"], fixed["view"], fixed["proj"], kw["tanfovx"],
                                                   kw["tanfovy"], dpix, args["shs"], kw["sh_degree"], fixed["campos"], o[3], o[0], o[4], o[5],
                                                   False, num_segments=o[7])
        torch.cuda.synchronize()
        planned += rz.PLAN_STATS["planned"] - before["planned"]
        outs.append((o[1].clone(), o[2].clone(), [None if x is None else x.clone() for x in g]))
    first, last = outs[0], outs[-1]
    assert torch.equal(first[0], last[0]) and torch.equal(first[1], last[1]), name
    for ga, gb in zip(first[2], last[2]):
        if ga is None or ga.numel() == 0:
            continue
        assert float((ga - gb).abs().max()) <= 2e-5 * float(gb.abs().max()) + 1e-30, name
    parity.check_image(last[0].cpu().numpy(), d["out_color"], f"{name} under a plan")
    assert planned >= 1 or name in ("edge_cases",), (name, planned)


@pytest.mark.parametrize("W,H,focal", [(325, 243, 260.0), (3840, 2160, 2400.0), (1000, 16, 300.0)])
def test_plans_at_odd_and_large_image_sizes(W, H, focal):
    """Image sizes that are not whole tiles, one of a single tile row, and one above 8 192 tiles (the plan builder's counts no
    longer fit its LDS staging, tile_scan's counts no longer fit registers): exact, exact + plan, planned -- same results."""
    from gaustar_amd import rasterizer as rz, scene
    dev = torch.device("cuda:0")
    v, f = scene.icosphere(4, scene.SUBJECT_RADIUS, scene.SUBJECT_CENTER)
    gs = scene.mesh_bound_gaussians(v, f, np.random.default_rng(0), 3.5e-6)
    cam = scene.look_at_camera((0.5, 1.6, 3.0), scene.SUBJECT_CENTER, W, H, focal_px=focal)
    bg = np.array([0.0, 1.0, 0.0], np.float32)
    ps, cam_t, bg_t, dpix = _inputs(dev, gs, cam, bg)
    rz.drop_plans()
    exact = _render(dev, ps, cam_t, bg_t, cam, dpix, use_plan=False)
    runs = [_render(dev, ps, cam_t, bg_t, cam, dpix) for _ in range(4)]
    for r in runs:
        _check_same(r, exact, f"{W}x{H}", gtol=1e-4)
    assert runs[0][3]["planned"] == 0
    print(f"[planned] {W}x{H}: R {exact[4][0]}, paths {[r[3] for r in runs]}")
    # (the 4K view of this small scene has lists above 2 048 entries: unplannable; the other two are planned from the third view on)
    if W < 3000:
        assert sum(r[3]["planned"] for r in runs) >= 1, [r[3] for r in runs]


def _reference_caller_settings(cam, bg_t, dev):
    """GaussianRasterizationSettings built the way the reference's mesh-bound caller builds them on EVERY render call
    (gaustar_scene/sugar_model.py:1149-1187): a fresh `torch.Tensor(getWorld2View(R, t)).transpose(0, 1).cuda()` (a strided,
    non-contiguous view), a fresh projection, their product by bmm, a fresh camera centre -- nothing persists between calls."""
    import math
    from gaustar_amd import GaussianRasterizationSettings, scene
    w2v = np.ascontiguousarray(np.asarray(cam.viewmatrix, np.float32).T)     # = getWorld2View(R, t) (graphics_utils.py:38-51)
    world_view_transform = torch.Tensor(w2v).transpose(0, 1).cuda()          # sugar_model.py:1149-1150
    fovx, fovy = 2.0 * math.atan(cam.tanfovx), 2.0 * math.atan(cam.tanfovy)
    proj_transform = torch.from_numpy(scene.get_projection_matrix(1e-4, 100.0, fovx, fovy)).transpose(0, 1).cuda()   # :1154-1158
    full_proj_transform = (world_view_transform.unsqueeze(0).bmm(proj_transform.unsqueeze(0))).squeeze(0)          # :1163
    camera_center = torch.Tensor(np.asarray(cam.campos, np.float32)[None]).cuda()                                 # [1, 3] like p3d's
    return GaussianRasterizationSettings(image_height=int(cam.H), image_width=int(cam.W), tanfovx=np.float32(cam.tanfovx),
                                         tanfovy=np.float32(cam.tanfovy), bg=bg_t, scale_modifier=1., viewmatrix=world_view_transform,
                                         projmatrix=full_proj_transform, sh_degree=0, campos=camera_center, prefiltered=False,
                                         debug=False)


def test_plans_find_their_camera_behind_the_reference_caller():
    """VERDICT r5 task 1.  40 cameras of the rig, three epochs in a fresh random order each, every call building its settings as
    sugar_model.py:1149-1187 does (fresh tensors, dropped after backward): epoch 0 renders the exact way and leaves the plans,
    epochs 1-2 must be binned by them (the plannable cameras: >= 90 %), no view may misfit (the scene is static), and every image
    is the exact path's bit for bit.  Under round 5's key (the address of the view-matrix tensor) consecutive cameras shared
    one recycled block and camera B ran against camera A's plan."""
    from gaustar_amd import GaussianRasterizer, rasterizer as rz, scene
    dev = torch.device("cuda:0")
    gs, cams, bg = scene.config_C()
    views = list(range(0, 160, 4))
    ps = dict(means3D=_t(gs.means3D, dev), opacities=_t(gs.opacities, dev), colors=_t(gs.colors_precomp, dev),
              scales=_t(gs.scales, dev), rotations=_t(gs.rotations, dev))
    for p in ps.values():
        p.requires_grad_(True)
    means2D = torch.zeros(gs.P, 3, device=dev, requires_grad=True)
    bg_t = _t(bg, dev)
    dpix = torch.randn(3, cams[0].H, cams[0].W, device=dev, generator=torch.Generator(device=dev).manual_seed(11))

    def render(v):
        for p in ps.values():
            p.grad = None
        means2D.grad = None
        rasterizer = GaussianRasterizer(raster_settings=_reference_caller_settings(cams[v], bg_t, dev))
        image, radii = rasterizer(means3D=ps["means3D"], means2D=means2D, opacities=ps["opacities"], colors_precomp=ps["colors"],
                                  scales=ps["scales"], rotations=ps["rotations"])
        image.backward(dpix)
        out = image.detach().clone(), ps["means3D"].grad.clone()
        del rasterizer, image, radii
        return out

    rz.drop_plans()
    was = rz._PLANNED
    rz._PLANNED = False
    try:
        ref = {v: render(v) for v in views}
    finally:
        rz._PLANNED = was
    rng = np.random.default_rng(3)
    keys0 = dict(rz.CAMERA_KEY_STATS)
    per_epoch = []
    for epoch in range(3):
        before = dict(rz.PLAN_STATS)
        for v in rng.permutation(views):
            img, g = render(int(v))
            assert torch.equal(img, ref[int(v)][0]), (epoch, int(v))
            scale = float(ref[int(v)][1].abs().max())
            assert float((g - ref[int(v)][1]).abs().max()) <= 2e-5 * scale, (epoch, int(v))
        per_epoch.append({k: rz.PLAN_STATS[k] - before[k] for k in before})
    print(f"[reference caller] per epoch {per_epoch}; keys {({k: rz.CAMERA_KEY_STATS[k] - keys0[k] for k in keys0})}")
    assert per_epoch[0]["planned"] == 0 and per_epoch[0]["exact"] == len(views), per_epoch
    for e in (1, 2):
        assert per_epoch[e]["misfit"] == 0, per_epoch
        assert per_epoch[e]["planned"] >= 0.9 * len(views), per_epoch
    # every call brought a tensor never seen before: each was read (no address, no object identity involved)
    assert rz.CAMERA_KEY_STATS["read"] - keys0["read"] == 3 * len(views)


def test_camera_key_is_a_function_of_the_contents():
    """gsr_camera_key: the same sixteen floats give the same key wherever they lie (contiguous, transposed view, another
    allocation), different cameras give different keys, and a tensor seen before is not read again until it is written to."""
    from gaustar_amd import _lib, rasterizer as rz, scene
    dev = torch.device("cuda:0")
    lib = _lib.load()
    _gs, cams, _bg = scene.config_C()
    keys = set()
    for c in cams:
        a = _t(c.viewmatrix, dev)
        b = torch.Tensor(np.ascontiguousarray(np.asarray(c.viewmatrix, np.float32).T)).transpose(0, 1).cuda()
        assert not b.is_contiguous() and torch.equal(a, b)
        ka, kb = rz._camera_key(lib, a, dev), rz._camera_key(lib, b, dev)
        assert ka == kb and isinstance(ka, int)
        keys.add(ka)
    assert len(keys) == len(cams)
    a = _t(cams[0].viewmatrix, dev)
    s0 = dict(rz.CAMERA_KEY_STATS)
    k0 = rz._camera_key(lib, a, dev)
    k1 = rz._camera_key(lib, a, dev)
    assert k0 == k1 and rz.CAMERA_KEY_STATS["read"] - s0["read"] == 1 and rz.CAMERA_KEY_STATS["known_tensor"] - s0["known_tensor"] == 1
    a.copy_(_t(cams[1].viewmatrix, dev))     # written in place: the version counter moves, the contents are read again
    k2 = rz._camera_key(lib, a, dev)
    assert k2 != k0 and k2 == rz._camera_key(lib, _t(cams[1].viewmatrix, dev), dev)


def test_plan_info_fields_name_what_the_library_does():
    """The smallest view a plan exists for -- 64 x 64 pixels = 16 tiles, 500 Gaussians -- three times on one stream: the fields of
    the plan_info block (_lib.PlanInfo, include/gsr.h gsr_plan_info) hold what the calls return and what the device wrote."""
    from gaustar_amd import _lib, scene
    from gaustar_amd import rasterizer as rz
    dev = torch.device("cuda:0")
    gs = scene.random_gaussians(500, np.random.default_rng(3))
    cam = scene.look_at_camera((0.0, 0.0, -4.0), (0.0, 0.0, 0.0), 64, 64, fovx=0.9, znear=0.01)
    ps, cam_t, bg_t, _ = _inputs(dev, gs, cam, np.zeros(3, np.float32))
    e = torch.Tensor([])

    def view(**kw):
        before = rz.PLAN_STATS["planned"]
        out = rz.rasterize_gaussians_native(bg_t, ps["means3D"], ps["colors"], ps["opacities"], ps["scales"], ps["rotations"], 1.0, e,
                                            cam_t["view"], cam_t["proj"], cam.tanfovx, cam.tanfovy, cam.H, cam.W, e, 0, cam_t["campos"],
                                            False, False, **kw)
        torch.cuda.synchronize(dev)
        return out, rz.PLAN_STATS["planned"] - before

    rz.drop_plans()
    # (not a view of the camera's plan: it gives the device a binning hint -- without one a first view leaves stage 2, and with it
    # the plan, to the caller)
    view(use_plan=False)
    assert not rz._PLANS
    first, planned = view()
    assert planned == 0 and len(rz._PLANS) == 1
    pi = next(iter(rz._PLANS.values())).pi
    assert first[0] > 0 and pi.state == 0 and pi.pending != 0 and pi.arrived == pi.pending   # exact, and its plan has landed
    for _ in range(2):
        (R, color, _radii, _geom, _bin, _img, maxc, nseg), planned = view()
        assert planned == 1 and pi.state == 1
        assert (R, nseg, maxc) == (pi.R_cap, pi.U_cap, pi.max_cap)
        assert pi.U_cap * 64 == pi.R_cap >= first[0]
        assert pi.header[_lib.PH_T] == pi.header[1] == 16
        assert pi.arrived == pi.pending or pi.pending == 0
        assert torch.equal(color, first[1])
