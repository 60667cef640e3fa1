"""Plane-sweep stereo without a GPU: the numpy restatement tests/stereo_ref.py against a per-pixel statement of the rules, the
host-side rules of gaustar_amd.stereo (source selection, relative pose), every argument check of the module and of the C entry
points (the library is loaded, nothing is launched), and the quality the GPU tests then ask of the kernels, checked here on
the restatement first."""
import ctypes

import numpy as np
import pytest

import hull_ref as hr
import stereo_ref as sr


# ------------------------------------------------------------------------------------------------ restatement vs. the rules
@pytest.fixture(scope="module")
def tiny():
    """Three neighbouring cameras of the scene's arc at 12 x 9, the sphere 8 pixels across: (rig, images, priors)."""
    _plain, dented, faces = sr.meshes()
    H, W = 9, 12
    rig = hr.look_at_rig(sr.eyes()[3:6], (0.0, 0.0, 0.0), H, W, 30.0)
    images, priors = [], []
    for i in range(3):
        img, depth, _mask = sr.render_view(dented, faces, rig["extrinsics"][i], *sr.reference_camera(rig, i), H, W)
        images.append(img), priors.append(depth)
    return rig, images, priors


@pytest.mark.parametrize("radius", [1, 2])
def test_restated_sweep_and_consistency_equal_the_per_pixel_statement(tiny, radius):
    rig, images, priors = tiny
    cfg = sr.scene_config(radius=radius, min_var=1.0, min_score=0.3, min_sources=1, min_consistent=1)
    views, brute = [], []
    for r in range(3):
        srcs = [s for s in range(3) if s != r]
        rows = sr.source_rows(rig, r, srcs, [images[s] for s in srcs])
        c = cfg.resolved(2)
        views.append(sr.sweep(images[r], priors[r], sr.reference_camera(rig, r), rows, c))
        brute.append(sr.sweep_brute(images[r], priors[r], sr.reference_camera(rig, r), rows, c))
        for name in ("depth", "score", "state", "plane"):
            assert views[r][name].dtype == brute[r][name].dtype and views[r][name].tobytes() == brute[r][name].tobytes(), (r, name)
    assert set(np.unique(views[1]["state"])) == {0, 1, 2, 3}          # the case holds every state the sweep can give
    covered, k_lo, k_hi = sr.bands(priors[1], cfg)
    has = views[1]["plane"] >= 0
    assert (views[1]["plane"][has] >= k_lo[has]).all() and (views[1]["plane"][has] <= k_hi[has]).all() and covered[has].all()
    n4 = 0
    for r in range(3):
        srcs = [s for s in range(3) if s != r]
        rows = sr.source_rows(rig, r, srcs, [views[s]["depth"] for s in srcs], [views[s]["state"] for s in srcs])
        for tol, need in ((0.008, 1), (0.008, 2), (0.05, 2)):
            a = sr.consistency(sr.reference_camera(rig, r), views[r]["depth"], views[r]["state"], rows, tol, need)
            b = sr.consistency_brute(sr.reference_camera(rig, r), views[r]["depth"], views[r]["state"], rows, tol, need)
            assert a.dtype == np.uint8 and np.array_equal(a, b), (r, tol, need)
            assert np.array_equal(a[views[r]["state"] != 3], views[r]["state"][views[r]["state"] != 3])
            n4 += int((a == 4).sum())
    assert n4 > 0


def test_restated_luma_and_merge_rules():
    rgb = np.array([[[0, 0, 0], [255, 255, 255], [255, 0, 0], [0, 255, 0], [0, 0, 255], [1, 2, 3]]], np.uint8)
    assert sr.luma(rgb).tolist() == [[0, 255, 77, 149, 29, (77 + 300 + 87 + 128) >> 8]]
    z = np.zeros((16, 16, 16), np.float32)
    th, wh, ts, ws = z + np.float32(-0.5), z + 1, z + np.float32(0.25), z + 3
    cs = np.stack([z + 10, z + 20, z + 30])
    t, w, c, touched = sr.merge(th, wh, ts, ws, cs, 3.0)
    assert (t == 0.25).all() and (w == 1).all() and (c[1] == 20).all() and touched.all()
    assert (sr.merge(th, wh, ts, z + 2, cs, 3.0)[0] == -0.5).all()                      # below min_weight: the hull stays
    assert (sr.merge(th, z, ts, ws, cs, 3.0)[0] == -0.5).all() and not sr.merge(th, z, ts, ws, cs, 3.0)[3].any()
    assert (sr.merge(z + np.float32(0.5), wh, ts, ws, cs, 3.0)[0] == 0.5).all()         # stereo only carves
    assert (sr.merge(th, wh, ts, z, cs, 3.0)[2] == 0).all()


# ------------------------------------------------------------------------------------------------ host rules
def _arc_rig(azimuths_deg, dist=2.0):
    eyes = [dist * np.array([np.cos(np.radians(a)), 0.0, np.sin(np.radians(a))]) for a in azimuths_deg]
    return hr.look_at_rig(eyes, (0.0, 0.0, 0.0), 45, 67, 200.0)


def test_select_sources_order_ties_padding_and_limits():
    from gaustar_amd import stereo
    # camera 2 is camera 1 again (the same angle to the last bit: the tie goes to the smaller index); 5 is 3 degrees off
    # camera 0 (below the minimum), 4 is 50 degrees off (above the maximum)
    rig = _arc_rig([0.0, 10.0, 10.0, 20.0, 50.0, 3.0])
    src = stereo.select_sources(rig, 4, focus=(0.0, 0.0, 0.0))
    assert src.dtype == np.int32 and src.shape == (6, 4)
    assert src[0].tolist() == [1, 2, 3, -1]
    assert src[3].tolist() == [1, 2, 5, 0]             # 10, 10, 17, 20 degrees; 30 (camera 4) is the fifth
    assert src[4].tolist() == [3, 1, 2, -1]            # 30, 40, 40; 47 and 50 are beyond the maximum
    assert stereo.select_sources(rig, 2, focus=(0.0, 0.0, 0.0))[3].tolist() == [1, 2]
    assert stereo.select_sources(rig, 3, 5.0, 12.0, focus=(0.0, 0.0, 0.0))[0].tolist() == [1, 2, -1]
    ring = hr.look_at_rig(hr.ring_eyes(12, 3.0, (0.0,)), (0.0, 0.0, 0.0), 45, 67, 200.0)      # 30 degrees apart
    got = stereo.select_sources(ring, 4)                   # the focus from hull.rig_box: the ring's centre
    for r in range(12):
        assert sorted(int(s) for s in got[r][:2]) == sorted([(r - 1) % 12, (r + 1) % 12]) and (got[r][2:] == -1).all(), r
    for bad in (dict(n_sources=0), dict(n_sources=9), dict(min_angle_deg=30.0, max_angle_deg=20.0)):
        with pytest.raises(ValueError):
            stereo.select_sources(rig, **bad)


def test_relative_pose_against_linalg_within_4_ulp():
    """Each element is three products and two adds against numpy's own order: both are within 2 ulp of the exact value at the
    scale of the largest term, so they differ by at most 4 ulp of that scale -- 1 for a rotation's elements, the largest of
    |t_s| and |R_sr| |t_r| for the translation's.  The restatement's table has the same bits as the module's."""
    from gaustar_amd import stereo
    rig = hr.concat_rigs(hr.ring_rig(5), hr.edge_rig())
    C = len(rig["shape"])
    for r in range(C):
        for s in range(C):
            R, t = stereo.relative_pose(rig, r, s)
            rR, rt = sr.relative_pose(rig["extrinsics"][r], rig["extrinsics"][s])
            assert R.tobytes() == rR.tobytes() and t.tobytes() == rt.tobytes()
            Er, Es = rig["extrinsics"][r], rig["extrinsics"][s]
            want_R = Es[:3, :3] @ Er[:3, :3].T
            want_t = Es[:3, 3] - want_R @ Er[:3, 3]
            assert np.abs(R - want_R).max() <= 4 * np.spacing(1.0)
            scale = max(np.abs(Es[:3, 3]).max(), (np.abs(want_R) @ np.abs(Er[:3, 3])).max())
            assert np.abs(t - want_t).max() <= 4 * np.spacing(scale)
    R, t = stereo.relative_pose(rig, 2, 2)
    assert np.abs(R - np.eye(3)).max() < 1e-15 and np.abs(t).max() < 1e-14


# ------------------------------------------------------------------------------------------------ argument checks
def test_config_checks_raise():
    from gaustar_amd import stereo
    ok = stereo.StereoConfig().resolved(4)
    assert ok.keep == 2 and ok.tol == 0.008 and stereo.StereoConfig(min_sources=1, min_consistent=1).resolved(1).keep == 1 and stereo.StereoConfig().resolved(8).keep == 4
    for S in (0, 9):
        with pytest.raises(ValueError):
            stereo.StereoConfig().resolved(S)
    bad = [dict(step=0.0), dict(step=-1.0), dict(step=float("nan")), dict(near=-0.1), dict(far=-0.1), dict(far=17.0),       # 4250 planes
           dict(step=0.001), dict(background=0.005), dict(radius=0), dict(radius=4), dict(min_var=0.0), dict(min_sources=0),
           dict(min_sources=5), dict(keep=0), dict(keep=5), dict(tol=0.0), dict(min_consistent=0), dict(min_consistent=5),
           dict(min_score=float("inf"))]
    for kw in bad:
        with pytest.raises(ValueError):
            stereo.StereoConfig(**kw).resolved(4)
    # the largest k_hi must fit int16: floor((50 + 0.12) / 0.004) = 12 530 does; a background of 131.1 at that step does not
    stereo.StereoConfig(background=130.9).resolved(4)
    with pytest.raises(ValueError, match="int16"):
        stereo.StereoConfig(background=131.1).resolved(4)


def test_host_argument_checks_raise():
    import torch

    from gaustar_amd import fusion, stereo
    with pytest.raises(ValueError):
        stereo.luma(np.zeros((8, 8, 3), np.float32))
    with pytest.raises(ValueError):
        stereo.luma(np.zeros((8, 8, 4), np.uint8))
    with pytest.raises(ValueError):
        stereo.luma(np.zeros((8,), np.uint8))
    with pytest.raises(ValueError):
        stereo.luma(torch.zeros(8, 8, 3, dtype=torch.uint8))                 # a CPU tensor: the wrong device
    rig = hr.ring_rig(3)
    H, W = 96, 128
    cpu = [torch.zeros(H, W, dtype=torch.uint8)] * 3
    prior = torch.zeros(H, W)
    for row in ([3, -1], [-2, 1], [0, 1], [-1, -1], [1, 2, 1, 2, 1, 2, 1, 2, 1], [[1, 2]], [1.0, 2.0]):
        with pytest.raises(ValueError):
            stereo.sweep_view(rig, 0, np.array(row), cpu, prior)
    with pytest.raises(ValueError):
        stereo.sweep_view(rig, 3, np.array([1, 2]), cpu, prior)
    with pytest.raises(ValueError, match="GPU"):
        stereo.sweep_view(rig, 0, np.array([1, 2]), cpu, prior)              # everything right but the device
    with pytest.raises(ValueError):
        stereo.sweep_view(rig, 0, np.array([1, 2]), [torch.zeros(H, W)] * 3, prior)
    with pytest.raises(ValueError):
        stereo.sweep_view(rig, 0, np.array([1, 2]), [torch.zeros(H, W + 1, dtype=torch.uint8)] * 3, prior)
    with pytest.raises(ValueError):
        stereo.sweep_view(rig, 0, np.array([1, 2]), [None] * 3, prior)
    with pytest.raises(ValueError):
        stereo.sweep_view(rig, 0, np.array([1, 2]), cpu, prior, stereo.StereoConfig(min_sources=3))
    images, priors = [np.zeros((H, W), np.uint8)] * 3, [np.zeros((H, W), np.float32)] * 3
    with pytest.raises(ValueError):
        stereo.sweep_rig(rig, images[:2], priors)
    with pytest.raises(ValueError):
        stereo.sweep_rig(rig, images, [p.astype(np.float64) for p in priors])
    with pytest.raises(ValueError):
        stereo.sweep_rig(rig, images, priors, np.array([[1, 2], [0, 2]]))
    with pytest.raises(ValueError):
        stereo.sweep_rig(rig, images, priors, np.array([[1, 2], [0, 2], [2, 0]]))        # camera 2 is its own source
    with pytest.raises(ValueError):
        stereo.sweep_rig(rig, images, priors, np.array([[1, 2], [0, 2], [0, 1]]), stereo.StereoConfig(radius=5))
    with pytest.raises(ValueError):
        stereo.check_consistency(rig, [], np.array([[1, 2], [0, 2], [0, 1]]))
    a = fusion.TSDFVolume(np.full(3, -0.1), np.full(3, 0.1), 0.008, 0.02, "cpu")
    b = fusion.TSDFVolume(np.full(3, -0.1), np.full(3, 0.3), 0.008, 0.02, "cpu")
    c = fusion.TSDFVolume(np.full(3, -0.1), np.full(3, 0.1), 0.008, 0.03, "cpu")
    for x, y, mw in ((a, b, 3.0), (a, c, 3.0), (a, object(), 3.0), (object(), a, 3.0), (a, a, 0.0), (a, a, float("nan"))):
        with pytest.raises(ValueError):
            stereo.merge_volumes(x, y, mw)
    with pytest.raises(ValueError):
        stereo.refine_hull(rig, images, images, taubin_iterations=-1)


def test_entry_points_check_their_arguments_before_any_launch(hip_lib):
    from gaustar_amd import stereo
    assert hip_lib.gsr_stereo_camera_bytes() == stereo.CAMERA_DTYPE.itemsize == 152
    buf = (ctypes.c_char * 96)()
    base = ctypes.addressof(buf) + (-ctypes.addressof(buf)) % 16
    p = ctypes.c_void_p(base)
    err = lambda: hip_lib.gsr_last_error()
    assert hip_lib.gsr_stereo_luma(0, 8, p, p, None) != 0 and b"positive" in err()
    assert hip_lib.gsr_stereo_luma(8, 8, None, p, None) != 0 and b"null" in err()
    assert hip_lib.gsr_stereo_luma(40000, 40000, p, p, None) != 0 and b"too large" in err()
    ref = (ctypes.c_double * 4)(100.0, 100.0, 4.0, 4.0)
    table = np.zeros(2, stereo.CAMERA_DTYPE)
    for k in range(2):
        table[k] = (np.eye(3).reshape(-1), np.zeros(3), 100.0, 100.0, 4.0, 4.0, base, base, 8, 8)
    good = [0.004, 0.008, 0.12, 50.0, 4.0, 0.6]
    par = lambda **kw: (ctypes.c_double * 6)(*[kw.get(n, v) for n, v in zip(("step", "near", "far", "background", "min_var", "min_score"), good)])

    def sweep(H=8, W=8, luma=p, prior=p, ref=ref, S=2, host=None, cams=p, params=None, R=3, mins=2, keep=1, depth=p, plane=p):
        return hip_lib.gsr_stereo_sweep(H, W, luma, prior, ref, S, ctypes.c_void_p(table.ctypes.data) if host is None else host, cams,
                                        par() if params is None else params, R, mins, keep, depth, p, p, plane, None)

    assert sweep(H=1) != 0 and b"2 x 2" in err()
    assert sweep(ref=None) != 0 and b"null" in err()
    assert sweep(ref=(ctypes.c_double * 4)(0.0, 100.0, 4.0, 4.0)) != 0 and b"focal" in err()
    assert sweep(S=0) != 0 and b"n_sources" in err()
    assert sweep(S=9) != 0 and b"n_sources" in err()
    assert sweep(R=0) != 0 and b"radius" in err()
    assert sweep(R=4) != 0 and b"radius" in err()
    assert sweep(params=par(step=0.0)) != 0 and b"step" in err()
    assert sweep(params=par(step=float("nan"))) != 0 and b"finite" in err()
    assert sweep(params=par(near=-1.0)) != 0 and b"near" in err()
    assert sweep(params=par(far=17.0)) != 0 and b"4096" in err()
    assert sweep(params=par(background=131.1)) != 0 and b"int16" in err()
    assert sweep(params=par(background=0.005)) != 0 and b"background" in err()
    assert sweep(params=par(min_var=0.0)) != 0 and b"min_var" in err()
    assert sweep(mins=0) != 0 and b"min_sources" in err()
    assert sweep(mins=3) != 0 and b"min_sources" in err()
    assert sweep(keep=0) != 0 and b"keep" in err()
    assert sweep(keep=3) != 0 and b"keep" in err()
    assert sweep(luma=None) != 0 and b"null" in err()
    assert sweep(depth=None) != 0 and b"null" in err()
    assert sweep(cams=None) != 0 and b"null" in err()
    assert sweep(prior=ctypes.c_void_p(base + 2)) != 0 and b"aligned" in err()
    assert sweep(plane=ctypes.c_void_p(base + 1)) != 0 and b"aligned" in err()
    assert sweep(cams=ctypes.c_void_p(base + 4)) != 0 and b"8-byte" in err()
    for field, value, word in (("W", 1, b"2 x 2"), ("fx", 0.0, b"focal"), ("image", 0, b"null"), ("cy", np.nan, b"finite"),
                               ("R", np.full(9, np.inf), b"finite")):
        bad = table.copy()
        bad[field][1] = value
        assert sweep(host=ctypes.c_void_p(bad.ctypes.data)) != 0 and word in err(), field

    def cons(H=8, W=8, depth=p, state=p, ref=ref, S=2, host=None, cams=p, tol=0.008, need=2, out=p):
        return hip_lib.gsr_stereo_consistency(H, W, depth, state, ref, S, ctypes.c_void_p(table.ctypes.data) if host is None else host, cams,
                                              tol, need, out, None)

    assert cons(W=1) != 0 and b"2 x 2" in err()
    assert cons(S=0) != 0 and b"n_sources" in err()
    assert cons(tol=0.0) != 0 and b"tol" in err()
    assert cons(tol=float("inf")) != 0 and b"tol" in err()
    assert cons(need=0) != 0 and b"min_consistent" in err()
    assert cons(need=3) != 0 and b"min_consistent" in err()
    assert cons(state=None) != 0 and b"null" in err()
    assert cons(out=None) != 0 and b"null" in err()
    assert cons(depth=ctypes.c_void_p(base + 2)) != 0 and b"aligned" in err()
    bad = table.copy()
    bad["state"][0] = 0
    assert cons(host=ctypes.c_void_p(bad.ctypes.data)) != 0 and b"state" in err()
    grid = (ctypes.c_int * 6)(0, 0, 0, 1, 1, 1)
    assert hip_lib.gsr_stereo_merge(None, p, p, p, p, p, 3.0, p, p, p, p, None) != 0 and b"grid" in err()
    assert hip_lib.gsr_stereo_merge(grid, p, p, p, p, p, 0.0, p, p, p, p, None) != 0 and b"min_weight" in err()
    assert hip_lib.gsr_stereo_merge(grid, p, p, p, None, p, 3.0, p, p, p, p, None) != 0 and b"null" in err()
    assert hip_lib.gsr_stereo_merge(grid, p, p, p, p, p, 3.0, p, p, p, None, None) != 0 and b"null" in err()
    assert hip_lib.gsr_stereo_merge(grid, p, ctypes.c_void_p(base + 4), p, p, p, 3.0, p, p, p, p, None) != 0 and b"16-byte" in err()


# ------------------------------------------------------------------------------------------------ quality on the restatement
def dent_quality(sc, views, states, step):
    """Over the dent pixels of every camera -- truth - prior > 3 step, the true point seen by every source of the camera --
    (their number, the share that reached state 4, the median |refined - truth| over those of state >= 3 and the prior's median
    error over all of them, both in steps)."""
    n = n4 = 0
    errs, prior_errs = [], []
    for r in range(len(views)):
        truth, prior = sc.truth[r].astype(np.float64), sc.prior[r].astype(np.float64)
        dent = (sc.masks[r] > 0) & (prior < 50) & (truth - prior > 3 * step)
        for s in sc.sources[r]:
            if s >= 0:
                dent &= sr.sees(sc, r, int(s))
        acc = dent & (views[r]["state"] >= 3)
        n, n4 = n + int(dent.sum()), n4 + int((dent & (states[r] == 4)).sum())
        errs += list(np.abs(views[r]["depth"][acc].astype(np.float64) - truth[acc]))
        prior_errs += list(np.abs(prior[dent] - truth[dent]))
    return n, n4 / max(n, 1), float(np.median(errs)) / step, float(np.median(prior_errs)) / step


@pytest.mark.parametrize("size", [(48, 64), (45, 67)])
def test_restated_sweep_recovers_the_dent(size):
    """The condition the GPU tests rest on: over the dent pixels the median |refined - truth| of the accepted ones is below one
    step (the best plane lies within step / 2 of the truth where the cost peaks there: a margin of 2), the prior's median
    error exceeds 3 steps by construction, and at least half of them reach state 4.  Measured at 64 x 48: 1 511 dent pixels,
    84 % of them state 4, median error 0.30 steps against the prior's 6.4."""
    sc = sr.scene(*size)
    cfg = sr.scene_config()
    views = [sr.restated_view(sc, r, cfg) for r in range(sr.N_CAMERAS)]
    states = sr.restated_consistency(sc, views, cfg)
    n, share4, err, prior_err = dent_quality(sc, views, states, cfg.step)
    print(f"{size}: {n} dent pixels, {share4:.3f} reach state 4, median error {err:.3f} steps, the prior's {prior_err:.3f}")
    assert n > 500 and prior_err > 3.0
    assert err < 1.0
    assert share4 >= 0.5
