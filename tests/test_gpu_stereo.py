"""Plane-sweep stereo on the device (gsr_stereo.hip behind gaustar_amd.stereo) against its numpy restatement
tests/stereo_ref.py: luma, the sweep, the consistency pass and the merge bit for bit, that the results do not depend on streams
or runs, and the whole path against the plain hull.  Images are 64 x 48 and 67 x 45 (no multiple of the 16 x 16 tile), one of
12 x 9 (smaller than a tile with its halo) and a source of 40 x 30; volumes are 4 units."""
import numpy as np
import pytest
import torch

import hull_ref as hr
import stereo_ref as sr
from gaustar_amd import evaluate, fusion, hull, stereo

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda")
NAMES = ("depth", "score", "state", "plane")


def _same(view, want, what=""):
    """A device view and a restated one: state and plane as integers, depth and score by their bytes."""
    for name in NAMES:
        g, w = getattr(view, name).cpu().numpy(), want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        assert g.tobytes() == w.tobytes(), (what, name, int((g != w).sum()))


def _lumas(images):
    return [stereo.luma(img, DEV) for img in images]


def _restated(rig, r, srcs, images, prior, cfg):
    rows = sr.source_rows(rig, r, srcs, [images[s] for s in srcs])
    return sr.sweep(images[r], prior, sr.reference_camera(rig, r), rows, cfg.resolved(len(srcs)))


def _device(rig, r, srcs, lumas, prior, cfg):
    return stereo.sweep_view(rig, r, np.array(srcs), lumas, torch.from_numpy(np.ascontiguousarray(prior)).to(DEV), cfg)


@pytest.fixture(scope="module")
def scenes():
    """(H, W) -> the scene, built once; its lumas on the device."""
    out = {}
    for size in ((48, 64), (45, 67)):
        sc = sr.scene(*size)
        out[size] = (sc, _lumas(sc.images))
    return out


# ------------------------------------------------------------------------------------------------ luma
def test_luma_equals_the_restatement():
    rng = np.random.default_rng(11)
    rgb = rng.integers(0, 256, (45, 67, 3)).astype(np.uint8)
    want = sr.luma(rgb)
    got = stereo.luma(rgb, DEV)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (45, 67) and got.is_cuda and np.array_equal(got.cpu().numpy(), want)
    wide = torch.from_numpy(np.repeat(rgb, 2, axis=1)).to(DEV)
    view = wide[:, ::2]
    assert not view.is_contiguous() and np.array_equal(stereo.luma(view).cpu().numpy(), want)
    odd = torch.zeros(45 * 67 * 3 + 1, dtype=torch.uint8, device=DEV)[1:].view(45, 67, 3)       # not 4-byte aligned: the byte path
    odd.copy_(torch.from_numpy(rgb))
    assert odd.data_ptr() % 16 != 0 and np.array_equal(stereo.luma(odd).cpu().numpy(), want)
    for shape in ((2, 2, 3), (3, 5, 3), (1, 7, 3)):                                             # tails of 0, 3 and 3 pixels
        small = rng.integers(0, 256, shape).astype(np.uint8)
        assert np.array_equal(stereo.luma(small, DEV).cpu().numpy(), sr.luma(small)), shape
    grey = torch.from_numpy(want).to(DEV)
    assert stereo.luma(grey).data_ptr() == grey.data_ptr()                                      # [H,W]: luma already


# ------------------------------------------------------------------------------------------------ the sweep
@pytest.mark.parametrize("radius", [1, 2, 3])
@pytest.mark.parametrize("size", [(48, 64), (45, 67)])
def test_sweep_equals_the_restatement_bit_for_bit(scenes, size, radius):
    sc, lumas = scenes[size]
    cfg = sr.scene_config(radius=radius)
    seen = np.zeros(5, np.int64)
    for r in range(sr.N_CAMERAS):
        srcs = [int(s) for s in sc.sources[r] if s >= 0]
        want = _restated(sc.rig, r, srcs, sc.images, sc.prior[r], cfg)
        _same(_device(sc.rig, r, srcs, lumas, sc.prior[r], cfg), want, (size, radius, r))
        seen += np.bincount(want["state"].reshape(-1), minlength=5)
    assert (seen[[0, 2, 3]] > 0).all() and seen[4] == 0


def test_sweep_of_an_image_smaller_than_a_tile():
    _plain, dented, faces = sr.meshes()
    H, W = 9, 12
    rig = hr.look_at_rig(sr.eyes()[3:6], (0.0, 0.0, 0.0), H, W, 30.0)
    images, priors = [], []
    for i in range(3):
        img, depth, _mask = sr.render_view(dented, faces, rig["extrinsics"][i], *sr.reference_camera(rig, i), H, W)
        images.append(img), priors.append(depth)
    lumas = _lumas(images)
    for radius in (1, 2, 3):
        cfg = sr.scene_config(radius=radius, min_var=1.0, min_score=0.3, min_sources=1)
        want = _restated(rig, 1, [0, 2], images, priors[1], cfg)
        _same(_device(rig, 1, [0, 2], lumas, priors[1], cfg), want, radius)
        assert radius == 3 or (want["state"] == 3).any()


@pytest.fixture(scope="module")
def mixed(scenes):
    """The 64 x 48 scene's cameras 3, 4, 5 and two more: camera 9 of 40 x 30 with its own focal length at camera 6's place, and
    camera 10 at camera 2's place looking past the sphere, so that half of the sphere lies off its image."""
    sc, _ = scenes[(48, 64)]
    _plain, dented, faces = sr.meshes()
    small = hr.look_at_rig([sr.eyes()[6]], (0.0, 0.0, 0.0), 30, 40, 90.0)
    aside = hr.look_at_rig([sr.eyes()[2]], (0.0, 0.0, 0.26), 48, 64, sr.FOCAL)
    rig = hr.concat_rigs(sc.rig, small, aside)
    images = list(sc.images)
    for i in (9, 10):
        H, W = (int(v) for v in rig["shape"][i])
        images.append(sr.render_view(dented, faces, rig["extrinsics"][i], *sr.reference_camera(rig, i), H, W)[0])
    return sc, rig, images, _lumas(images)


def test_sweep_with_a_smaller_source_and_one_that_crops_the_subject(mixed):
    sc, rig, images, lumas = mixed
    assert images[9].shape == (30, 40) and 0 < (images[10][:, -1] != sr.BACKGROUND_GREY).sum()      # the sphere crosses the border
    cfg = sr.scene_config()
    for srcs in ([3, 9], [10, 5], [3, 5, 9, 10]):
        want = _restated(rig, 4, srcs, images, sc.prior[4], cfg)
        _same(_device(rig, 4, srcs, lumas, sc.prior[4], cfg), want, srcs)
        assert (want["state"] == 3).sum() > 100
    # the cropping source's warps are valid for a part of the covered pixels only
    row = sr.source_rows(rig, 4, [10], [images[10]])[0]
    rr, cc = np.mgrid[0:48, 0:64]
    w = sr.warp(sr.reference_camera(rig, 4), row, rr, cc, 0.66)[sc.prior[4] < 50]
    assert (w < 0).sum() > 50 and (w >= 0).sum() > 50


def test_sweep_with_one_source_and_with_eight(scenes):
    sc, lumas = scenes[(48, 64)]
    one = sr.scene_config(min_sources=1, min_consistent=1)
    want = _restated(sc.rig, 4, [5], sc.images, sc.prior[4], one)
    _same(_device(sc.rig, 4, [5], lumas, sc.prior[4], one), want, "S = 1")
    assert (want["state"] == 3).sum() > 100
    srcs = [3, 5, 2, 6, 3, 5, 1, 7]                          # two rows of the table name camera 3, two camera 5
    for kw in (dict(), dict(keep=8, min_sources=8), dict(keep=1)):
        cfg = sr.scene_config(**kw)
        want = _restated(sc.rig, 4, srcs, sc.images, sc.prior[4], cfg)
        _same(_device(sc.rig, 4, srcs, lumas, sc.prior[4], cfg), want, ("S = 8", kw))
        assert (want["state"] >= 2).sum() > 100


def test_sweep_priors_two_surfaces_near_constant_and_empty(scenes):
    sc, lumas = scenes[(48, 64)]
    cfg = sr.scene_config()
    srcs = [int(s) for s in sc.sources[4]]
    # two surfaces at different depths inside every tile: odd columns 0.2 farther.  The tile's range is the union of the
    # bands; a pixel's plane lies in its OWN band
    two = sc.prior[4].copy()
    two[:, 1::2] += np.float32(0.2)
    want = _restated(sc.rig, 4, srcs, sc.images, two, cfg)
    got = _device(sc.rig, 4, srcs, lumas, two, cfg)
    _same(got, want, "two surfaces")
    covered, k_lo, k_hi = sr.bands(two, cfg.resolved(4))
    plane = got.plane.cpu().numpy().astype(np.int64)
    has = plane >= 0
    assert has.sum() > 200 and covered[has].all() and (plane[has] >= k_lo[has]).all() and (plane[has] <= k_hi[has]).all()
    assert (k_lo[:, 1::2][covered[:, 1::2]].min() > k_hi[:, 0::2][covered[:, 0::2]].max())          # the two bands do not even meet
    # a prior so near that k_lo clamps at k_min = floor(0.01 / 0.004) + 1 = 3
    near = np.full_like(sc.prior[4], 0.015)
    covered, k_lo, _ = sr.bands(near, cfg.resolved(4))
    assert covered.all() and (k_lo == 3).all() and np.ceil((0.015 - cfg.near) / cfg.step) < 3
    _same(_device(sc.rig, 4, srcs, lumas, near, cfg), _restated(sc.rig, 4, srcs, sc.images, near, cfg), "near")
    # constant images: every covered pixel has state 1, score -2 and the prior's bits
    flat = [np.full_like(img, 90) for img in sc.images]
    got = _device(sc.rig, 4, srcs, _lumas(flat), sc.prior[4], cfg)
    _same(got, _restated(sc.rig, 4, srcs, flat, sc.prior[4], cfg), "constant")
    state = got.state.cpu().numpy()
    cov = sc.prior[4] < 50
    assert (state[cov] == 1).all() and (state[~cov] == 0).all() and (got.score.cpu().numpy() == -2).all()
    assert got.depth.cpu().numpy().tobytes() == sc.prior[4].tobytes() and (got.plane.cpu().numpy() == -1).all()
    # an all-background prior (with one NaN that carries a payload): state 0 everywhere, the prior's bits
    empty = np.full_like(sc.prior[4], 100.0)
    empty.view(np.uint32)[7, 9] = 0x7FC12345
    got = _device(sc.rig, 4, srcs, lumas, empty, cfg)
    _same(got, _restated(sc.rig, 4, srcs, sc.images, empty, cfg), "empty")
    assert not got.state.any() and got.depth.cpu().numpy().tobytes() == empty.tobytes()


# ------------------------------------------------------------------------------------------------ rig, consistency
@pytest.fixture(scope="module")
def swept(scenes):
    """The 67 x 45 scene swept on the device and restated, R = 2: (scene, cfg, device views, restated views)."""
    sc, _ = scenes[(45, 67)]
    cfg = sr.scene_config(radius=2)
    views = stereo.sweep_rig(sc.rig, sc.images, sc.prior, sc.sources, cfg, device=DEV)
    return sc, cfg, views, [sr.restated_view(sc, r, cfg) for r in range(sr.N_CAMERAS)]


def _bits(views):
    return [getattr(v, n).cpu().numpy().tobytes() for v in views for n in NAMES]


def test_sweep_rig_is_reproducible_and_equals_per_camera_sweeps(scenes, swept):
    sc, cfg, views, want = swept
    _, lumas = scenes[(45, 67)]
    for r in range(sr.N_CAMERAS):
        _same(views[r], want[r], r)
    base = _bits(views)
    priors = [torch.from_numpy(p).to(DEV) for p in sc.prior]
    stack = np.stack(sc.images)
    assert _bits(stereo.sweep_rig(sc.rig, stack, priors, sc.sources, cfg, views_in_flight=2, device=DEV)) == base     # a second run
    assert _bits(stereo.sweep_rig(sc.rig, lambda i: sc.images[i], sc.prior, sc.sources, cfg, views_in_flight=1, device=DEV)) == base
    assert _bits([stereo.sweep_view(sc.rig, r, sc.sources[r], lumas, priors[r], cfg) for r in range(sr.N_CAMERAS)]) == base


def test_consistency_equals_the_restatement(swept):
    sc, cfg, views, want = swept
    states = sr.restated_consistency(sc, want, cfg)
    got = stereo.check_consistency(sc.rig, views, sc.sources, cfg)
    n4 = 0
    for r in range(sr.N_CAMERAS):
        g = got[r].state.cpu().numpy()
        assert g.dtype == np.uint8 and np.array_equal(g, states[r]), r
        assert got[r].depth is views[r].depth and np.array_equal(views[r].state.cpu().numpy(), want[r]["state"])     # the input is not written
        n4 += int((g == 4).sum())
    assert n4 > 1000
    # min_consistent = S: the two nearest neighbours, both must agree
    two = np.array([[int(s) for s in row if s >= 0][:2] for row in sc.sources])
    strict = sr.scene_config(radius=2, min_consistent=2)
    got = stereo.check_consistency(sc.rig, views, two, strict)
    for r in range(sr.N_CAMERAS):
        rows = sr.source_rows(sc.rig, r, two[r], [want[s]["depth"] for s in two[r]], [want[s]["state"] for s in two[r]])
        assert np.array_equal(got[r].state.cpu().numpy(),
                              sr.consistency(sr.reference_camera(sc.rig, r), want[r]["depth"], want[r]["state"], rows, strict.resolved(2).tol, 2)), r


def test_consistency_tolerance_is_inclusive(swept):
    """tol at exactly one measured difference: that pixel agrees (<=), and at the next smaller double it does not."""
    sc, cfg, views, want = swept
    r, s = 4, 5
    one = np.array([[s] if i == r else [r] for i in range(sr.N_CAMERAS)])       # camera 4 reads 5, the others read 4
    row = sr.source_rows(sc.rig, r, [s], [want[s]["depth"]], [want[s]["state"]])
    ok, gap = sr.agreement_gaps(sr.reference_camera(sc.rig, r), want[r]["depth"], row[0])
    cand = ok & (want[r]["state"] == 3) & (gap > 1e-4) & (gap < 0.004)
    assert cand.any()
    y, x = (int(v[0]) for v in np.nonzero(cand))
    tol = float(gap[y, x])
    for t, state in ((tol, 4), (float(np.nextafter(tol, 0.0)), 3)):
        c = sr.scene_config(radius=2, min_sources=1, min_consistent=1, tol=t)
        got = stereo.check_consistency(sc.rig, views, one, c)[r].state.cpu().numpy()
        assert got[y, x] == state
        assert np.array_equal(got, sr.consistency(sr.reference_camera(sc.rig, r), want[r]["depth"], want[r]["state"], row, t, 1))


# ------------------------------------------------------------------------------------------------ merge
def test_merge_equals_the_restatement():
    rng = np.random.default_rng(5)
    a = fusion.TSDFVolume.from_units((0, -1, 2), (2, 2, 1), hr.VOXEL, hr.TRUNC, DEV)        # 4 units: 16 x 32 x 32 voxels
    b = fusion.TSDFVolume.from_units((0, -1, 2), (2, 2, 1), hr.VOXEL, hr.TRUNC, DEV)
    shape = tuple(a.tsdf.shape)
    th = rng.uniform(-1, 1, shape).astype(np.float32)
    ts = rng.uniform(-1, 1, shape).astype(np.float32)
    wh = (rng.random(shape) < 0.8).astype(np.float32)                                       # w_h = 0 voxels
    ws = rng.integers(0, 6, shape).astype(np.float32)                                       # 3 = exactly min_weight
    cs = rng.uniform(0, 255, (3, *shape)).astype(np.float32)
    # unit (0, 0): touched under the hull (-0.5), carved away to +1 everywhere: becomes untouched
    th[:, :16, :16], wh[:, :16, :16], ts[:, :16, :16], ws[:, :16, :16] = -0.5, 1, 1.0, 3
    # unit (1, 0): the hull's is -1 throughout (untouched), stereo puts a surface there: becomes touched
    th[:, :16, 16:], wh[:, :16, 16:], ts[:, :16, 16:], ws[:, :16, 16:] = -1.0, 1, 0.25, 4
    for vol, t, w in ((a, th, wh), (b, ts, ws)):
        vol.tsdf.copy_(torch.from_numpy(t)), vol.weight.copy_(torch.from_numpy(w))
    b.color.copy_(torch.from_numpy(cs))
    t, w, c, touched = sr.merge(th, wh, ts, ws, cs, 3.0)
    out = stereo.merge_volumes(a, b, 3.0)
    assert isinstance(out, fusion.TSDFVolume) and out is not a and [int(v) for v in out.nu] == [2, 2, 1]
    for name, g, want in (("tsdf", out.tsdf, t), ("weight", out.weight, w), ("color", out.color, c)):
        assert g.cpu().numpy().tobytes() == want.tobytes(), name
    assert np.array_equal(out.touched.cpu().numpy(), touched.reshape(-1).astype(np.uint8))
    before = ((wh == 1) & (np.abs(th) < 1)).reshape(1, 16, 2, 16, 2, 16).any(axis=(1, 3, 5)).reshape(-1)
    assert before[0] and not touched.reshape(-1)[0] and not before[1] and touched.reshape(-1)[1]
    assert ((ws == 3) & (wh == 1) & (ts > th)).sum() > 100 and a.tsdf.cpu().numpy().tobytes() == th.tobytes()     # the inputs stay
    assert stereo.merge_volumes(a, b, 3.0).tsdf.cpu().numpy().tobytes() == t.tobytes()


# ------------------------------------------------------------------------------------------------ the whole path
def test_refine_hull_recovers_the_dent(scenes):
    """Samples of the true dent farther than 3 voxels from the hull's mesh: more than 100, and their median distance to the
    refined mesh is below 1.5 voxels (a depth within one step is half a voxel, plus the TSDF's sub-voxel error: a margin of
    1.5).  The same chain restated on the CPU (stereo_ref.restated_chain) gives 0.44 voxels over such samples, the hull 3.2.
    Outside the dent the refined mesh is not farther from the truth than the hull by more than one voxel."""
    sc, _ = scenes[(48, 64)]
    cfg = sr.scene_config()
    colour = [np.repeat(img[:, :, None], 3, axis=2) for img in sc.images]
    kw = dict(lo=hr.BOX[0], hi=hr.BOX[1], voxel_size=hr.VOXEL, sdf_trunc=hr.TRUNC, min_views=sr.MIN_VIEWS, taubin_iterations=0,
              target_faces=0, device=DEV)
    hv, hf = hull.hull_mesh(sc.rig, sc.masks, **kw)
    rv, rf, info = stereo.refine_hull(sc.rig, colour, sc.masks, **kw, sources=sc.sources, cfg=cfg)
    assert info["states"].shape == (sr.N_CAMERAS, 5) and (info["states"].sum(1) == 48 * 64).all() and (info["states"][:, 4] > 300).all()
    assert info["hull_faces"] == int(hf.shape[0]) and info["faces"] == int(rf.shape[0])
    pts = torch.from_numpy(sr.dent_samples(sc)).to(DEV)
    to_hull = evaluate.surface_distance(pts, hv, hf).dist
    to_refined = evaluate.surface_distance(pts, rv, rf).dist
    far = to_hull > 3 * hr.VOXEL
    median = float(to_refined[far].median())
    print(f"{int(far.sum())} samples beyond 3 voxels of the hull: median distance to the refined mesh {median / hr.VOXEL:.3f} voxels, "
          f"to the hull {float(to_hull[far].median()) / hr.VOXEL:.3f}")
    assert int(far.sum()) > 100
    assert median < 1.5 * hr.VOXEL
    truth_v, truth_f = torch.from_numpy(sc.dented).to(DEV), torch.from_numpy(sc.faces.astype(np.int32)).to(DEV)
    axis = torch.from_numpy(sr.dent_axis()).to(DEV)

    def worst_outside(v):
        v = v.double()
        away = torch.arccos(torch.clamp((v / v.norm(dim=1, keepdim=True)) @ axis, -1, 1)) > sr.DENT_HALF_ANGLE + 0.15
        return float(evaluate.surface_distance(v[away].contiguous(), truth_v, truth_f).dist.max())

    assert worst_outside(rv) <= worst_outside(hv) + hr.VOXEL


def test_stereo_files_carry_the_hull_files_names(scenes, tmp_path):
    """write_stereo_meshes on one frame of the scene: the name write_hull_meshes writes, the mesh refine_hull returns."""
    import os

    from gaustar_amd import formats
    sc, _ = scenes[(48, 64)]
    gstar, src, meshes = (os.path.join(tmp_path, n) for n in ("gstar", "capture", "meshes"))
    os.makedirs(gstar)
    np.savez(os.path.join(gstar, "rgb_cameras.npz"), ids=np.arange(sr.N_CAMERAS), intrinsics=sc.rig["intrinsics"],
             extrinsics=sc.rig["extrinsics"], shape=sc.rig["shape"])
    image_of, mask_of = stereo.gstar_image_path(gstar), hull.actorshq_mask_path(src)
    assert image_of(3, 7).endswith(os.path.join("0007", "images", "img_0003.png"))
    for c in range(sr.N_CAMERAS):
        for path, save, data in ((image_of(c, 0), formats.save_png_rgb8, np.repeat(sc.images[c][:, :, None], 3, axis=2)),
                                 (mask_of(c, 0), formats.save_png_gray8, sc.masks[c])):
            os.makedirs(os.path.dirname(path), exist_ok=True)
            save(path, data)
    kw = dict(lo=hr.BOX[0], hi=hr.BOX[1], voxel_size=hr.VOXEL, sdf_trunc=hr.TRUNC, min_views=sr.MIN_VIEWS, taubin_iterations=0,
              target_faces=0, cfg=sr.scene_config())
    written = stereo.write_stereo_meshes(gstar, gstar, src, meshes, 0, 1, 1, **kw)
    assert [os.path.basename(p) for p in written] == ["mesh_000000_smooth_100k.obj"]
    colour = [np.repeat(img[:, :, None], 3, axis=2) for img in sc.images]
    verts, faces, _info = stereo.refine_hull(sc.rig, colour, sc.masks, sources=stereo.select_sources(sc.rig, 4), device=DEV, **kw)
    v, f = formats.load_obj(written[0])[:2]
    assert len(f) == int(faces.shape[0]) > 3000 and len(v) == int(verts.shape[0])
    with pytest.raises(ValueError):
        stereo.write_stereo_meshes(gstar, gstar, src, meshes, 0, 0, 1)
