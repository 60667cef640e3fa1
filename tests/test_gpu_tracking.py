"""gaustar_amd.tracking on the GPU against the numpy restatement tests/tracking_ref.py (itself pinned by tests/test_tracking.py).
Ids, barycentrics, positions and counts are compared bit for bit: every operation is an IEEE add, multiply, divide or square
root of float64 in a stated order."""
import functools

import numpy as np
import pytest
import torch

import tracking_ref as ref

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")


def _t(a, dtype=None):
    t = torch.from_numpy(np.array(a, order="C"))
    return t.to(DEV) if dtype is None else t.to(DEV, dtype)


def _n(t):
    return t.cpu().numpy()


def _same(got, want):
    got, want = _n(got) if torch.is_tensor(got) else np.asarray(got), np.asarray(want)
    return got.shape == want.shape and got.dtype == want.dtype and got.tobytes() == want.tobytes()


def _tracker(ids, bary=None):
    from gaustar_amd import tracking
    return tracking.SurfaceTracker(np.asarray(ids, np.int32), None if bary is None else np.asarray(bary, np.float64), device=DEV)


def _soup(rng, n, lo=0.0, hi=1.0, size=0.05):
    """n separate small triangles in [lo, hi]^3 -> (verts [3n,3], faces [n,3])"""
    c = rng.uniform(lo, hi, size=(n, 1, 3))
    verts = (c + rng.uniform(-size, size, size=(n, 3, 3))).reshape(-1, 3)
    return verts, np.arange(3 * n, dtype=np.int32).reshape(n, 3)


def _check_rebind(verts, faces, ids, bary, mask, new_verts, new_faces):
    """positions + rebind on the GPU equal the restatement -> (tracker, stats, want_ids, want_bary)"""
    tr = _tracker(ids, bary)
    pos = tr.positions(_t(verts), _t(faces))
    bary = np.ones((len(ids), 3)) / 3 if bary is None else bary
    want_pos = ref.positions(verts, faces, np.asarray(ids), bary)
    assert _same(pos, want_pos)
    stats = tr.rebind(pos, _t(np.asarray(mask, bool)), _t(new_verts), _t(new_faces))
    want_ids, want_bary, want_stats = ref.rebind(ids, bary, want_pos, mask, new_verts, new_faces)
    assert tuple(stats) == want_stats, (tuple(stats), want_stats)
    assert tr.face_ids.dtype == torch.int32 and tr.face_bary.dtype == torch.float64
    assert np.array_equal(_n(tr.face_ids), want_ids), np.nonzero(_n(tr.face_ids) != want_ids)[0][:10]
    assert _same(tr.face_bary, want_bary), np.nonzero((_n(tr.face_bary) != want_bary).any(axis=1))[0][:10]
    assert np.array_equal(_n(tr.face_ids_ori), np.asarray(ids))
    return tr, stats, want_ids, want_bary


# ---------------------------------------------------------------------------------------------------- 1 positions
@pytest.mark.parametrize("K", (1, 63, 64, 65, 1000))
def test_positions(K):
    rng = np.random.default_rng(K)
    verts, faces = ref.grid_mesh(12, height=lambda X, Y: 0.1 * np.sin(4 * X + Y))
    verts = verts + rng.normal(0, 0.01, size=verts.shape)
    special = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [0.5, 0.5, 0], [0, 0.25, 0.75], [1, 0, 0]], np.float64)
    bary = rng.dirichlet(np.ones(3), size=K)
    bary[:min(K, 6)] = special[:min(K, 6)]                          # rows holding exact zeros and ones
    ids = rng.integers(0, len(faces), size=K).astype(np.int32)
    tr = _tracker(ids, bary)
    pos = tr.positions(_t(verts), _t(faces))
    assert pos.dtype == torch.float64 and tuple(pos.shape) == (K, 3)
    assert _same(pos, ref.positions(verts, faces, ids, bary))
    # a point of barycentric (1, 0, 0) is its face's first vertex, exactly
    assert np.array_equal(_n(pos)[0], verts[faces[ids[0], 0]])
    # f32 vertices and int64 faces are widened / narrowed, exactly
    v32 = verts.astype(np.float32)
    assert _same(tr.positions(_t(v32), _t(faces.astype(np.int64))), ref.positions(v32.astype(np.float64), faces, ids, bary))


def test_default_barycentrics_and_constructors():
    from gaustar_amd import tracking
    tr = tracking.SurfaceTracker.sample(1000, device=DEV)
    assert _n(tr.face_ids).tolist() == [10, 210, 410, 610] and _same(tr.face_bary, np.ones((4, 3)) / 3)
    assert len(tracking.SurfaceTracker.sample(210, device=DEV)) == 0
    tr = tracking.SurfaceTracker.dense(77, device=DEV)
    assert _n(tr.face_ids).tolist() == list(range(77)) and _n(tr.face_ids_ori).tolist() == list(range(77))
    with pytest.raises(ValueError):
        tracking.SurfaceTracker(np.zeros(3, np.float32), device=DEV)
    with pytest.raises(ValueError):
        tracking.SurfaceTracker(np.zeros(3, np.int32), np.zeros((3, 3), np.float32), device=DEV)
    with pytest.raises(ValueError):
        tracking.SurfaceTracker(np.zeros(3, np.int32), device="cpu")


# ---------------------------------------------------------------------------------------------------- 2 the three branches
@functools.lru_cache(maxsize=None)
def _branches():
    c = ref.branches_case()
    for a in c.values():
        a.setflags(write=False)
    return c


def test_three_branches():
    c = _branches()
    pos = ref.positions(c["verts"], c["faces"], c["ids"], c["bary"])
    _i, _b, (kept, moved, lost) = ref.rebind(c["ids"], c["bary"], pos, c["mask"], c["new_verts"], c["new_faces"])
    print("kept / moved / lost:", kept, moved, lost)
    assert min(kept, moved, lost) >= 100
    assert len(c["new_faces"]) == 4152                              # four LDS tiles and a remainder
    _check_rebind(c["verts"], c["faces"], c["ids"], c["bary"], c["mask"], c["new_verts"], c["new_faces"])


# ---------------------------------------------------------------------------------------------------- 3 search boundaries
TODO_LENGTHS = (0, 1, 15, 16, 17, 257)


@pytest.mark.parametrize("F1", (1, 1023, 1024, 1025, 2049))
def test_search_boundaries(F1):
    from gaustar_amd import _lib, tracking
    lib = _lib.load()
    assert lib.gsr_track_nn_tile() == 1024 and lib.gsr_track_nn_queries() == 16      # what the sizes here straddle
    rng = np.random.default_rng(F1)
    for n in TODO_LENGTHS:
        s = min(3, F1)                                              # survivors: the first faces of the new mesh
        K = n + s
        verts, faces = _soup(rng, K)
        mask = np.zeros(K, bool)
        mask[np.linspace(0, K - 1, s).astype(int)] = True
        fv, ff = _soup(rng, F1 - s)
        new_verts = np.concatenate([verts, fv])
        new_faces = np.concatenate([faces[mask], ff + len(verts)]).astype(np.int32)
        _tr, stats, want_ids, _wb = _check_rebind(verts, faces, np.arange(K, dtype=np.int32), None, mask, new_verts, new_faces)
        assert tuple(stats) == (s, 0, n)
        # bind_points: the same search, unclamped
        pts = rng.uniform(0, 1, size=(n, 3))
        ids, bary = tracking.bind_points(_t(new_verts), _t(new_faces), _t(pts))
        wi, wb = ref.bind_points(new_verts, new_faces, pts)
        assert ids.dtype == torch.int32 and np.array_equal(_n(ids), wi) and _same(bary, wb)


def test_exact_tie_takes_the_lower_index():
    from gaustar_amd import tracking
    rng = np.random.default_rng(5)
    verts, faces = _soup(rng, 2049)
    verts[faces[3]] += 10.0                                         # face 3 alone out there ...
    verts[faces[1027]] = verts[faces[3]]                            # ... but for its copy in the second tile
    cen = ref.centres(verts, faces)
    assert np.array_equal(cen[3], cen[1027])
    pts = np.stack([cen[3], cen[3] + 0.01, cen[5]])
    ids, bary = tracking.bind_points(_t(verts), _t(faces), _t(pts))
    wi, wb = ref.bind_points(verts, faces, pts)
    assert _n(ids).tolist() == [3, 3, 5] == wi.tolist() and _same(bary, wb)


def _collision_mesh(F1, at_far, at_near):
    x_far, x_near, y, _i, _j = ref.sqrt_collision()
    rng = np.random.default_rng(F1)
    verts, faces = _soup(rng, F1, 5.0, 6.0)
    verts[faces[at_far]] = ref.centre_face(x_far, y)
    verts[faces[at_near]] = ref.centre_face(x_near, y)
    cen = ref.centres(verts, faces)
    assert np.array_equal(cen[at_far], [x_far, y, 0.0]) and np.array_equal(cen[at_near], [x_near, y, 0.0])
    d2 = ((cen[:, 0] * cen[:, 0] + cen[:, 1] * cen[:, 1]) + cen[:, 2] * cen[:, 2])
    assert d2[at_far] > d2[at_near] and np.sqrt(d2[at_far]) == np.sqrt(d2[at_near])
    return verts, faces


@pytest.mark.parametrize("F1,at_far,at_near", [(40, 3, 7), (40, 3, 19), (2049, 3, 1027), (2049, 1030, 2048)])
def test_sqrt_collision_takes_the_lower_index(F1, at_far, at_near):
    """Two centres whose squared distances from the query differ and whose rounded square roots are equal: numpy's argmin sees
    a tie and takes the lower index, the FARTHER centre.  A search that ranks squared distances takes the other one."""
    new_verts, new_faces = _collision_mesh(F1, at_far, at_near)
    assert ref.nearest(np.zeros(3), ref.centres(new_verts, new_faces)) == at_far
    old_verts = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0]], np.float64)
    old_faces = np.array([[0, 1, 2]], np.int32)
    tr, stats, want_ids, _wb = _check_rebind(old_verts, old_faces, np.array([0], np.int32), np.array([[1.0, 0, 0]]), np.array([False]),
                                             new_verts, new_faces)
    assert tuple(stats) == (0, 0, 1) and _n(tr.face_ids).tolist() == [at_far] == want_ids.tolist()


# ---------------------------------------------------------------------------------------------------- 4 clamp
def test_clamp_and_unclamped_binding():
    from gaustar_amd import tracking
    verts, faces = ref.grid_mesh(6)
    new_verts, new_faces = ref.grid_mesh(3, 0.4, 0.6)
    rng = np.random.default_rng(2)
    K = len(faces)
    bary = rng.dirichlet(np.ones(3), size=K)
    tr, stats, _wi, want_bary = _check_rebind(verts, faces, np.arange(K, dtype=np.int32), bary, np.zeros(K, bool), new_verts, new_faces)
    assert tuple(stats) == (0, 0, K) and bool((tr.face_bary >= 0).all())
    pos = ref.positions(verts, faces, np.arange(K), bary)
    ids, unclamped = tracking.bind_points(_t(new_verts), _t(new_faces), _t(pos))
    wi, wb = ref.bind_points(new_verts, new_faces, pos)
    assert np.array_equal(_n(ids), wi) and _same(unclamped, wb)
    outside = (wb < 0).any(axis=1)
    assert outside.sum() >= K // 2 and (wb[outside].min(axis=1) < -1.0).sum() >= 10     # well outside their nearest face
    assert np.array_equal(_n(tr.face_ids), wi)
    assert np.array_equal(want_bary[~outside], wb[~outside]) and (want_bary[outside] == 0).any(axis=1).all()


# ---------------------------------------------------------------------------------------------------- 5 errors
def test_errors_raise_and_leave_the_tracker_alone():
    from gaustar_amd import tracking
    c = _branches()
    verts, faces, new_verts, new_faces = _t(c["verts"]), _t(c["faces"]), _t(c["new_verts"]), _t(c["new_faces"])
    mask = _t(c["mask"])
    F0 = len(c["faces"])
    tr = _tracker(c["ids"], c["bary"])
    before = (tr.face_ids.clone(), tr.face_bary.clone())
    pos = tr.positions(verts, faces)

    def unchanged():
        return torch.equal(tr.face_ids, before[0]) and torch.equal(tr.face_bary, before[1])

    for bad in (mask[:-1], torch.cat([mask, mask[:1]])):           # a mask of the wrong length
        with pytest.raises(ValueError):
            tr.rebind(pos, bad, new_verts, new_faces)
        assert unchanged()
    fresh = _tracker(c["ids"], c["bary"])                           # ... also where no positions() call told the tracker F0
    with pytest.raises(ValueError):
        fresh.rebind(pos, mask[:-1], new_verts, new_faces)
    with pytest.raises(ValueError):                                 # an id >= F0
        far = _tracker([0, F0], None)
        far.rebind(far.positions(verts, faces), mask, new_verts, new_faces)
    nan_verts = new_verts.clone()
    nan_verts[int(c["new_faces"][5, 1]), 2] = float("nan")
    with pytest.raises(ValueError):                                 # a NaN vertex of the new mesh
        tr.rebind(pos, mask, nan_verts, new_faces)
    assert unchanged()
    old_nan = verts.clone()
    old_nan[int(c["faces"][9, 0]), 0] = float("inf")
    with pytest.raises(ValueError):                                 # ... and of the old one: a position that is not finite
        tr.rebind(tr.positions(old_nan, faces), mask, new_verts, new_faces)
    with pytest.raises(ValueError):                                 # a face index outside the vertices
        bad_faces = new_faces.clone()
        bad_faces[0, 0] = new_verts.shape[0]
        tr.rebind(pos, mask, new_verts, bad_faces)
    with pytest.raises(ValueError):                                 # a new mesh with no faces
        tr.rebind(pos, mask, new_verts, new_faces[:0])
    with pytest.raises(ValueError):
        tracking.bind_points(new_verts, new_faces[:0], pos)
    with pytest.raises(ValueError):                                 # wrong dtype, wrong device
        tr.rebind(pos.float(), mask, new_verts, new_faces)
    with pytest.raises(ValueError):
        tr.rebind(pos, mask.cpu(), new_verts, new_faces)
    with pytest.raises(ValueError):
        tr.rebind(pos, mask, new_verts.cpu(), new_faces.cpu())
    with pytest.raises(ValueError):
        tr.positions(verts.cpu(), faces.cpu())
    assert unchanged()
    # a degenerate face (two equal vertices) that is the nearest of some point: the reference's assert (:125)
    dv = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 0], [5, 5, 0], [6, 5, 0]], np.float64)
    one = _tracker([0], None)
    p = one.positions(_t(dv), _t(np.array([[0, 1, 2]], np.int32)))
    with pytest.raises(ValueError, match="degenerate"):
        one.rebind(p, _t(np.array([False])), _t(dv), _t(np.array([[3, 4, 5]], np.int32)))
    assert _n(one.face_ids).tolist() == [0]
    # after all that the tracker still works
    stats = tr.rebind(tr.positions(verts, faces), mask, new_verts, new_faces)
    assert sum(stats) == F0


# ---------------------------------------------------------------------------------------------------- 6 sequence
def _sequence(tmp_path):
    from gaustar_amd import formats
    rng = np.random.default_rng(11)
    height = lambda X, Y: 0.05 * np.sin(3.0 * X) * np.cos(2.0 * Y)
    v0, f_all = ref.grid_mesh(23, height=height)
    f0 = f_all[:1000]
    v1 = v0 + np.array([0.01, 0.0, 0.005]) + 0.01 * np.sin(5 * v0[:, :1])
    cen = ref.centres(v1, f0)
    mask = ~(np.abs(cen[:, 0] - 0.4) < 0.15)                        # a strip: face 410 of the sample is in it
    nv = v1.copy()
    nv[:, :2] += rng.normal(0.0, 0.004, size=(len(nv), 2))
    pv, pf = ref.grid_mesh(10, 0.25, 0.55, height=height)
    new_verts = np.concatenate([nv, pv])
    new_faces = np.concatenate([f0[mask], pf + len(nv)]).astype(np.int32)
    v2 = new_verts + np.array([0.0, 0.02, 0.0])
    base = str(tmp_path)
    ref.write_sequence(base, formats.save_obj, {0: (v0, f0), 1: (v1, f0), 2: (v2, new_faces)}, 1, (mask, new_verts, new_faces))
    return base, dict(v0=v0, f0=f0, v1=v1, mask=mask, new_verts=new_verts, new_faces=new_faces, v2=v2)


@pytest.mark.parametrize("dense", (False, True))
def test_sequence(tmp_path, dense):
    import os
    from gaustar_amd import formats, tracking
    base, s = _sequence(tmp_path)
    path, largest = tracking.track_faces(base, frame_0=0, frame_end=3, interval=1, sample_points=True, dense=dense, device=DEV)
    ids = np.arange(1000, dtype=np.int32) if dense else ref.sample_ids(1000).astype(np.int32)
    K = len(ids)
    assert K == (1000 if dense else 4)
    assert path == os.path.join(base, "tracking", f"tracking_{K}faces_0to3.npz") and os.path.exists(path)
    assert not os.path.exists(os.path.join(base, "tracking", "tracking_debug.ply"))

    def load(f, tail=""):
        v, fc, _c = formats.load_obj(os.path.join(base, f"{f:04d}{tail}", "color_mesh.obj"))
        return v, fc

    want, _wi, _wb = ref.track_sequence(load, lambda f: f == 1, lambda f: (s["mask"],) + load(f, "_update"), ids, np.ones((K, 3)) / 3,
                                        0, 3, 1)
    with np.load(path) as z:
        assert sorted(z.files) == ["face_ids_ori", "face_trajectory", "frames"]
        assert z["face_ids_ori"].dtype == np.int32 and np.array_equal(z["face_ids_ori"], ids)
        assert z["frames"].dtype == np.int64 and z["frames"].tolist() == [0, 3, 1]
        traj = z["face_trajectory"]
    assert _same(traj, want) and traj.shape == (3, K, 3)
    # frame 1's row is the position BEFORE the re-bind: the original ids on frame 1's own mesh
    assert _same(traj[1], ref.positions(s["v1"], s["f0"], ids, np.ones((K, 3)) / 3))
    steps = np.linalg.norm(np.diff(want, axis=0), axis=-1)
    assert abs(largest - steps.max()) <= 1e-15 and (~s["mask"][ids]).any()


# ---------------------------------------------------------------------------------------------------- 7 a real update
def test_rebind_update_on_the_chain_case():
    from gaustar_amd import regions, tracking
    from test_gpu_splice import _Mesh, _regions_of
    from test_splice import chain_case
    bv, bf, fv, ff, raw = chain_case()
    upd = regions.update_mesh_topology(_t(bv), _t(bf), _regions_of(raw), _Mesh(fv, ff))
    assert not upd.nothing_to_update
    K = len(bf)
    bary = np.random.default_rng(4).dirichlet(np.ones(3), size=K)
    ids = np.arange(K, dtype=np.int32)
    tr = _tracker(ids, bary)
    pos = tr.positions(_t(bv), _t(bf))
    want_pos = ref.positions(bv.astype(np.float64), bf, ids, bary)
    assert _same(pos, want_pos)
    stats = tr.rebind_update(pos, upd)
    want_ids, want_bary, want_stats = ref.rebind(ids, bary, want_pos, _n(upd.track_face_mask), _n(upd.verts).astype(np.float64),
                                                 _n(upd.faces))
    print("kept / moved / lost:", want_stats)
    assert tuple(stats) == want_stats and want_stats[0] > 0 and want_stats[2] > 0
    assert np.array_equal(_n(tr.face_ids), want_ids) and _same(tr.face_bary, want_bary)
    none = regions.update_mesh_topology(_t(bv), _t(bf), _regions_of(np.zeros((0, 2, 3))), _Mesh(fv, ff))
    with pytest.raises(ValueError):
        tr.rebind_update(pos, none)


def test_model_hook():
    from gaustar_amd import harness
    verts, faces = ref.grid_mesh(4)
    model = harness.SurfaceGaussians(_t(verts, torch.float32), _t(faces, torch.long), n_gaussians_per_surface_triangle=1, sh_levels=1)
    tr = _tracker(np.arange(len(faces)), None)
    want = ref.positions(verts.astype(np.float32).astype(np.float64), faces, np.arange(len(faces)), np.ones((len(faces), 3)) / 3)
    assert _same(model.track(tr), want)


# ---------------------------------------------------------------------------------------------------- 8 determinism, purity
def test_determinism_and_purity():
    c = _branches()
    args = (_t(c["mask"]), _t(c["new_verts"]), _t(c["new_faces"]))
    out = []
    for _ in range(2):
        tr = _tracker(c["ids"], c["bary"])
        before = (tr.face_ids.clone(), tr.face_bary.clone(), tr.face_ids_ori.clone())
        pos = tr.positions(_t(c["verts"]), _t(c["faces"]))
        assert all(torch.equal(a, b) for a, b in zip(before, (tr.face_ids, tr.face_bary, tr.face_ids_ori)))
        assert torch.equal(pos, tr.positions(_t(c["verts"]), _t(c["faces"])))
        stats = tr.rebind(pos, *args)
        out.append((_n(pos).tobytes(), _n(tr.face_ids).tobytes(), _n(tr.face_bary).tobytes(), tuple(stats)))
    assert out[0] == out[1]
