"""tests/handover_ref.py, the numpy restatement of the colour hand-over, pinned: the face colours against the reference's
expression written directly in numpy, the SH dc against the torch CPU expression of sugar_model.py:237-240 with RGB2SH, the
face -> vertex means against a dense float64 matrix product, face_origin against splice_ref's loop and its own invariants.  The
parts of the feature that run without a GPU (TopologyUpdate.save with colours, load_tracking, tracked_pre_sh, from_mesh's
argument checks) are tested here as well.  No GPU."""
import functools

import numpy as np
import pytest
import torch

import handover_ref as ref
import regions_ref as rr
import splice_ref
from test_splice import GAP_FACE, chain_case, chain_want, grid_case

GS = (1, 3, 4, 6)


# ---------------------------------------------------------------------------------------------------- inputs on the edges
@functools.lru_cache(maxsize=None)
def edge_dc(G, F):
    """[F G,3] f32 face-major SH dc whose face colours sit on the integer edges, F faces (the pattern below, tiled and cut):
      * for k = 1 .. 254: dc = RGB2SH(k / 255) and its two f32 neighbours, the same for all G Gaussians (the mean is then exact
        for G = 1, 4 and off by a rounding for 3, 6), where one rounding more or less flips the integer;
      * results below 0, among them one in (-1, 0) that must truncate to 0, and results above 255;
      * faces whose G values differ in magnitude by 2^24 and more, so that another summation order gives another mean.
    Read-only."""
    k = np.arange(1, 255, dtype=np.float32)
    mid = ref.rgb_to_sh(np.divide(k, np.float32(255.0)))
    rows = [np.nextafter(mid, np.float32(-np.inf)), mid, np.nextafter(mid, np.float32(np.inf))]
    flat = np.stack(rows, axis=1).reshape(-1)                                        # 762 values, one per face-channel
    special = ref.rgb_to_sh(np.array([-0.5, -0.003, -1e-9, 0.0, 1.0, 1.0039, 1.5, 300.0, -300.0], np.float32))
    flat = np.concatenate([flat, special, np.zeros((-len(flat) - len(special)) % 3, np.float32)])
    same = np.repeat(flat.reshape(-1, 1, 3), G, axis=1)                              # [n,G,3]
    rng = np.random.default_rng(11)
    n_mixed = 40
    mixed = rng.uniform(-1.5, 1.5, size=(n_mixed, G, 3)).astype(np.float32)
    if G > 2:
        mixed[:, 0] = np.float32(2.0 ** 24) * np.sign(mixed[:, 0])                    # big + small + ... - big: the order shows
        mixed[:, -1] = -mixed[:, 0]
    pattern = np.concatenate([same, mixed])
    reps = -(-F // len(pattern))
    out = np.tile(pattern, (reps, 1, 1))[:F].reshape(F * G, 3).copy()
    out.setflags(write=False)
    return out


def reference_face_colors(sh_dc, G):
    """sugar_model.py:583-586 as it stands, on the float32 array a state dict gives."""
    C0 = 0.28209479177387814
    face_color = np.asarray(sh_dc, np.float32).reshape(-1, G, 3)
    face_color = np.int32((np.average(face_color, axis=1) * C0 + 0.5) * 255)
    return np.clip(face_color, 0, 255)


@pytest.mark.parametrize("G", GS)
def test_face_colors_against_the_reference_expression(G):
    dc = edge_dc(G, 1000)
    got = ref.sh_face_colors(dc, G)
    assert got.dtype == np.uint8 and got.shape == (1000, 4) and (got[:, 3] == 255).all()
    assert np.array_equal(got[:, :3], reference_face_colors(dc, G))
    rng = np.random.default_rng(G)
    dc = rng.normal(0, 1.2, size=(5000 * G, 3)).astype(np.float32)
    assert np.array_equal(ref.sh_face_colors(dc, G)[:, :3], reference_face_colors(dc, G))


@pytest.mark.parametrize("G", GS)
def test_edge_inputs_do_test_something(G):
    """The three neighbours of a k / 255 edge do not all give the same integer, results beyond both ends are there, and for
    G > 2 another summation order gives other colours."""
    dc = edge_dc(G, 1000).reshape(-1, G, 3)
    got = ref.sh_face_colors(dc, G)[:, :3]
    trip = got.reshape(-1)[:762].reshape(254, 3)                                      # [k, (below, at, above)]
    assert (trip[:, 0] != trip[:, 2]).sum() > 100 and (np.diff(trip.astype(int), axis=1) >= 0).all()
    raw = np.multiply(np.add(np.multiply(np.divide(dc.astype(np.float32).sum(axis=1, dtype=np.float32), np.float32(G)), ref.C0),
                             np.float32(0.5)), np.float32(255.0))
    assert ((raw > -1) & (raw < 0)).any() and (raw < -1).any() and (raw > 256).any()
    if G > 2:
        backwards = ref.sh_face_colors(dc[:, ::-1].reshape(-1, 3), G)[:, :3]
        assert not np.array_equal(backwards, got)
    # a contracted multiply-add (one rounding for m C0 + 0.5) gives other integers somewhere
    if G == 1:
        m = dc[:, 0]
        fused = ((m.astype(np.float64) * np.float64(ref.C0) + 0.5).astype(np.float32) * np.float32(255.0))
        fused = np.clip(np.trunc(fused).astype(np.int64), 0, 255)
        assert not np.array_equal(fused, got)


def test_vertex_to_face_roundings():
    # 0.5 / 255 and 1.5 / 255 are ties in f32 only if the product is exact; 127.5 / 255 = 0.5 is: rint(127.5) = 128 (even)
    assert ref.unit_to_u8(np.array([0.5, 0.0, 1.0, -0.2, 1.2, 2.5 / 255], np.float32)).tolist()[:5] == [128, 0, 255, 0, 255]
    col = np.array([[0, 0, 0], [1, 1, 1], [1 / 255, 2 / 255, 0.5]], np.float32)
    out = ref.vertex_to_face_colors([[0, 1, 2], [1, 1, 2]], col)
    assert out.tolist() == [[(0 + 255 + 1) // 3, (0 + 255 + 2) // 3, (0 + 255 + 128) // 3, 255],
                            [(255 + 255 + 1) // 3, (255 + 255 + 2) // 3, (255 + 255 + 128) // 3, 255]]


def fan_case(n=300):
    """n faces of colour 255 round vertex 0: its sum, 76 500, does not fit 16 bits."""
    faces = np.array([[0, 1 + i, 1 + (i + 1) % n] for i in range(n)], np.int32)
    return faces, np.full((n, 4), 255, np.uint8), n + 1


def test_face_to_vertex_against_a_matrix_product():
    faces, V = grid_case()
    rng = np.random.default_rng(3)
    rgba = rng.integers(0, 256, size=(len(faces), 4)).astype(np.uint8)
    rgba[:, 3] = np.where(rng.random(len(faces)) < 0.2, 0, 255)
    for f, c, nv in ((faces, rgba, V), fan_case(), (np.array([[0, 1, 2], [2, 1, 4]], np.int32), np.array([[9, 8, 7, 255], [1, 2, 4, 0]], np.uint8), 6)):
        got = ref.face_to_vertex_colors(f, c, nv)
        inc = np.zeros((nv, len(f)), np.float64)
        for k in range(3):
            np.add.at(inc, (f[:, k], np.arange(len(f))), 1.0)
        inc[:, c[:, 3] == 0] = 0.0
        count = inc.sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            mean = (inc @ c[:, :3].astype(np.float64)) / count[:, None]
        want = np.where(count[:, None] > 0, mean, 0.0).astype(np.uint8)               # (the cast truncates: the floor of a mean >= 0)
        assert np.array_equal(got[:, :3], want)
        assert np.array_equal(got[:, 3], np.where(count > 0, 255, 0))
    fan = ref.face_to_vertex_colors(*fan_case())
    assert fan[0].tolist() == [255, 255, 255, 255]
    assert ref.face_to_vertex_colors(np.array([[0, 1, 2]], np.int32), np.array([[3, 4, 5, 255]], np.uint8), 5)[3:].tolist() == [[0] * 4] * 2


@pytest.mark.parametrize("G", GS)
def test_sh_dc_against_torch(G):
    """sugar_model.py:236-240 and :386 on the CPU, in torch, as the reference writes them."""
    C0 = 0.28209479177387814
    rng = np.random.default_rng(20 + G)
    _bv, bf, _fv, _ff, _raw = chain_case()
    V = int(bf.max()) + 1
    for col in (rng.random((V, 3)), np.zeros((V, 3)), np.ones((V, 3)), rng.random((V, 4))):
        vertex_colors = torch.tensor(np.array(col[:, :3])).float()
        faces = torch.from_numpy(bf.astype(np.int64))
        bary = torch.tensor(ref.BARY_COORDS[G], dtype=torch.float32)[..., None]
        faces_colors = vertex_colors[faces]
        colors = faces_colors[:, None] * bary[None]
        colors = colors.sum(dim=-2)
        colors = colors.reshape(-1, 3)
        want = ((colors - 0.5) / C0).numpy()
        got = ref.sh_dc_from_vertex_colors(bf, col, G)
        assert got.dtype == np.float32 and got.shape == (len(bf) * G, 3)
        assert got.tobytes() == want.tobytes()
    x = torch.full((1,), 0.1, dtype=torch.float32)
    assert np.float32(ref.from_mesh(bf, col, G)["density"]).tobytes() == torch.log(x / (1 - x)).numpy().tobytes()


# ---------------------------------------------------------------------------------------------------- face_origin
@functools.lru_cache(maxsize=None)
def origin_want(gap=False):
    bv, bf, fv, ff, raw = chain_case()
    if gap:
        ff = np.delete(ff, GAP_FACE, axis=0)
    return ref.update_mesh_topology(bv, bf, 2, rr.padded_boxes(raw, 0.02), fv, ff), ff


@pytest.mark.parametrize("gap", [False, True])
def test_face_origin_invariants(gap):
    bv, bf, fv, _ff, raw = chain_case()
    want, ff = origin_want(gap)
    plain = chain_want() if not gap else splice_ref.update_mesh_topology(bv, bf, 2, rr.padded_boxes(raw, 0.02), fv, ff)
    # the loop with origins is the loop without
    assert np.array_equal(want["faces"], plain["faces"]) and want["verts"].tobytes() == plain["verts"].tobytes()
    assert np.array_equal(want["track_face_mask"], plain["track_face_mask"]) and want["n_spliced"] == plain["n_spliced"] == 2
    o = want["face_origin"]
    tn = int(want["track_face_mask"].sum())
    assert o.dtype == np.int32 and o.shape == (len(want["faces"]),)
    assert np.array_equal(o[:tn], np.nonzero(want["track_face_mask"])[0]) and (o[tn:] < 0).all()
    filled = o == ref.FILLED
    fusion = -1 - o[(o < 0) & ~filled].astype(np.int64)
    assert len(fusion) > 100 and fusion.min() >= 0 and fusion.max() < len(ff) and len(np.unique(fusion)) == len(fusion)
    print("filled faces:", int(filled.sum()), "fills made:", want["n_fills_made"])
    assert int(filled.sum()) == want["n_fills_made"] and (int(filled.sum()) > 0) == gap
    # a fusion face of the result is the fusion face its origin names: the same three positions, unless the stitch moved one
    idx = np.nonzero((o < 0) & ~filled)[0]
    got_tri = want["verts"][want["faces"][idx]]
    src_tri = fv[ff[fusion]]
    same = (got_tri == src_tri).all(axis=(1, 2))
    assert same.sum() > len(idx) // 2


def test_with_colors_restatement():
    bv, bf, fv, _ff, _raw = chain_case()
    want, ff = origin_want(True)
    rng = np.random.default_rng(8)
    base = rng.integers(0, 256, size=(len(bf), 4)).astype(np.uint8)
    base[:, 3] = 255
    fcol = rng.random((len(fv), 3)).astype(np.float32)
    fc, vc = ref.with_colors(want, base, ff, fcol)
    o = want["face_origin"]
    tn = int(want["track_face_mask"].sum())
    assert np.array_equal(fc[:tn], base[want["track_face_mask"]])
    assert (fc[o == ref.FILLED] == 0).all() and (fc[o != ref.FILLED][:, 3] == 255).all()
    assert (vc[:, 3] == 255).all()                                     # every vertex has a coloured face, the filled rims' too
    # a default colour on the filled faces would have tinted their vertices
    tinted = fc.copy()
    tinted[o == ref.FILLED] = [102, 102, 102, 255]
    assert not np.array_equal(ref.face_to_vertex_colors(want["faces"], tinted, len(want["verts"])), vc)


# ---------------------------------------------------------------------------------------------------- files, prefixes (no GPU)
def _update_of(want, **kw):
    from gaustar_amd import regions
    t = torch.from_numpy
    plain = chain_want()
    return regions.TopologyUpdate(verts=t(plain["verts"]), faces=t(plain["faces"]), track_face_mask=t(plain["track_face_mask"]),
                                  track_face_num=plain["track_face_num"], new_ref_area=t(plain["new_ref_area"]),
                                  new_area_mean=plain["new_area_mean"], cc_update_num=2, n_spliced=2,
                                  max_dist_in_connection=plain["max_dist_in_connection"], nothing_to_update=False, **kw)


def test_save_with_colours_and_load_tracking(tmp_path):
    from gaustar_amd import formats, regions
    bv, bf, fv, ff, _raw = chain_case()
    want, _ff = origin_want(False)
    rng = np.random.default_rng(9)
    base = rng.integers(0, 256, size=(len(bf), 4)).astype(np.uint8)
    _fc, vc = ref.with_colors(want, base, ff, rng.random((len(fv), 3)).astype(np.float32))
    upd = _update_of(want)
    assert upd.face_origin is None and upd.face_colors is None and upd.vertex_colors is None      # new fields, with defaults
    plain_obj, _npz = upd.save(str(tmp_path / "plain"))
    assert formats.load_obj(plain_obj)[2] is None                       # without colours: the file as before
    upd.vertex_colors = torch.from_numpy(vc)
    obj, npz = upd.save(str(tmp_path / "coloured"))
    v, f, c = formats.load_obj(obj)
    assert np.array_equal(f, want["faces"]) and v.astype(np.float32).tobytes() == want["verts"].tobytes()
    assert c.shape == (len(v), 3) and np.array_equal(c, vc[:, :3].astype(np.float64) / 255.0)
    assert np.array_equal(ref.unit_to_u8(c), vc[:, :3])                 # u8 / 255 reads back as the same u8
    first = open(obj).readline().split()
    assert first[0] == "v" and len(first) == 7
    mask, area = regions.load_tracking(npz)
    assert mask.dtype == np.bool_ and np.array_equal(mask, want["track_face_mask"])
    assert area.dtype == np.float32 and np.array_equal(area, chain_want()["new_ref_area"])
    with pytest.raises(ValueError):
        upd.with_colors(torch.zeros(len(bf), 4, dtype=torch.uint8), torch.zeros(len(fv), 3))      # no face_origin


def test_tracked_pre_sh():
    from gaustar_amd import harness
    rng = np.random.default_rng(4)
    F0, G, K = 12, 3, 4
    sd = {"_sh_coordinates_dc": torch.from_numpy(rng.normal(size=(F0 * G, 1, 3)).astype(np.float32)),
          "_sh_coordinates_rest": torch.from_numpy(rng.normal(size=(F0 * G, K - 1, 3)).astype(np.float32)), "_points": torch.zeros(3, 3)}
    full = torch.cat([sd["_sh_coordinates_dc"], sd["_sh_coordinates_rest"]], dim=1)
    dc, sh = harness.tracked_pre_sh(sd, G=G)
    assert torch.equal(sh, full) and torch.equal(dc, full[:, 0]) and dc.is_contiguous()
    mask = rng.random(F0) < 0.5
    for m in (mask, torch.from_numpy(mask)):
        dc, sh = harness.tracked_pre_sh({"state_dict": sd, "epoch": 3}, m, G)
        keep = np.repeat(mask, G)                                       # refine.py:382: every face's G Gaussians together
        assert tuple(sh.shape) == (int(mask.sum()) * G, K, 3) and torch.equal(sh, full[torch.from_numpy(keep)])
        assert torch.equal(dc, sh[:, 0])
    with pytest.raises(ValueError):
        harness.tracked_pre_sh(sd, mask, G=6)


def test_from_mesh_needs_colours():
    from gaustar_amd import harness
    v, f = splice_ref.icosahedron()
    with pytest.raises(ValueError):
        harness.SurfaceGaussians.from_mesh(v, f, None)
