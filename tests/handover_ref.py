"""A numpy-only restatement of gaustar_amd.handover and of the colour bookkeeping of gaustar_amd.regions.update_mesh_topology:
the five passes of gsr_handover.hip, TopologyUpdate.face_origin / with_colors and harness.SurfaceGaussians.from_mesh.  Every
float step is a separate ufunc on float32 arrays, so nothing is fused and every operation rounds on its own; integers are
exact.  The loop over the boxes repeats splice_ref.update_mesh_topology's (pinned by tests/test_splice.py) with one array more,
the origin of every face, and tests/test_handover.py checks that the two loops give the same mesh."""
import numpy as np

import regions_ref as rr
import splice_ref
import stitch_ref as sr

C0 = np.float32(0.28209479177387814)
FILLED = np.int32(-2 ** 31)
BARY_COORDS = {   # gaustar_scene/sugar_model.py:186-226, as gaustar_amd.harness.BARY_COORDS holds them
    1: [[1 / 3, 1 / 3, 1 / 3]],
    3: [[1 / 2, 1 / 4, 1 / 4], [1 / 4, 1 / 2, 1 / 4], [1 / 4, 1 / 4, 1 / 2]],
    4: [[1 / 3, 1 / 3, 1 / 3], [2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3]],
    6: [[2 / 3, 1 / 6, 1 / 6], [1 / 6, 2 / 3, 1 / 6], [1 / 6, 1 / 6, 2 / 3], [1 / 6, 5 / 12, 5 / 12], [5 / 12, 1 / 6, 5 / 12],
        [5 / 12, 5 / 12, 1 / 6]],
}


def _rgba(rgb):
    rgb = np.asarray(rgb).reshape(-1, 3)
    return np.concatenate([rgb, np.full((len(rgb), 1), 255)], axis=1).astype(np.uint8)


# ---------------------------------------------------------------------------------------------------- 1a
def sh_face_colors(sh_dc, G):
    """[F,4] uint8.  m = (((x0 + x1) + ...) + x_{G-1}) / G, c = (m C0 + 0.5) 255, truncation toward zero, clip."""
    x = np.asarray(sh_dc, np.float32).reshape(-1, G, 3)
    s = x[:, 0].copy()
    for g in range(1, G):
        s = np.add(s, x[:, g])
    m = np.divide(s, np.float32(G))
    c = np.multiply(np.add(np.multiply(m, C0), np.float32(0.5)), np.float32(255.0))
    assert c.dtype == np.float32
    return _rgba(np.clip(np.trunc(c).astype(np.int64), 0, 255))


def rgb_to_sh(rgb):
    """RGB2SH on float32: (rgb - 0.5) / C0."""
    return np.divide(np.subtract(np.asarray(rgb, np.float32), np.float32(0.5)), C0)


# ---------------------------------------------------------------------------------------------------- 1b
def unit_to_u8(c):
    """clip(rint(255 c), 0, 255) on float32, ties to even."""
    return np.clip(np.rint(np.multiply(np.asarray(c, np.float32), np.float32(255.0))), 0, 255).astype(np.int64)


def vertex_to_face_colors(faces, vertex_colors):
    """[F,4] uint8: the floor of the integer mean of the three vertices' uint8 colours."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    u = unit_to_u8(np.asarray(vertex_colors)[:, :3])
    return _rgba((u[f[:, 0]] + u[f[:, 1]] + u[f[:, 2]]) // 3)


# ---------------------------------------------------------------------------------------------------- 1c
def face_to_vertex_colors(faces, face_rgba, n_verts):
    """[V,4] uint8: per vertex the floor of the integer mean over its incident faces with alpha != 0 (a face that names the
    vertex twice counts twice); none: (0, 0, 0, 0).  A Python loop over the face corners."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    rgba = np.asarray(face_rgba, np.uint8).reshape(-1, 4)
    total = [[0, 0, 0] for _ in range(n_verts)]
    count = [0] * n_verts
    for t, c in zip(f.tolist(), rgba.tolist()):
        if c[3] == 0:
            continue
        for v in t:
            count[v] += 1
            for k in range(3):
                total[v][k] += c[k]
    out = np.zeros((n_verts, 4), np.uint8)
    for v in range(n_verts):
        if count[v]:
            out[v] = [total[v][0] // count[v], total[v][1] // count[v], total[v][2] // count[v], 255]
    return out


# ---------------------------------------------------------------------------------------------------- 1d
def sh_dc_from_vertex_colors(faces, vertex_colors, G):
    """[F G,3] float32: c = (b_g0 v0 + b_g1 v1) + b_g2 v2, dc = (c - 0.5) / C0."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    col = np.asarray(vertex_colors)[:, :3].astype(np.float32)
    bary = np.asarray(BARY_COORDS[G], np.float64).astype(np.float32)                  # [G,3]
    p = [np.multiply(bary[None, :, k, None], col[f[:, k]][:, None, :]) for k in range(3)]   # [F,G,3] each
    c = np.add(np.add(p[0], p[1]), p[2])
    assert c.dtype == np.float32
    return rgb_to_sh(c).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------- 1e
def gather_face_colors(origin, base_rgba, fusion_faces, fusion_vertex_colors):
    origin = np.asarray(origin, np.int64)
    base_rgba = np.asarray(base_rgba, np.uint8).reshape(-1, 4)
    fusion_rgba = vertex_to_face_colors(fusion_faces, fusion_vertex_colors)
    out = np.zeros((len(origin), 4), np.uint8)
    for i, o in enumerate(origin.tolist()):
        if o >= 0:
            out[i] = base_rgba[o]
        elif o != int(FILLED):
            out[i] = fusion_rgba[-1 - o]
    return out


# ---------------------------------------------------------------------------------------------------- 2. the loop, with origins
def update_mesh_topology(verts, faces, n_regions, boxes, fusion_verts, fusion_faces, outlier_face_threshold=50, force_watertight=True,
                         max_hole_vert_num=10, pad=0.02):
    """splice_ref.update_mesh_topology's loop (force_short_edge off) with face_origin.  -> dict(verts, faces, track_face_mask,
    face_origin [Nf] int32, n_fills_made: the faces fill_small_holes made in the boxes that were spliced, at its three places,
    n_spliced, cc_update_num)."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int32).reshape(-1, 3)
    fusion_verts, fusion_faces = np.asarray(fusion_verts, np.float32), np.asarray(fusion_faces, np.int32).reshape(-1, 3)
    F0 = len(faces)
    base_v, base_f = verts, faces
    origin = np.arange(F0, dtype=np.int64)
    track = np.ones(F0, bool)
    if n_regions == 0:
        return dict(verts=verts, faces=faces, track_face_mask=track, face_origin=origin.astype(np.int32), n_fills_made=0, n_spliced=0,
                    cc_update_num=-1)
    run = lambda n: np.full(n, int(FILLED), np.int64)
    failed = n_spliced = n_fills_made = 0
    for box in boxes:
        patch = rr.cut_mesh_by_box(fusion_verts, fusion_faces, box, False)
        if len(patch["verts"]) == 0:
            failed += 1
            continue
        pfill = splice_ref.fill_small_holes(patch["faces"])
        p_origin = np.concatenate([-1 - np.nonzero(patch["face_mask"])[0], run(pfill["n_new"])])
        p_keep = rr.outlier_component_mask(pfill["faces"], outlier_face_threshold)
        patch = sr.select_faces(patch["verts"], pfill["faces"], p_keep)
        p_origin = p_origin[np.asarray(p_keep, bool)]
        pb = rr.boundary_vertices(patch["verts"], patch["faces"], box, cut_inner=False)
        if len(pb) == 0:
            failed += 1
            continue
        cut = rr.cut_mesh_by_box(base_v, base_f, box, True)
        if len(cut["verts"]) == 0:
            failed += 1
            continue
        n_cut = len(cut["faces"])
        cfill = splice_ref.fill_small_holes(cut["faces"])
        bb = rr.boundary_vertices(cut["verts"], cfill["faces"], box, cut_inner=True, pad=pad)
        if len(bb) == 0:
            failed += 1
            continue
        st = sr.connect_two_meshes(cut["verts"], cfill["faces"], bb, patch["verts"], patch["faces"], pb, max_hole_vert_num)
        if force_watertight and not st["watertight"]:
            continue
        sfill = splice_ref.fill_small_holes(st["faces"])
        both = np.concatenate([origin[cut["face_mask"]], run(cfill["n_new"]), p_origin])
        origin = np.concatenate([both[np.asarray(st["face_mask"], bool)], run(sfill["n_new"])])
        mask_cc = cut["face_mask"].copy()
        mask_cc[cut["face_mask"]] = st["face_mask"][:n_cut]
        base_v, base_f = st["verts"], sfill["faces"]
        tn = int(track.sum())
        track[track] = mask_cc[:tn]
        n_spliced += 1
        n_fills_made += pfill["n_new"] + cfill["n_new"] + sfill["n_new"]
    assert len(origin) == len(base_f)
    return dict(verts=base_v, faces=base_f, track_face_mask=track, face_origin=origin.astype(np.int32),
                n_fills_made=n_fills_made, n_spliced=n_spliced, cc_update_num=n_regions - failed)


def with_colors(update, base_face_rgba, fusion_faces, fusion_vertex_colors):
    """(face_colors [Nf,4], vertex_colors [Nv,4]) uint8 of an update_mesh_topology result."""
    fc = gather_face_colors(update["face_origin"], base_face_rgba, fusion_faces, fusion_vertex_colors)
    return fc, face_to_vertex_colors(update["faces"], fc, len(update["verts"]))


# ---------------------------------------------------------------------------------------------------- 3. from_mesh
def inverse_sigmoid_f32(p):
    x = np.float32(p)
    return np.log(np.divide(x, np.subtract(np.float32(1.0), x)))


def from_mesh(faces, vertex_colors, G=6, initial_opacity=0.1):
    """dict(sh_dc [F G,3] f32, density: the f32 value every Gaussian's all_densities starts at)."""
    return dict(sh_dc=sh_dc_from_vertex_colors(faces, vertex_colors, G), density=inverse_sigmoid_f32(initial_opacity))
