"""A numpy-only restatement of the stitch in gaustar_amd.regions (connect_two_meshes, gaustar_trainers/refined_mesh.py:158-215,
with reset_duplicate_vert :114-123 and merge_vert_around_holes :126-155; the watertight test :639), term by term: what
knn_points, trimesh and scipy compute there, written out with plain arrays, dictionaries and a plain union-find.  float64
arithmetic goes through separate ufuncs, so nothing is fused.  Every result is an integer or an exactly defined float, so the
GPU tests compare with np.array_equal."""
import numpy as np

import regions_ref


# ---------------------------------------------------------------------------------------------------- meshes for the tests
def torus(nu, nv, R=2.0, r=1.0):
    """A closed nu x nv quad grid with wrap-around indices, two triangles per quad: (verts [nu nv,3] f32, faces [2 nu nv,3]
    int32).  Vertex (i, j) is j nu + i; quad (i, j)'s faces are 2 (j nu + i) and the next."""
    u = 2 * np.pi * np.arange(nu) / nu
    v = 2 * np.pi * np.arange(nv) / nv
    uu, vv = np.meshgrid(u, v)                      # [nv, nu]
    x = (R + r * np.cos(vv)) * np.cos(uu)
    y = (R + r * np.cos(vv)) * np.sin(uu)
    z = r * np.sin(vv)
    verts = np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], 1).astype(np.float32)
    idx = lambda i, j: (j % nv) * nu + (i % nu)
    faces = []
    for j in range(nv):
        for i in range(nu):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return verts, np.asarray(faces, np.int32).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------- a. nearest vertex
def nearest_vertices(queries, candidates, rows=256):
    """(idx int32 [Bq], d2 float64 [Bq]): the minimum of (d2, index), d2 = (dx dx + dy dy) + dz dz in float64 on the widened
    f32 coordinates.  np.argmin returns the first minimum: the lowest index among equals."""
    q = np.asarray(queries, np.float32).astype(np.float64).reshape(-1, 3)
    c = np.asarray(candidates, np.float32).astype(np.float64).reshape(-1, 3)
    idx = np.zeros(len(q), np.int32)
    d2 = np.zeros(len(q), np.float64)
    for s in range(0, len(q), rows):
        p = q[s:s + rows]
        dx = np.subtract(p[:, None, 0], c[None, :, 0])
        dy = np.subtract(p[:, None, 1], c[None, :, 1])
        dz = np.subtract(p[:, None, 2], c[None, :, 2])
        d = np.add(np.add(np.multiply(dx, dx), np.multiply(dy, dy)), np.multiply(dz, dz))
        k = np.argmin(d, axis=1)
        idx[s:s + rows] = k
        d2[s:s + rows] = d[np.arange(len(p)), k]
    return idx, d2


# ---------------------------------------------------------------------------------------------------- b. groups by position
def position_remap(verts, listed):
    """reset_duplicate_vert (:114-123) as a vertex map [V] int32: the identity, but every listed vertex -> the listed vertex
    earliest in the list among those at its position.  Equal = the three coordinates compare equal as numbers (-0 == +0,
    NaN equals nothing)."""
    verts = np.asarray(verts, np.float32)
    remap = np.arange(len(verts), dtype=np.int32)
    first = {}
    for k, v in enumerate(np.asarray(listed).reshape(-1)):
        p = verts[v]
        key = ("nan", k) if np.isnan(p).any() else tuple(float(x) + 0.0 for x in p)
        first.setdefault(key, int(v))
        remap[v] = first[key]
    return remap


# ---------------------------------------------------------------------------------------------------- c. degenerate faces
def select_faces(verts, faces, face_mask, attrs=()):
    """update_faces + remove_unreferenced_vertices: dict(verts, faces int32, face_mask, vert_map [V] int32, attrs)."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    keep = np.asarray(face_mask, bool)
    used = np.zeros(len(verts), bool)
    used[faces[keep].reshape(-1)] = True
    vert_map = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    return dict(verts=verts[used], faces=vert_map[faces[keep]].astype(np.int32).reshape(-1, 3), face_mask=keep, vert_map=vert_map,
                attrs=tuple(np.asarray(a)[used] for a in attrs))


def nondegenerate(faces):
    """[F] bool: the three indices differ (nondegenerate_faces without the height test)."""
    f = np.asarray(faces).reshape(-1, 3)
    return (f[:, 0] != f[:, 1]) & (f[:, 1] != f[:, 2]) & (f[:, 2] != f[:, 0])


# ---------------------------------------------------------------------------------------------------- d. holes
def hole_components(faces):
    """(hole_verts ascending, label per hole vertex): the ends of the face-edges whose vertex pair occurs other than exactly
    twice (:129-133), and their components under those edges numbered by ascending lowest vertex (:142)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if len(f) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    edges = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1)
    hole_edges = edges[regions_ref.face_edge_counts(f) != 2]
    hole_verts = np.unique(hole_edges.reshape(-1))
    parent = {int(v): int(v) for v in hole_verts}

    def find(x):
        while parent[x] != x:
            x = parent[x]
        return x

    for a, b in hole_edges:
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    roots = np.array([find(int(v)) for v in hole_verts], np.int64)
    _, label = np.unique(roots, return_inverse=True)
    return hole_verts, label


def merge_vertices_around_holes(verts, faces, max_hole_vert_num=10):
    """merge_vert_around_holes (:126-155) and the degenerate pass after it (:201-203): select_faces' dict, vert_map with merged
    vertices at their representative's new index."""
    verts = np.asarray(verts, np.float32).copy()
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    hole_verts, label = hole_components(faces)
    for h in range(int(label.max()) + 1 if len(label) else 0):
        members = hole_verts[label == h]
        if len(members) > max_hole_vert_num:
            continue
        verts[members] = verts[members.min()]
    remap = position_remap(verts, hole_verts)
    faces = remap[faces] if len(faces) else faces
    out = select_faces(verts, faces, nondegenerate(faces))
    out["vert_map"] = out["vert_map"][remap]
    return out


# ---------------------------------------------------------------------------------------------------- e. watertight
def is_watertight(faces):
    f = np.asarray(faces).reshape(-1, 3)
    return bool(len(f) > 0 and (regions_ref.face_edge_counts(f) == 2).all())


# ---------------------------------------------------------------------------------------------------- connect_two_meshes
def connect_two_meshes(verts1, faces1, boundary1, verts2, faces2, boundary2, max_hole_vert_num=10):
    """connect_two_meshes (:158-215): dict(verts, faces, face_mask [F1+F2], vert_map [V1+V2], n_faces_from_first, max_dist,
    watertight)."""
    v1, v2 = np.asarray(verts1, np.float32).copy(), np.asarray(verts2, np.float32).copy()
    f1, f2 = np.asarray(faces1, np.int64).reshape(-1, 3), np.asarray(faces2, np.int64).reshape(-1, 3)
    b1, b2 = np.asarray(boundary1, np.int64), np.asarray(boundary2, np.int64)
    V1 = len(v1)
    pc1, pc2 = v1[b1], v2[b2]
    n21, d21 = nearest_vertices(pc2, pc1)                                   # :166
    v2[b2] = pc1[n21]                                                       # :171
    pc2 = v2[b2]
    n12, d12 = nearest_vertices(pc1, pc2)                                   # :175
    v1[b1] = pc2[n12]                                                       # :178
    vert = np.concatenate([v1, v2])
    face = np.concatenate([f1, f2 + V1])
    remap1 = position_remap(vert, np.concatenate([b1, b2 + V1]))           # :188
    face = remap1[face]
    keep1 = nondegenerate(face)                                             # :193
    m1 = select_faces(vert, face, keep1)                                    # :194-195
    m2 = merge_vertices_around_holes(m1["verts"], m1["faces"], max_hole_vert_num)   # :198-203
    face_mask = keep1.copy()
    face_mask[keep1] = m2["face_mask"]                                      # :205-206
    a = m1["vert_map"][remap1]
    vert_map = np.where(a < 0, -1, m2["vert_map"][np.maximum(a, 0)] if len(m2["vert_map"]) else -1).astype(np.int32)
    max_dist = float(np.sqrt(np.maximum(d21.max(), d12.max())))            # :211
    return dict(verts=m2["verts"], faces=m2["faces"], face_mask=face_mask, vert_map=vert_map,
                n_faces_from_first=int(face_mask[:len(f1)].sum()), max_dist=max_dist, watertight=is_watertight(m2["faces"]))
