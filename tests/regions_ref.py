"""A numpy-only restatement of gaustar_amd.regions (the front half of update_mesh_topo, gaustar_trainers/refined_mesh.py:463-693):
what trimesh, scipy and numpy compute there, written out with plain arrays and a plain union-find.  Vertex identity is the
vertex index.  Every result is an integer or an exactly defined float, so the GPU tests compare with np.array_equal."""
import numpy as np


# ---------------------------------------------------------------------------------------------------- meshes for the tests
def quad_grid(nx, ny, v0=0):
    """An nx x ny grid of quads, two triangles each: (verts [(nx+1)(ny+1),3] f32 in the z = 0 plane, faces [2 nx ny,3] int32,
    vertex numbers starting at v0).  Quad (i, j)'s faces are 2 (j nx + i) and the next."""
    xs, ys = np.meshgrid(np.arange(nx + 1), np.arange(ny + 1))
    verts = np.stack([xs.reshape(-1), ys.reshape(-1), np.zeros(xs.size)], 1).astype(np.float32)
    idx = lambda i, j: v0 + j * (nx + 1) + i
    faces = []
    for j in range(ny):
        for i in range(nx):
            a, b, c, d = idx(i, j), idx(i + 1, j), idx(i + 1, j + 1), idx(i, j + 1)
            faces += [(a, b, c), (a, c, d)]
    return verts, np.asarray(faces, np.int32).reshape(-1, 3)


# ---------------------------------------------------------------------------------------------------- 1. edge multiplicity
def face_edges(faces):
    """[F,3,2]: face-edge e of (a, b, c) is (a, b), (b, c), (c, a) (trimesh faces_to_edges), each sorted to (min, max)."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    e = np.stack([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], 1)
    return np.sort(e, axis=2)


def face_edge_counts(faces, mask=None):
    """[F,3] int32: the face-edges of the (masked) mesh with the same vertex pair; 0 outside the mask."""
    e = face_edges(faces)
    F = e.shape[0]
    m = np.ones(F, bool) if mask is None else np.asarray(mask, bool)
    seen = {}
    for f in range(F):
        if m[f]:
            for k in range(3):
                key = (int(e[f, k, 0]), int(e[f, k, 1]))
                seen[key] = seen.get(key, 0) + 1
    out = np.zeros((F, 3), np.int32)
    for f in range(F):
        if m[f]:
            for k in range(3):
                out[f, k] = seen[(int(e[f, k, 0]), int(e[f, k, 1]))]
    return out


def face_adjacency(faces, mask=None):
    """The pairs of different (masked) faces that share an edge exactly two face-edges have."""
    e = face_edges(faces)
    F = e.shape[0]
    m = np.ones(F, bool) if mask is None else np.asarray(mask, bool)
    owners = {}
    for f in range(F):
        if m[f]:
            for k in range(3):
                owners.setdefault((int(e[f, k, 0]), int(e[f, k, 1])), []).append(f)
    return [(o[0], o[1]) for o in owners.values() if len(o) == 2 and o[0] != o[1]]


# ---------------------------------------------------------------------------------------------------- 2. components
def face_components(faces, mask=None):
    """(label [F] int32, count [n] int32): components of face_adjacency, numbered by ascending smallest face; -1 outside."""
    F = np.asarray(faces).reshape(-1, 3).shape[0]
    m = np.ones(F, bool) if mask is None else np.asarray(mask, bool)
    parent = list(range(F))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for a, b in face_adjacency(faces, m):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    label = np.full(F, -1, np.int32)
    number = {}
    for f in range(F):          # ascending f: a component is numbered when its smallest face comes by
        if m[f]:
            r = find(f)
            if r not in number:
                number[r] = len(number)
            label[f] = number[r]
    count = np.bincount(label[label >= 0], minlength=len(number)).astype(np.int32)
    return label, count


# ---------------------------------------------------------------------------------------------------- 3. / 4. selection, boxes
def inside_box(points, box):
    """find_points_in_boundingbox (:218-224) in float64: strictly between the bounds on every axis."""
    p = np.asarray(points, np.float64)
    b = np.asarray(box, np.float64)
    return ((p > b[0]) & (p < b[1])).all(axis=1)


def combine_overlap_aabbs(boxes):
    """combine_overlap_aabbs (:254-288).  The i-th merged entry is tested through the i-th box of the INPUT list."""
    boxes = [np.asarray(b, np.float64) for b in boxes]
    merged = []
    for b in boxes:
        corners = np.array([[b[i, 0], b[j, 1], b[k, 2]] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
        target = None
        for i in range(len(merged)):
            if inside_box(corners, boxes[i]).any():
                target = i
                break
        if target is None:
            merged.append(b.copy())
        else:
            merged[target] = np.stack([np.minimum(merged[target][0], b[0]), np.maximum(merged[target][1], b[1])])
    if len(merged) == len(boxes):
        return merged
    return combine_overlap_aabbs(merged)


def select_update_regions(verts, faces, points, face_colour, G, delta_threshold=0.6, cc_face_threshold=80):
    """dict(component [F], region [F], n_components, labels [n], counts [n], raw_boxes float64 [n,2,3])."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces).reshape(-1, 3)
    F = faces.shape[0]
    pts = np.asarray(points, np.float32).reshape(F, G, 3)
    mask = np.asarray(face_colour).astype(np.float64) >= 255 * delta_threshold          # :516
    component, count = face_components(faces, mask)
    labels = np.where(count > cc_face_threshold)[0].astype(np.int32)                   # :526
    region = np.full(F, -1, np.int32)
    boxes = np.zeros((len(labels), 2, 3))
    for r, lab in enumerate(labels):
        of = component == lab
        region[of] = r
        cloud = np.concatenate([verts[faces[of].reshape(-1)], pts[of].reshape(-1, 3)], 0) + np.float32(0)   # (-0 -> +0)
        boxes[r, 0], boxes[r, 1] = cloud.min(0), cloud.max(0)                          # :561-567, before the pad
    return dict(component=component, region=region, n_components=len(count), labels=labels, counts=count[labels], raw_boxes=boxes)


def padded_boxes(raw_boxes, aabb_pad):
    """float64 [m,2,3]: :568-569 and :574."""
    grown = np.asarray(raw_boxes, np.float64).copy()
    grown[:, 0] -= aabb_pad
    grown[:, 1] += aabb_pad
    out = combine_overlap_aabbs(list(grown))
    return np.stack(out) if out else np.zeros((0, 2, 3))


# ---------------------------------------------------------------------------------------------------- 5. cut
def cut_mesh_by_box(verts, faces, box, cut_inner, attrs=()):
    """cut_mesh_by_boundingbox (:227-251): dict(verts, faces int32, face_mask [F] bool, vert_map [V] int32, attrs)."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    ins = inside_box(verts, box)
    any_in = ins[faces].any(axis=1) if len(faces) else np.zeros(0, bool)
    keep = ~any_in if cut_inner else any_in
    used = np.zeros(len(verts), bool)
    used[faces[keep].reshape(-1)] = True
    vert_map = np.where(used, np.cumsum(used) - 1, -1).astype(np.int32)
    return dict(verts=verts[used], faces=vert_map[faces[keep]].astype(np.int32).reshape(-1, 3), face_mask=keep, vert_map=vert_map,
                attrs=tuple(np.asarray(a)[used] for a in attrs))


# ---------------------------------------------------------------------------------------------------- 6. / 7. primitives
def boundary_vertices(verts, faces, box=None, cut_inner=False, pad=0.02):
    """find_boundary_verts (:84-111): ascending int32 indices."""
    verts = np.asarray(verts, np.float32)
    faces = np.asarray(faces, np.int64).reshape(-1, 3)
    e = face_edges(faces)
    on = np.zeros(len(verts), bool)
    on[e[face_edge_counts(faces) == 1].reshape(-1)] = True
    if box is not None:
        b = np.asarray(box, np.float64)
        if cut_inner:
            on &= inside_box(verts, np.stack([b[0] - pad, b[1] + pad]))
        else:
            k = inside_box(verts, b)[faces].sum(axis=1) if len(faces) else np.zeros(0, int)
            across = np.zeros(len(verts), bool)
            across[faces[(k > 0) & (k < 3)].reshape(-1)] = True
            on &= across
    return np.where(on)[0].astype(np.int32)


def outlier_component_mask(faces, face_num_threshold=None):
    """get_outlier_cc_mask (:291-307): [F] bool."""
    label, count = face_components(faces)
    if len(label) == 0:
        return np.zeros(0, bool)
    bound = count.max() * 0.3
    if face_num_threshold is not None:
        bound = np.minimum(face_num_threshold, bound)
    return np.isin(label, np.where(count >= bound)[0])
