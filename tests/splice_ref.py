"""A numpy-only restatement of the back end of gaustar_amd.regions: fill_small_holes (this project's canonical rule for
trimesh's fill_holes, gaustar_trainers/refined_mesh.py:589, :617, :652), the loop of update_mesh_topo over the boxes with its
chaining (:578-664), cc_update_num (:666-681), the reference areas (:683-687) and the choice among the aabb_pad trials
(:1033-1060).  Plain dictionaries and Python loops over regions_ref and stitch_ref; nothing here knows of neighbour slots or of a
union-find.  Integers and masks are exact; areas are float64 through separate ufuncs, so nothing is fused."""
import math

import numpy as np

import regions_ref as rr
import stitch_ref as sr


# ---------------------------------------------------------------------------------------------------- meshes for the tests
def icosahedron():
    """(verts [12,3] f32, faces [20,3] int32), outward winding, closed."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, t, 0], [1, t, 0], [-1, -t, 0], [1, -t, 0], [0, -1, t], [0, 1, t], [0, -1, -t], [0, 1, -t],
                  [t, 0, -1], [t, 0, 1], [-t, 0, -1], [-t, 0, 1]], np.float64)
    f = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6],
                  [7, 1, 8], [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7],
                  [9, 8, 1]], np.int32)
    return (v / np.linalg.norm(v[0])).astype(np.float32), f


def icosphere(level, radius=1.0, centre=(0.0, 0.0, 0.0)):
    """The icosahedron subdivided `level` times (every face into four, midpoints pushed to the sphere): closed, 20 4^level
    faces, the children of a face in its place and order."""
    v, f = icosahedron()
    v = [tuple(float(c) for c in p) for p in v.astype(np.float64)]
    f = [tuple(int(i) for i in t) for t in f]
    for _ in range(level):
        mid = {}

        def midpoint(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                p = np.add(v[a], v[b]) / 2.0
                p = p / np.linalg.norm(p)
                mid[key] = len(v)
                v.append(tuple(p))
            return mid[key]

        nf = []
        for a, b, c in f:
            ab, bc, ca = midpoint(a, b), midpoint(b, c), midpoint(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    verts = (np.asarray(v, np.float64) * radius + np.asarray(centre, np.float64)).astype(np.float32)
    return verts, np.asarray(f, np.int32)


# ---------------------------------------------------------------------------------------------------- 1. the rule
def boundary_edges(faces, n_verts=None):
    """The face-edges of count exactly 1 as directed pairs (a, b), in face-edge order.  With n_verts, faces that hold an index
    outside [0, n_verts) are left out."""
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    if n_verts is not None:
        f = f[((f >= 0) & (f < n_verts)).all(axis=1)]
    if len(f) == 0:
        return []
    counts = rr.face_edge_counts(f)
    return [(int(f[i, e]), int(f[i, (e + 1) % 3])) for i in range(len(f)) for e in range(3) if counts[i, e] == 1]


def rim_components(faces):
    """[(sorted vertices, is_rim)] for every component of the boundary edges, taken undirected, in ascending lowest vertex.
    is_rim = every vertex ends exactly two boundary edges (a self-edge ends twice at its vertex)."""
    edges = boundary_edges(faces)
    ends, nbr = {}, {}
    for a, b in edges:
        ends[a] = ends.get(a, 0) + 1
        ends[b] = ends.get(b, 0) + 1
        nbr.setdefault(a, set()).add(b)
        nbr.setdefault(b, set()).add(a)
    seen, out = set(), []
    for v in sorted(nbr):
        if v in seen:
            continue
        comp, todo = [], [v]
        seen.add(v)
        while todo:
            u = todo.pop()
            comp.append(u)
            for w in nbr[u]:
                if w not in seen:
                    seen.add(w)
                    todo.append(w)
        out.append((sorted(comp), all(ends[u] == 2 for u in comp)))
    return out


def rim_census(faces):
    """(rims of 3, rims of 4, other components)."""
    comps = rim_components(faces)
    n3 = sum(1 for c, ok in comps if ok and len(c) == 3)
    n4 = sum(1 for c, ok in comps if ok and len(c) == 4)
    return n3, n4, len(comps) - n3 - n4


def _wound(a, b, c, directed):
    """(a, b, c), or (a, c, b) when the boundary face-edge between a and b runs a -> b in its own face."""
    return (a, c, b) if (a, b) in directed else (a, b, c)


def fill_small_holes(faces, tie_windings=False, test_second_edge=False):
    """dict(faces [F + n_new,3] int32, n_new, rim_of_new [n_new] int32, watertight).  The rule is stated in
    gaustar_amd.regions.fill_small_holes.  tie_windings / test_second_edge: two WRONG variants, for the tests that must tell
    them from the rule (B reversed whenever A is; the winding tested on the face's second edge)."""
    f = np.asarray(faces, np.int32).reshape(-1, 3)
    directed = set(boundary_edges(f))
    undirected = {}
    for a, b in directed:
        undirected.setdefault(a, set()).add(b)
        undirected.setdefault(b, set()).add(a)

    def wound(a, b, c):
        if test_second_edge:
            return (a, c, b) if (b, c) in directed else (a, b, c)
        return _wound(a, b, c, directed)

    new, rim = [], []
    for comp, ok in rim_components(f):
        if not ok or len(comp) not in (3, 4):
            continue
        m = comp[0]
        x, y = sorted(undirected[m])
        if len(comp) == 3:
            new.append(wound(m, x, y))
            rim.append(m)
            continue
        (o,) = [u for u in comp if u not in (m, x, y)]
        A = wound(m, x, o)
        B = wound(o, y, m)
        if tie_windings:
            B = (o, m, y) if A != (m, x, o) else (o, y, m)
        new += [A, B]
        rim += [m, m]
    out = np.concatenate([f, np.asarray(new, np.int32).reshape(-1, 3)]) if new else f.copy()
    return dict(faces=out, n_new=len(new), rim_of_new=np.asarray(rim, np.int32), watertight=sr.is_watertight(out))


# ---------------------------------------------------------------------------------------------------- 3. areas
def face_areas(verts, faces):
    """trimesh's area_faces: float64 [F]."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    f = np.asarray(faces, np.int64).reshape(-1, 3)
    tri = v[f]
    u = np.subtract(tri[:, 1], tri[:, 0])
    w = np.subtract(tri[:, 2], tri[:, 1])
    cx = np.subtract(np.multiply(u[:, 1], w[:, 2]), np.multiply(u[:, 2], w[:, 1]))
    cy = np.subtract(np.multiply(u[:, 2], w[:, 0]), np.multiply(u[:, 0], w[:, 2]))
    cz = np.subtract(np.multiply(u[:, 0], w[:, 1]), np.multiply(u[:, 1], w[:, 0]))
    s = np.add(np.add(np.multiply(cx, cx), np.multiply(cy, cy)), np.multiply(cz, cz))
    return np.multiply(0.5, np.sqrt(s))


def exact_mean(x):
    """The mean of float64 values with a correctly rounded sum (math.fsum): any summation order over n positive terms lies
    within a relative n 2^-53 of it."""
    x = np.asarray(x, np.float64)
    return float("nan") if len(x) == 0 else math.fsum(x.tolist()) / len(x)


def mean_edge_length(verts, faces):
    """:484-485: the mean length of the unique edges, float64."""
    v = np.asarray(verts, np.float32).astype(np.float64)
    e = np.unique(rr.face_edges(faces).reshape(-1, 2), axis=0)
    d = np.subtract(v[e[:, 0]], v[e[:, 1]])
    n = np.sqrt(np.add(np.add(np.multiply(d[:, 0], d[:, 0]), np.multiply(d[:, 1], d[:, 1])), np.multiply(d[:, 2], d[:, 2])))
    return exact_mean(n)


# ---------------------------------------------------------------------------------------------------- 3. the driver
def update_mesh_topology(verts, faces, n_regions, boxes, fusion_verts, fusion_faces, outlier_face_threshold=50, force_watertight=True,
                         force_short_edge=False, max_hole_vert_num=10, pad=0.02, cut_from_uncut=False):
    """:578-693 over the merged `boxes` of `n_regions` selected regions.  cut_from_uncut: a WRONG variant that cuts every box
    out of the input mesh instead of what the previous box left (no chaining), for the test that must tell the two apart."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int32).reshape(-1, 3)
    fusion_verts, fusion_faces = np.asarray(fusion_verts, np.float32), np.asarray(fusion_faces, np.int32).reshape(-1, 3)
    F0 = len(faces)
    base_v, base_f = verts, faces
    track = np.ones(F0, bool)
    if n_regions == 0:
        return dict(verts=verts, faces=faces, track_face_mask=track, track_face_num=F0, new_ref_area=None, new_area_mean=float("nan"),
                    cc_update_num=-1, n_spliced=0, max_dist_in_connection=0.0, nothing_to_update=True)
    edge_len = mean_edge_length(verts, faces) if force_short_edge else None
    failed, n_spliced, max_dist = 0, 0, 0.0
    for box in boxes:
        patch = rr.cut_mesh_by_box(fusion_verts, fusion_faces, box, False)                      # :583
        if len(patch["verts"]) == 0:
            failed += 1
            continue
        pf = fill_small_holes(patch["faces"])["faces"]                                          # :589
        patch = sr.select_faces(patch["verts"], pf, rr.outlier_component_mask(pf, outlier_face_threshold))   # :590-599
        pb = rr.boundary_vertices(patch["verts"], patch["faces"], box, cut_inner=False)         # :600
        if len(pb) == 0:
            failed += 1
            continue
        src_v, src_f = (verts, faces) if cut_from_uncut else (base_v, base_f)
        cut = rr.cut_mesh_by_box(src_v, src_f, box, True)                                       # :609
        if len(cut["verts"]) == 0:
            failed += 1
            continue
        n_cut = len(cut["faces"])
        cf = fill_small_holes(cut["faces"])["faces"]                                            # :617
        bb = rr.boundary_vertices(cut["verts"], cf, box, cut_inner=True, pad=pad)               # :619
        if len(bb) == 0:
            failed += 1
            continue
        st = sr.connect_two_meshes(cut["verts"], cf, bb, patch["verts"], patch["faces"], pb, max_hole_vert_num)   # :628
        max_dist = max(max_dist, st["max_dist"])                                                # :633
        if force_watertight and not st["watertight"]:                                           # :639
            continue
        if force_short_edge and st["max_dist"] > 6 * edge_len:                                  # :645
            continue
        filled = fill_small_holes(st["faces"])["faces"]                                         # :652
        mask_cc = cut["face_mask"].copy()                                                       # :656-658
        mask_cc[cut["face_mask"]] = st["face_mask"][:n_cut]
        base_v, base_f = st["verts"], filled                                                    # :660
        tn = int(track.sum())
        track[track] = mask_cc[:tn]                                                             # :663-664
        n_spliced += 1
    tn = int(track.sum())
    area = face_areas(base_v, base_f)                                                           # :683-687
    mean = exact_mean(area[tn:])
    ref_area = np.empty(len(base_f), np.float32)
    ref_area[:tn] = face_areas(verts, faces)[track].astype(np.float32)
    ref_area[tn:] = np.float32(mean)
    return dict(verts=base_v, faces=base_f, track_face_mask=track, track_face_num=tn, new_ref_area=ref_area, new_area_mean=mean,
                cc_update_num=n_regions - failed, n_spliced=n_spliced, max_dist_in_connection=float(max_dist), nothing_to_update=False)


def prefix_is_original(out_verts, out_faces, track_face_mask, verts, faces, boxes, pad=0.02):
    """Whether the surviving input faces are the prefix of out_faces, in their order.  A stitch moves only boundary vertices
    inside a box grown by `pad` (:94-99, :178), so every surviving face with no vertex inside a grown box must sit at its
    place in the prefix with its three positions bit for bit; the others, with at least the positions of the input mesh.
    -> (ok, the number of faces compared exactly)."""
    verts, faces = np.asarray(verts, np.float32), np.asarray(faces, np.int64).reshape(-1, 3)
    out_verts, out_faces = np.asarray(out_verts, np.float32), np.asarray(out_faces, np.int64).reshape(-1, 3)
    keep = np.asarray(track_face_mask, bool)
    tn = int(keep.sum())
    if tn > len(out_faces):
        return False, 0
    near = np.zeros(len(verts), bool)
    for b in boxes:
        b = np.asarray(b, np.float64)
        near |= rr.inside_box(verts, np.stack([b[0] - 2 * pad, b[1] + 2 * pad]))
    orig = faces[keep]
    exact = ~near[orig].any(axis=1)
    got, want = out_verts[out_faces[:tn]], verts[orig]
    ok = got[exact].tobytes() == want[exact].tobytes()
    known = {p.tobytes() for p in verts}
    ok = ok and all(p.tobytes() in known for p in got[~exact].reshape(-1, 3))
    return bool(ok), int(exact.sum())


# ---------------------------------------------------------------------------------------------------- 4. the pads
def choose_aabb_pad(run, pads=(0.01, 0.015, 0.02, 0.025, 0.03)):
    """:1034-1048.  run(pad) -> dict with cc_update_num, max_dist_in_connection.  (best pad or None, scores)."""
    scores = [100.0] * len(pads)
    for i, pad in enumerate(pads):
        out = run(pad)
        if out["cc_update_num"] == -1:
            return None, scores
        if out["cc_update_num"] > 0:
            scores[i] = out["max_dist_in_connection"]
    return pads[int(np.argmin(np.asarray(scores)))], scores
