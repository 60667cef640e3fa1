"""Which regions of the mesh are re-meshed at topology errors, and the cuts around them: the front half of update_mesh_topo
(gaustar_trainers/refined_mesh.py:463-693) on the GPU.

After detect_topo_err has coloured the faces and extract_mesh_fusion has given the TSDF surface, update_mesh_topo takes the
faces above the colour cut-off (:516), groups them into connected components (:524), keeps the large ones (:526), puts a box
around each one's vertices and Gaussian centres (:552-571), merges boxes that overlap (:574) and cuts the fused surface and the
base mesh by every box (:583, :609).  The reference does that with trimesh, scipy and numpy on the host; here the meshes stay
device tensors and the passes are HIP kernels (include/gsr.h, gsr_regions.hip):

    counts = face_edge_counts(faces)                                   # [F,3] int32: faces sharing each face-edge
    label, count = face_components(faces, mask)                        # trimesh.graph.connected_component_labels(face_adjacency)
    regions = select_update_regions(verts, faces, points, face_colour, G)        # once per frame: UpdateRegions
    boxes = regions.boxes(aabb_pad)                                    # per aabb_pad trial: float64 [m,2,3], host numpy
    cut = cut_mesh_by_box(verts, faces, box, cut_inner, attrs=(colors,))         # cut_mesh_by_boundingbox (:227-251): CutMesh
    idx = boundary_vertices(verts, faces, box, cut_inner)              # find_boundary_verts (:84-111)
    keep = outlier_component_mask(faces, face_num_threshold)           # get_outlier_cc_mask (:291-307)

Vertex identity is the vertex index: nothing merges vertices by position, and the reference's OBJ round trip of the detected
mesh is not reproduced.  Two faces are adjacent iff they share an edge that exactly two face-edges of the mesh have and they
are different faces; an edge of three or more faces links nothing.  With a mask the edges are counted among the masked faces
only, as the reference counts them after update_faces.  Components are numbered by ascending smallest face index, the order
scipy.sparse.csgraph.connected_components gives.  Every output is an integer or an exactly defined float: the same inputs give
the same bits.

The stitch that follows the cuts is here too (gsr_stitch.hip), as far as it can be defined exactly:

    idx, d2 = nearest_vertices(queries, candidates)                     # knn_points(K=1) (:166, :175)
    st = connect_two_meshes(verts1, faces1, b1, verts2, faces2, b2)     # connect_two_meshes (:158-215): StitchedMesh
    cut = merge_vertices_around_holes(verts, faces)                     # merge_vert_around_holes (:126-155) and :201-203
    cut = select_faces(verts, faces, face_mask, attrs)                  # update_faces + remove_unreferenced_vertices
    ok = is_watertight(faces)                                           # trimesh is_watertight (:639)

Where the stitch departs from the reference's libraries, on purpose:
  * nearest_vertices takes the f32 coordinates to float64 and forms d2 = (dx dx + dy dy) + dz dz there, without contraction;
    among equal distances the lowest candidate index wins.  pytorch3d's knn_points sums in f32 (:166, :175 pass .float()
    copies), so it can rank two candidates differently only when their distances agree to f32 rounding.
  * Vertices are grouped by position when their three coordinates compare equal as numbers (-0 equals +0, NaN equals
    nothing).  trimesh.grouping.group_rows groups after rounding to 1e-8.
  * A face is degenerate iff two of its three vertex indices are equal.  trimesh's nondegenerate_faces also drops faces
    thinner than 1e-8; they are kept here, because dropping them opens a hole.
  * fill_small_holes replaces trimesh's fill_holes (:589, :617, :652), whose result follows networkx's cycle_basis traversal,
    by one canonical rule (its docstring): rims of 3 or 4 vertices are filled, the quad's diagonal passes through the rim's
    lowest vertex, new faces come in ascending lowest vertex, and a component of boundary edges with a vertex of degree != 2
    (two holes meeting at a vertex) is left alone, where trimesh may fill part of it.  Where trimesh's answer does not depend
    on the traversal the two agree.

The rest of update_mesh_topo is here as well (gsr_splice.hip):

    filled = fill_small_holes(faces, n_verts)                           # fill_holes (:589, :617, :652): FilledMesh
    area = face_areas(verts, faces)                                     # trimesh area_faces (:683), float64
    upd = update_mesh_topology(verts, faces, regions, fusion_mesh)      # the loop over the boxes (:578-693): TopologyUpdate
    pad, scores = choose_aabb_pad(run)                                  # the five aabb_pad trials (:1034-1048)

The reference applies find_boundary_verts and get_outlier_cc_mask after fill_holes; boundary_vertices and
outlier_component_mask are primitives on whatever mesh they are given, and update_mesh_topology gives them the filled one.
update_mesh_topology records where every face of its result came from (TopologyUpdate.face_origin), and
TopologyUpdate.with_colors carries the colours along it (gsr_handover.hip, gaustar_amd.handover): an input face keeps its colour,
a fusion face is coloured from its vertices, a filled face has none -- a departure from trimesh, whose fill_holes gives new faces
a library default colour that would tint the rim vertices; the roundings of the vertex <-> face conversions are this project's
statement of trimesh's, and parity with trimesh is not pinned (it is not a dependency).

    upd = update_mesh_topology(...).with_colors(base_face_rgba, fusion_mesh.colors)    # face_colors, vertex_colors; save() writes them
    track_face_mask, ref_area = load_tracking("face_corr.npz")          # what refine.py:315-323 reads back

Stated once for all of the above: a mesh's edge counts (_edge_counts); the tail of a compaction (_emit: cut_mesh_by_box and
select_faces / the degenerate passes differ in the mark call before it); steps 1 and 2 of one box (_patch_for_box,
_base_for_box: update_mesh_topology fills holes, harness's stitch_update_region does not).  The checks of a mesh argument and
the err word of the four kernel files with its decoder are gaustar_amd._meshargs', shared with the other mesh features.
"""
from __future__ import annotations

import ctypes
import itertools
import math
import os
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _host, _lib, _meshargs as _ma
from ._lib import ptr as _p
from ._meshargs import MAX_FACES      # (this module's limit since its first kernel: it stays in __all__)


def _box6(box) -> Tuple[np.ndarray, ctypes.Array]:
    b = np.asarray(box, np.float64)
    if b.shape != (2, 3) or np.isnan(b).any():
        raise ValueError("box must be [2,3] (lo, hi) without NaN")
    return b, (ctypes.c_double * 6)(*b.reshape(-1))


# ------------------------------------------------------------------------------------------------ edges and components
# (Throughout: an underscore worker launches on its tensors' stream; the public function around it has made their device current.)
def _edge_keys(faces: torch.Tensor, mask: Optional[torch.Tensor], colour: Optional[torch.Tensor], cut: int, err: torch.Tensor, st):
    """faces [F,3] int32 (F > 0) -> (selected [F] uint8, keys [3F] int64: min << 32 | max of every face-edge's vertex pair, a
    sentinel for the faces not selected).  st: the caller's _host.stream_of(faces), which it needs for its next launch anyway."""
    F = int(faces.shape[0])
    sel = torch.empty(F, dtype=torch.uint8, device=faces.device)
    keys = torch.empty(3 * F, dtype=torch.int64, device=faces.device)
    _lib.check(_lib.load().gsr_regions_edge_keys(F, _p(faces), _p(mask), _p(colour), int(cut), _p(sel), _p(keys), _p(err), st),
               "gsr_regions_edge_keys")
    return sel, keys


def _edge_runs(faces: torch.Tensor, mask: Optional[torch.Tensor], colour: Optional[torch.Tensor], cut: int, err: torch.Tensor):
    """faces [F,3] int32 (F > 0) -> (selected [F] uint8, counts [F,3] int32, pairs [3F,2] int32)."""
    dev, F = faces.device, int(faces.shape[0])
    st = _host.stream_of(faces)
    sel, keys = _edge_keys(faces, mask, colour, cut, err, st)
    skeys, order = torch.sort(keys, stable=True)
    del keys
    counts = torch.empty(F, 3, dtype=torch.int32, device=dev)
    pairs = torch.empty(3 * F, 2, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gsr_regions_edge_runs(F, _p(skeys), _p(order), _p(counts), _p(pairs), st), "gsr_regions_edge_runs")
    return sel, counts, pairs


def _edge_counts(faces: torch.Tensor, err: torch.Tensor, mask: Optional[torch.Tensor] = None) -> Optional[torch.Tensor]:
    """The edge counts of a mesh: [F,3] int32 as face_edge_counts gives them, None without faces.  Nothing is read."""
    return _edge_runs(faces, mask, None, 0, err)[1] if faces.shape[0] else None


def face_edge_counts(faces: torch.Tensor, mask: Optional[torch.Tensor] = None) -> torch.Tensor:
    """[F,3] int32: for face-edge e of face (a, b, c) -- (a, b), (b, c), (c, a) -- how many face-edges of the mesh have the same
    vertex pair, itself included (trimesh: group_rows(edges_sorted, require_count=1) are the ones, require_count=2 the twos).
    With a mask the masked faces' edges are counted among themselves and the others get 0.  The call has no vertex count:
    a negative index raises ValueError, an index past the mesh's vertices is an edge end like any other and is only caught by
    the calls that take verts."""
    faces = _ma.faces_i32(faces)
    dev, F = faces.device, int(faces.shape[0])
    if F == 0:
        return torch.empty(0, 3, dtype=torch.int32, device=dev)
    err, mask = _ma.new_err(dev), _ma.mask_u8(mask, F, dev)
    with _host.on_device(dev):
        counts = _edge_counts(faces, err, mask)
    _ma.raise_if(int(err.cpu()))
    return counts


def _components(faces: torch.Tensor, mask: Optional[torch.Tensor], colour: Optional[torch.Tensor], cut: int, err: torch.Tensor):
    """faces [F,3] int32 (F > 0) -> (label [F] int32, count [F] int32 with the faces of label l at l and zeros behind, n [1]
    int32 on the device = the number of components, parent [F] int32 = the smallest face of every face's component).  Nothing
    is read back."""
    lib = _lib.load()
    dev, F = faces.device, int(faces.shape[0])
    sel, _counts, pairs = _edge_runs(faces, mask, colour, cut, err)
    parent = torch.empty(F, dtype=torch.int32, device=dev)
    flag = torch.empty(F, dtype=torch.int32, device=dev)
    st = _host.stream_of(faces)
    _lib.check(lib.gsr_regions_components(F, _p(pairs), _p(sel), _p(parent), _p(flag), st), "gsr_regions_components")
    scan = torch.cumsum(flag, 0, dtype=torch.int32)
    label = torch.empty(F, dtype=torch.int32, device=dev)
    count = torch.zeros(F, dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_regions_labels(F, _p(parent), _p(scan), _p(sel), _p(label), _p(count), st), "gsr_regions_labels")
    return label, count, scan[-1:], parent


def face_components(faces: torch.Tensor, mask: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """(label [F] int32, count [n] int32): the connected components of the faces with `mask` set (all without one) under the
    adjacency of the module docstring, numbered by ascending smallest face index; label is -1 outside the mask.  What
    trimesh.graph.connected_component_labels(mesh.face_adjacency, node_count=F) and np.bincount give for the masked mesh
    (refined_mesh.py:524-525).  One host read: n.  As face_edge_counts, it has no vertex count: only a negative index raises."""
    faces = _ma.faces_i32(faces)
    dev, F = faces.device, int(faces.shape[0])
    if F == 0:
        return torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.int32, device=dev)
    err, mask = _ma.new_err(dev), _ma.mask_u8(mask, F, dev)
    with _host.on_device(dev):
        label, count, n, _parent = _components(faces, mask, None, 0, err)
    head = torch.cat([n, err]).cpu()
    _ma.raise_if(int(head[1]))
    return label, count[:int(head[0])]


# ------------------------------------------------------------------------------------------------ selection and boxes
def combine_overlap_aabbs(boxes: Sequence[np.ndarray]) -> List[np.ndarray]:
    """combine_overlap_aabbs (refined_mesh.py:254-288), its order dependence included: box j joins the first merged entry i
    for which one of j's eight corners lies strictly inside the i-th box OF THE INPUT LIST (:269 tests aabb_list[i], not the
    merged list), by min / max; whenever a pass merged something the result goes through again."""
    boxes = [np.asarray(b, np.float64) for b in boxes]
    out: List[np.ndarray] = []
    for b in boxes:
        corners = np.array([[b[i, 0], b[j, 1], b[k, 2]] for i, j, k in itertools.product((0, 1), repeat=3)])
        hit = -1
        for i in range(len(out)):
            lo, hi = boxes[i][0], boxes[i][1]
            if ((corners > lo) & (corners < hi)).all(axis=1).any():
                hit = i
                break
        if hit < 0:
            out.append(b)
        else:
            out[hit] = np.stack([np.minimum(out[hit][0], b[0]), np.maximum(out[hit][1], b[1])])
    return out if len(out) == len(boxes) else combine_overlap_aabbs(out)


@dataclass
class UpdateRegions:
    """What select_update_regions found.  component [F] int32: the component of every face above the cut-off (-1 below);
    region [F] int32: its kept region (-1: none); n_components; n_regions; labels [n_regions]: the component each region is;
    counts [n_regions]: its faces; raw_boxes float64 [n_regions,2,3]: min and max over the region's vertices and Gaussian
    centres (f32 values, exact); nothing_to_update = no region (the reference's cc_update_num == -1, :528-529).  component and
    region are device tensors, the rest numpy."""
    component: torch.Tensor
    region: torch.Tensor
    n_components: int
    n_regions: int
    labels: np.ndarray
    counts: np.ndarray
    raw_boxes: np.ndarray

    @property
    def nothing_to_update(self) -> bool:
        return self.n_regions == 0

    def boxes(self, aabb_pad: float = 0.02) -> np.ndarray:
        """float64 [m,2,3]: every raw box grown by aabb_pad in float64 (refined_mesh.py:567-569), then merged by
        combine_overlap_aabbs (:574).  Host numpy on a handful of boxes."""
        grown = self.raw_boxes.copy()
        grown[:, 0] -= float(aabb_pad)
        grown[:, 1] += float(aabb_pad)
        merged = combine_overlap_aabbs(list(grown))
        return np.stack(merged) if merged else np.zeros((0, 2, 3))


def _decode_boxes(enc: np.ndarray) -> np.ndarray:
    """gsr_regions_boxes' uint32 [n,2,3] -> float64 (the f32 values, widened)."""
    u = enc.astype(np.uint32)
    bits = np.where(u & np.uint32(0x80000000), u ^ np.uint32(0x80000000), ~u).astype(np.uint32)
    return bits.view(np.float32).astype(np.float64)


@torch.no_grad()
def select_update_regions(verts: torch.Tensor, faces: torch.Tensor, points: torch.Tensor, face_colour: torch.Tensor, G: int,
                          delta_threshold: float = 0.6, cc_face_threshold: int = 80) -> UpdateRegions:
    """refined_mesh.py:516-571 without the pad: the faces with face_colour >= 255 delta_threshold (:516), their components
    (:524), those with MORE than cc_face_threshold faces (:526) in label order, and per kept component the box of its faces'
    vertices and of its faces' G Gaussian centres (points [F G,3], face-major; :538-567).  face_colour: [F] uint8
    (topology.TopologyErrors.face_colour).  Does not depend on aabb_pad: once per frame.  One host read (the kept components'
    counts and boxes).  A NaN among a kept region's vertices or centres raises ValueError (numpy's min / max would answer NaN)."""
    lib = _lib.load()
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, F, V, G = faces.device, int(faces.shape[0]), int(verts.shape[0]), int(G)
    thr = int(cc_face_threshold)
    if thr < 0 or G < 0:
        raise ValueError("cc_face_threshold and G must not be negative")
    if tuple(points.shape) != (F * G, 3) or points.dtype != torch.float32 or points.device != dev:
        raise ValueError("points must be [F G,3] float32 on the faces' GPU")
    if tuple(face_colour.shape) != (F,) or face_colour.dtype != torch.uint8 or face_colour.device != dev:
        raise ValueError("face_colour must be [F] uint8 on the faces' GPU")
    cut = math.ceil(255 * float(delta_threshold))     # an integer colour c has c >= x iff c >= ceil(x); x in float64 (:516)
    empty = torch.empty(0, dtype=torch.int32, device=dev)
    if F == 0:
        return UpdateRegions(empty, empty, 0, 0, np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros((0, 2, 3)))
    points, face_colour = points.detach().contiguous(), face_colour.contiguous()
    err = _ma.new_err(dev)
    cap = F // (thr + 1)                               # (a kept component has at least thr + 1 faces)
    kept_label = torch.zeros(cap, dtype=torch.int32, device=dev)
    kept_count = torch.zeros(cap, dtype=torch.int32, device=dev)
    region = torch.empty(F, dtype=torch.int32, device=dev)
    enc = torch.empty(cap, 6, dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        st = _host.stream_of(faces)
        label, count, n, _parent = _components(faces, None, face_colour, cut, err)
        kscan = torch.cumsum(count > thr, 0, dtype=torch.int32)
        _lib.check(lib.gsr_regions_select(F, _p(count), thr, _p(kscan), _p(label), cap, _p(kept_label), _p(kept_count), _p(region), st),
                   "gsr_regions_select")
        _lib.check(lib.gsr_regions_boxes(F, G, V, _p(faces), _p(verts), _p(points), _p(region), cap, _p(enc), _p(err), st),
                   "gsr_regions_boxes")
    head = torch.cat([n, kscan[-1:], err, kept_label, kept_count, enc.reshape(-1)]).cpu().numpy()
    _ma.raise_if(int(head[2]))
    m = int(head[1])
    body = head[3:]
    return UpdateRegions(component=label, region=region, n_components=int(head[0]), n_regions=m, labels=body[:m].copy(),
                         counts=body[cap:cap + m].copy(),
                         raw_boxes=_decode_boxes(body[2 * cap:2 * cap + 6 * m].view(np.uint32).reshape(m, 2, 3)))


# ------------------------------------------------------------------------------------------------ cut
@dataclass
class CutMesh:
    """verts [Nv,3] f32, faces [Nf,3] int32 (new vertex numbers), face_mask [F] bool (the input faces kept: the reference's
    'inside_face_mask'), vert_map [V] int32 (old vertex -> new, -1 = dropped), attrs (the per-vertex arrays given, gathered)."""
    verts: torch.Tensor
    faces: torch.Tensor
    face_mask: torch.Tensor
    vert_map: torch.Tensor
    attrs: Tuple[torch.Tensor, ...]


def _inside(verts: torch.Tensor, box6) -> torch.Tensor:
    V = int(verts.shape[0])
    inside = torch.empty(V, dtype=torch.uint8, device=verts.device)
    _lib.check(_lib.load().gsr_regions_inside(V, _p(verts), box6, _p(inside), _host.stream_of(verts)), "gsr_regions_inside")
    return inside


def _gather(old_of_new: torch.Tensor, src: torch.Tensor) -> torch.Tensor:
    n = int(old_of_new.shape[0])
    C = int(np.prod(src.shape[1:])) if src.dim() > 1 else 1
    out = torch.empty((n, *src.shape[1:]), dtype=src.dtype, device=src.device)
    _lib.check(_lib.load().gsr_regions_gather(n, C, _p(old_of_new), _p(src), _p(out), _host.stream_of(src)), "gsr_regions_gather")
    return out


def _vertex_attrs(attrs: Sequence[torch.Tensor], V: int, dev) -> Tuple[torch.Tensor, ...]:
    attrs = tuple(attrs)
    for a in attrs:
        if a.dim() < 1 or a.shape[0] != V or a.element_size() != 4 or a.device != dev:
            raise ValueError("attrs must be per-vertex arrays [V, ...] of a 4-byte dtype on the mesh's GPU")
    return attrs


def _emit(verts: torch.Tensor, faces: torch.Tensor, keep: torch.Tensor, ref: torch.Tensor, attrs: Sequence[torch.Tensor],
          err: torch.Tensor, st) -> Tuple[CutMesh, torch.Tensor]:
    """The tail of a compaction, after a mark call on stream st has written keep [F] and ref [V] int32 (0 / 1): the faces with
    keep set, in their order, the vertices with ref set renumbered in ascending old index -> (CutMesh, keep_scan [F] int32).
    One host read: the two totals and err."""
    dev, F, V = faces.device, int(faces.shape[0]), int(verts.shape[0])
    kscan = torch.cumsum(keep, 0, dtype=torch.int32)
    vscan = torch.cumsum(ref, 0, dtype=torch.int32)
    zero = torch.zeros(1, dtype=torch.int32, device=dev)
    head = torch.cat([kscan[-1:] if F else zero, vscan[-1:] if V else zero, err]).cpu()
    _ma.raise_if(int(head[2]), _ma.NAN_BOUNDARY)      # (bit 1 comes from connect_two_meshes' searches only)
    nf, nv = int(head[0]), int(head[1])
    faces_out = torch.empty(nf, 3, dtype=torch.int32, device=dev)
    face_mask = torch.empty(F, dtype=torch.bool, device=dev)
    vert_map = torch.empty(V, dtype=torch.int32, device=dev)
    old_of_new = torch.empty(nv, dtype=torch.int32, device=dev)
    _lib.check(_lib.load().gsr_regions_cut_emit(F, V, _p(faces), _p(keep), _p(kscan), _p(ref), _p(vscan), _p(faces_out), _p(face_mask),
                                                _p(vert_map), _p(old_of_new), st), "gsr_regions_cut_emit")
    cut = CutMesh(verts=_gather(old_of_new, verts), faces=faces_out, face_mask=face_mask, vert_map=vert_map,
                  attrs=tuple(_gather(old_of_new, a.detach().contiguous()) for a in attrs))
    return cut, kscan


@torch.no_grad()
def cut_mesh_by_box(verts: torch.Tensor, faces: torch.Tensor, box, cut_inner: bool, attrs: Sequence[torch.Tensor] = ()) -> CutMesh:
    """cut_mesh_by_boundingbox (refined_mesh.py:218-251).  box: [2,3] (lo, hi), taken as float64.  A vertex is inside iff all
    three coordinates are strictly between the bounds, compared in float64 (the f32 coordinate widens exactly).
    cut_inner=False keeps the faces with any vertex inside, cut_inner=True those with none.  Kept faces keep their order;
    the vertices they use are renumbered in ascending old index (remove_unreferenced_vertices).  attrs: per-vertex arrays
    [V, ...] of a 4-byte dtype (the fusion's colours) that follow the vertices.  An empty result is legal.  One host read: the
    two totals."""
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, F, V = faces.device, int(faces.shape[0]), int(verts.shape[0])
    _b, box6 = _box6(box)
    attrs = _vertex_attrs(attrs, V, dev)
    keep = torch.empty(F, dtype=torch.int32, device=dev)
    ref = torch.empty(V, dtype=torch.int32, device=dev)
    err, st = _ma.new_err(dev), _host.stream_of(faces)
    with _host.on_device(dev):
        inside = _inside(verts, box6)
        _lib.check(_lib.load().gsr_regions_cut_mark(F, V, _p(faces), _p(inside), int(bool(cut_inner)), _p(keep), _p(ref), _p(err), st),
                   "gsr_regions_cut_mark")
        return _emit(verts, faces, keep, ref, attrs, err, st)[0]


@dataclass
class RegionCut:
    """One merged box of a frame (harness.SurfaceGaussians.cut_update_regions): box float64 [2,3]; fusion_patch: the fused
    surface's faces with any vertex inside it (attrs[0]: the vertex colours); base_cut: the base mesh without the faces that
    have a vertex inside it."""
    box: np.ndarray
    fusion_patch: CutMesh
    base_cut: CutMesh


# ------------------------------------------------------------------------------------------------ primitives
@torch.no_grad()
def boundary_vertices(verts: torch.Tensor, faces: torch.Tensor, box=None, cut_inner: bool = False, pad: float = 0.02) -> torch.Tensor:
    """find_boundary_verts (refined_mesh.py:84-111): the vertices on edges that exactly one face-edge has, as ascending int32
    indices.  With a box and cut_inner=True those inside the box grown by `pad` (:94-99, grown in float64); with a box and
    cut_inner=False those that belong to a face with some but not all of its vertices inside the box (:101-111).
    A primitive on the mesh it is given: the reference calls it after fill_holes (:589-600, :617-619), and so does
    update_mesh_topology, with fill_small_holes."""
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, F, V = faces.device, int(faces.shape[0]), int(verts.shape[0])
    err, st = _ma.new_err(dev), _host.stream_of(faces)
    bmark = torch.empty(V, dtype=torch.uint8, device=dev)
    fmark = inside = None
    with _host.on_device(dev):
        counts = _edge_counts(faces, err)
        if box is not None:
            b, box6 = _box6(box)
            if cut_inner:
                grown = np.stack([b[0] - float(pad), b[1] + float(pad)])
                grown_inside = _inside(verts, (ctypes.c_double * 6)(*grown.reshape(-1)))
            else:
                inside = _inside(verts, box6)
                fmark = torch.empty(V, dtype=torch.uint8, device=dev)
        _lib.check(_lib.load().gsr_regions_boundary(F, V, _p(faces), _p(counts), _p(inside), _p(bmark), _p(fmark), _p(err), st),
                   "gsr_regions_boundary")
    sel = bmark if box is None else (bmark & grown_inside if cut_inner else bmark & fmark)
    idx = torch.nonzero(sel).view(-1).to(torch.int32)
    _ma.raise_if(int(err.cpu()))
    return idx


@torch.no_grad()
def outlier_component_mask(faces: torch.Tensor, face_num_threshold: Optional[float] = None) -> torch.Tensor:
    """get_outlier_cc_mask (refined_mesh.py:291-307): [F] bool, True for the faces of components with at least
    min(face_num_threshold, 0.3 max count) faces -- 0.3 max count when the threshold is None -- the product in float64 on the
    host.  A primitive on the mesh it is given: the reference calls it after fill_holes (:589-592), and so does
    update_mesh_topology, with fill_small_holes.  One host read: the components' counts."""
    label, count = face_components(faces)
    F = int(label.shape[0])
    out = torch.empty(F, dtype=torch.bool, device=label.device)
    if F == 0:
        return out
    bound = float(count.max().cpu()) * 0.3
    if face_num_threshold is not None:
        bound = min(float(face_num_threshold), bound)
    with _host.on_device(label.device):
        _lib.check(_lib.load().gsr_regions_label_mask(F, _p(label), _p(count), int(math.ceil(bound)), _p(out), _host.stream_of(label)),
                   "gsr_regions_label_mask")
    return out


# ------------------------------------------------------------------------------------------------ stitch
def _nn_const(name: str) -> int:
    return int(getattr(_lib.load(), name)())


def __getattr__(name: str):
    """NN_TILE: the candidates the nearest-vertex kernel stages in LDS at once; NN_QUERIES: the queries of one workgroup.  Read
    from the library, so importing this module does not need it."""
    if name == "NN_TILE":
        return _nn_const("gsr_stitch_nn_tile")
    if name == "NN_QUERIES":
        return _nn_const("gsr_stitch_nn_queries")
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")


def _nearest(q: torch.Tensor, c: torch.Tensor, err: torch.Tensor):
    """q [Bq,3], c [Bc,3] f32 contiguous, Bq, Bc > 0 -> (idx [Bq] int32, d2 [Bq] f64, max_bits [1] int64).  Nothing is read."""
    Bq, Bc = int(q.shape[0]), int(c.shape[0])
    idx = torch.empty(Bq, dtype=torch.int32, device=q.device)
    d2 = torch.empty(Bq, dtype=torch.float64, device=q.device)
    mx = torch.empty(1, dtype=torch.int64, device=q.device)
    _lib.check(_lib.load().gsr_stitch_nearest(Bq, Bc, _p(q), _p(c), _p(idx), _p(d2), _p(mx), _p(err), _host.stream_of(q)),
               "gsr_stitch_nearest")
    return idx, d2, mx


@torch.no_grad()
def nearest_vertices(queries: torch.Tensor, candidates: torch.Tensor, return_max: bool = False):
    """(idx int32 [Bq], d2 float64 [Bq]): per query the nearest candidate and the squared distance to it, as the module
    docstring defines them: knn_points(K=1) of refined_mesh.py:166, :175 in float64, the lowest index among equals.
    return_max=True adds the largest d2 as a Python float (0.0 without queries).  No candidates, or a coordinate that is NaN or
    infinite, raise ValueError.  One host read: the err word (and the maximum)."""
    for t in (queries, candidates):
        if t.dim() != 2 or t.shape[1] != 3 or t.dtype != torch.float32:
            raise ValueError("queries and candidates must be [B,3] float32")
        if t.device.type != "cuda" or t.device != queries.device:
            raise RuntimeError("queries and candidates must be on one GPU")
    if candidates.shape[0] == 0:
        raise ValueError("no candidates")
    dev = queries.device
    if queries.shape[0] == 0:
        out = torch.empty(0, dtype=torch.int32, device=dev), torch.empty(0, dtype=torch.float64, device=dev)
        return (*out, 0.0) if return_max else out
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        idx, d2, mx = _nearest(queries.detach().contiguous(), candidates.detach().contiguous(), err)
    head = torch.cat([err.to(torch.int64), mx]).cpu().numpy()
    _ma.raise_if(int(head[0]), _ma.NAN_BOUNDARY)
    return (idx, d2, float(head[1:].view(np.float64)[0])) if return_max else (idx, d2)


def _compact(verts: torch.Tensor, faces: torch.Tensor, remap: Optional[torch.Tensor], mask: Optional[torch.Tensor],
             attrs: Sequence[torch.Tensor], err: torch.Tensor) -> Tuple[CutMesh, torch.Tensor]:
    """The faces rewritten by `remap`, kept by `mask` (without one: unless degenerate), their vertices renumbered in ascending
    old index -> (CutMesh, keep_scan [F] int32).  One host read: the two totals and err."""
    dev, F, V = faces.device, int(faces.shape[0]), int(verts.shape[0])
    faces_rw = torch.empty(F, 3, dtype=torch.int32, device=dev)
    keep = torch.empty(F, dtype=torch.int32, device=dev)
    ref = torch.empty(V, dtype=torch.int32, device=dev)
    st = _host.stream_of(faces)
    _lib.check(_lib.load().gsr_stitch_mark(F, V, _p(faces), _p(remap), _p(mask), _p(faces_rw), _p(keep), _p(ref), _p(err), st),
               "gsr_stitch_mark")
    return _emit(verts, faces_rw, keep, ref, attrs, err, st)


@torch.no_grad()
def select_faces(verts: torch.Tensor, faces: torch.Tensor, face_mask: torch.Tensor, attrs: Sequence[torch.Tensor] = ()) -> CutMesh:
    """update_faces(face_mask) and remove_unreferenced_vertices (refined_mesh.py:598-599): the faces with face_mask set, in
    their order, their vertices renumbered in ascending old index; attrs as in cut_mesh_by_box.  One host read: the totals."""
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, F, V = faces.device, int(faces.shape[0]), int(verts.shape[0])
    mask = _ma.mask_u8(face_mask, F, dev)
    if mask is None:
        raise ValueError("face_mask must be [F] bool or uint8")
    attrs = _vertex_attrs(attrs, V, dev)
    with _host.on_device(dev):
        return _compact(verts, faces, None, mask, attrs, _ma.new_err(dev))[0]


def _watertight_word(faces: torch.Tensor, err: torch.Tensor) -> torch.Tensor:
    """[1] int32 on the device: 1 where some face-edge's count is not 2."""
    bad = torch.empty(1, dtype=torch.int32, device=faces.device)
    _lib.check(_lib.load().gsr_stitch_watertight(int(faces.shape[0]), _p(_edge_counts(faces, err)), _p(bad), _host.stream_of(faces)),
               "gsr_stitch_watertight")
    return bad


@torch.no_grad()
def is_watertight(faces: torch.Tensor) -> bool:
    """trimesh's is_watertight (refined_mesh.py:639): F > 0 and every face-edge's vertex pair occurs exactly twice.  Reduced on
    the device; one word is read."""
    faces = _ma.faces_i32(faces)
    if faces.shape[0] == 0:
        return False
    err = _ma.new_err(faces.device)
    with _host.on_device(faces.device):
        head = torch.cat([_watertight_word(faces, err), err]).cpu()
    _ma.raise_if(int(head[1]))
    return int(head[0]) == 0


def _merge_holes(verts: torch.Tensor, faces: torch.Tensor, max_hole_vert_num: int, err: torch.Tensor):
    """verts [V,3] f32, faces [F,3] int32, contiguous -> (CutMesh, keep_scan, remap [V] int32): merge_vert_around_holes and the
    degenerate pass after it.  Host reads: the hole vertices' number (torch.nonzero) and _compact's totals."""
    lib = _lib.load()
    dev, F, V = faces.device, int(faces.shape[0]), int(verts.shape[0])
    st = _host.stream_of(faces)
    remap = torch.arange(V, dtype=torch.int32, device=dev)
    if F == 0 or V == 0:
        return (*_compact(verts, faces, remap, None, (), err), remap)
    counts = _edge_counts(faces, err)
    pairs = torch.empty(3 * F, 2, dtype=torch.int32, device=dev)
    hole = torch.empty(V, dtype=torch.uint8, device=dev)
    parent = torch.empty(V, dtype=torch.int32, device=dev)
    flag = torch.empty(V, dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_stitch_hole_components(F, V, _p(faces), _p(counts), _p(pairs), _p(hole), _p(parent), _p(flag), _p(err), st),
               "gsr_stitch_hole_components")
    size = torch.empty(V, dtype=torch.int32, device=dev)
    moved = torch.empty_like(verts)
    _lib.check(lib.gsr_stitch_hole_move(V, int(max_hole_vert_num), _p(hole), _p(parent), _p(size), _p(verts), _p(moved), st),
               "gsr_stitch_hole_move")
    hv = torch.nonzero(hole).view(-1).to(torch.int32)
    H = int(hv.shape[0])
    if H:
        kxy = torch.empty(H, dtype=torch.int64, device=dev)
        kz = torch.empty(H, dtype=torch.int64, device=dev)
        _lib.check(lib.gsr_stitch_pos_keys(H, _p(hv), _p(moved), _p(kxy), _p(kz), st), "gsr_stitch_pos_keys")
        o1 = torch.sort(kz, stable=True)[1]
        order = o1[torch.sort(kxy[o1], stable=True)[1]].contiguous()
        head = torch.empty(H, dtype=torch.int32, device=dev)
        _lib.check(lib.gsr_stitch_pos_heads(H, _p(order), _p(hv), _p(moved), _p(head), st), "gsr_stitch_pos_heads")
        first = torch.cummax(head, 0)[0].contiguous()
        _lib.check(lib.gsr_stitch_pos_remap(H, _p(order), _p(hv), _p(first), _p(remap), st), "gsr_stitch_pos_remap")
    return (*_compact(moved, faces, remap, None, (), err), remap)


@torch.no_grad()
def merge_vertices_around_holes(verts: torch.Tensor, faces: torch.Tensor, max_hole_vert_num: int = 10) -> CutMesh:
    """merge_vert_around_holes (refined_mesh.py:126-155) and the degenerate pass that follows it (:201-203).  Hole edges are the
    face-edges whose vertex pair occurs other than exactly twice, hole vertices their ends.  Every component of the hole
    vertices under the hole edges with at most max_hole_vert_num vertices moves to its lowest vertex's position; then ALL hole
    vertices are grouped by equal position and every face entry is rewritten to its group's lowest vertex; faces with two
    equal indices are dropped and the vertices renumbered.  -> CutMesh (face_mask over the input faces, vert_map with merged
    vertices at their representative's new index).  The inputs are not modified."""
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, V = faces.device, int(verts.shape[0])
    with _host.on_device(dev):
        cut, _kscan, remap = _merge_holes(verts, faces, max_hole_vert_num, _ma.new_err(dev))
        if V and cut.verts.shape[0]:
            ident = torch.arange(int(cut.verts.shape[0]), dtype=torch.int32, device=dev)
            out = torch.empty(V, dtype=torch.int32, device=dev)
            # (remap, then the compaction's map; the second pair of maps is the identity)
            _lib.check(_lib.load().gsr_stitch_vert_map(V, _p(remap), _p(cut.vert_map), _p(ident), _p(ident), _p(out), _host.stream_of(faces)),
                       "gsr_stitch_vert_map")
            cut.vert_map = out
    return cut


@dataclass
class StitchedMesh:
    """What connect_two_meshes returns.  verts [Nv,3] f32, faces [Nf,3] int32: the stitched mesh; face_mask [F1 + F2] bool: the
    faces of concat(mesh 1, mesh 2) kept after both degenerate passes (the reference's 'valid_face_mask', :205-206); vert_map
    [V1 + V2] int32: old vertex (mesh 2's shifted by V1) -> new, -1 = dropped, merged vertices at their representative's new
    index; n_faces_from_first: the kept faces that came from mesh 1 (they come first); max_dist: sqrt of the larger of the two
    searches' largest d2, in float64 (:211); watertight: is_watertight(faces)."""
    verts: torch.Tensor
    faces: torch.Tensor
    face_mask: torch.Tensor
    vert_map: torch.Tensor
    n_faces_from_first: int
    max_dist: float
    watertight: bool


def _boundary_list(b: torch.Tensor, dev) -> torch.Tensor:
    if b.dim() != 1 or b.dtype != torch.int32:
        raise ValueError("a boundary list must be a 1-d int32 tensor")
    if b.device != dev:
        raise RuntimeError("a boundary list must be on the mesh's GPU")
    if b.shape[0] == 0:
        raise ValueError("a boundary list is empty: there is nothing to stitch along")
    return b.contiguous()


@torch.no_grad()
def connect_two_meshes(verts1: torch.Tensor, faces1: torch.Tensor, boundary1: torch.Tensor, verts2: torch.Tensor,
                       faces2: torch.Tensor, boundary2: torch.Tensor, max_hole_vert_num: int = 10) -> StitchedMesh:
    """connect_two_meshes (refined_mesh.py:158-215).  The boundary vertices of mesh 2 snap to their nearest boundary vertex of
    mesh 1 (:164-171), those of mesh 1 to their nearest of the snapped ones (:174-178); the meshes are concatenated, mesh 2's
    faces shifted by V1 (:181-184); the listed vertices concat(boundary1, V1 + boundary2) are grouped by position and every
    face entry naming one is rewritten to its group's earliest list entry (:188); degenerate faces go and the vertices are
    renumbered (:193-195); merge_vertices_around_holes (:198-203).  See the module docstring for what "nearest", "equal
    position" and "degenerate" mean here.  Boundary lists: int32, unique, in range, not empty, else ValueError; a boundary
    position that is NaN or infinite raises ValueError.  The inputs are not modified.  Host reads: the lists' err word, the
    two compactions' totals, the hole vertices' number, and one last read of the flags and maxima."""
    lib = _lib.load()
    faces1, faces2 = _ma.faces_i32(faces1), _ma.faces_i32(faces2)
    dev = faces1.device
    if faces2.device != dev:
        raise RuntimeError("the two meshes must be on one GPU")
    verts1, verts2 = _ma.verts_f32(verts1, dev), _ma.verts_f32(verts2, dev)
    b1, b2 = _boundary_list(boundary1, dev), _boundary_list(boundary2, dev)
    V1, V2, F1, F2 = int(verts1.shape[0]), int(verts2.shape[0]), int(faces1.shape[0]), int(faces2.shape[0])
    B1, B2 = int(b1.shape[0]), int(b2.shape[0])
    if V1 + V2 > 2 ** 31 - 1 or F1 + F2 > MAX_FACES:
        raise ValueError("the two meshes together are too large for int32 indices")
    st, err = _host.stream_of(faces1), _ma.new_err(dev)
    mark = torch.empty(max(V1, V2, 1), dtype=torch.int32, device=dev)
    with _host.on_device(dev):
        _lib.check(lib.gsr_stitch_check_list(B1, V1, _p(b1), _p(mark), _p(err), st), "gsr_stitch_check_list")
        _lib.check(lib.gsr_stitch_check_list(B2, V2, _p(b2), _p(mark), _p(err), st), "gsr_stitch_check_list")
        _ma.raise_if(int(err.cpu()), _ma.NAN_BOUNDARY)            # (before anything is gathered through the lists)
        # the two snaps
        pc1 = _gather(b1, verts1)
        pc2 = _gather(b2, verts2)
        n21, _d21, max21 = _nearest(pc2, pc1, err)
        pc2s = _gather(n21, pc1)
        n12, _d12, max12 = _nearest(pc1, pc2s, err)
        verts = torch.cat([verts1, verts2])
        verts[b1.long()] = _gather(n12, pc2s)
        verts[b2.long() + V1] = pc2s
        faces = torch.cat([faces1, faces2 + V1])
        # reset_duplicate_vert over the listed vertices, the first degenerate pass
        rep = torch.empty(B1, dtype=torch.int32, device=dev)
        remap1 = torch.empty(V1 + V2, dtype=torch.int32, device=dev)
        _lib.check(lib.gsr_stitch_snap_groups(B1, B2, V1, V2, _p(b1), _p(b2), _p(n21), _p(n12), _p(rep), _p(remap1), st),
                   "gsr_stitch_snap_groups")
        cut1, kscan1 = _compact(verts, faces, remap1, None, (), err)      # (raises on NaN / a bad face index: err is read here)
        # merge_vert_around_holes, the second degenerate pass
        cut2, _kscan2, remap2 = _merge_holes(cut1.verts, cut1.faces, max_hole_vert_num, err)
        F, V = F1 + F2, V1 + V2
        face_mask = torch.empty(F, dtype=torch.bool, device=dev)
        _lib.check(lib.gsr_stitch_compose_mask(F, _p(cut1.face_mask), _p(kscan1), _p(cut2.face_mask), int(cut2.face_mask.shape[0]),
                                               _p(face_mask), st), "gsr_stitch_compose_mask")
        vert_map = torch.empty(V, dtype=torch.int32, device=dev)
        if cut1.verts.shape[0]:
            _lib.check(lib.gsr_stitch_vert_map(V, _p(remap1), _p(cut1.vert_map), _p(remap2), _p(cut2.vert_map), _p(vert_map), st),
                       "gsr_stitch_vert_map")
        else:
            vert_map.fill_(-1)
        n_first = face_mask[:F1].sum(dtype=torch.int64).view(1)
        if cut2.faces.shape[0]:
            bad = _watertight_word(cut2.faces, err).to(torch.int64)
        else:
            bad = torch.ones(1, dtype=torch.int64, device=dev)
    head = torch.cat([err.to(torch.int64), bad, n_first, max21, max12]).cpu().numpy()
    _ma.raise_if(int(head[0]), _ma.NAN_BOUNDARY)
    d2max = head[3:5].view(np.float64)
    return StitchedMesh(verts=cut2.verts, faces=cut2.faces, face_mask=face_mask, vert_map=vert_map, n_faces_from_first=int(head[2]),
                        max_dist=float(np.sqrt(np.maximum(d2max[0], d2max[1]))), watertight=int(head[1]) == 0)


def compose_face_mask(outer: torch.Tensor, inner: torch.Tensor) -> torch.Tensor:
    """`m = outer.clone(); m[outer] = inner[:outer.sum()]` without a host read (refined_mesh.py:656-658): outer [F] bool, inner
    [>= outer.sum()] bool."""
    F = int(outer.shape[0])
    out = torch.empty(F, dtype=torch.bool, device=outer.device)
    scan = torch.cumsum(outer, 0, dtype=torch.int32)
    outer, inner = outer.contiguous(), inner.contiguous()
    with _host.on_device(outer.device):
        _lib.check(_lib.load().gsr_stitch_compose_mask(F, _p(outer), _p(scan), _p(inner), int(inner.shape[0]), _p(out), _host.stream_of(outer)),
                   "gsr_stitch_compose_mask")
    return out


@dataclass
class RegionStitch:
    """What harness.SurfaceGaussians.stitch_update_region returns for one box: stitched (StitchedMesh: the base cut, mesh 1,
    joined with the patch, mesh 2); patch (CutMesh: the fused patch without its outlier components, colours in attrs[0]);
    base_face_mask [F_base] bool: the faces of the UNCUT base mesh that are in the stitched mesh (refined_mesh.py:656-658)."""
    stitched: StitchedMesh
    patch: CutMesh
    base_face_mask: torch.Tensor


# ------------------------------------------------------------------------------------------------ hole filling
@dataclass
class FilledMesh:
    """What fill_small_holes returns.  faces [F + n_new,3] int32: the input faces, untouched and in their order, then the new
    ones; n_new; rim_of_new [n_new] int32: the lowest vertex of the rim each new face closes; watertight:
    is_watertight(faces)."""
    faces: torch.Tensor
    n_new: int
    rim_of_new: torch.Tensor
    watertight: bool


def _fill(faces: torch.Tensor, V: int, err: torch.Tensor) -> Tuple[torch.Tensor, int, torch.Tensor]:
    """faces [F,3] int32 contiguous -> (faces with the new ones appended, n_new, rim_of_new).  One host read: n_new and err."""
    lib = _lib.load()
    dev, F = faces.device, int(faces.shape[0])
    none = torch.empty(0, dtype=torch.int32, device=dev)
    if F and V == 0:
        _ma.raise_if(1)             # (faces without vertices: every index is outside the mesh)
    if F == 0:
        return faces, 0, none
    st = _host.stream_of(faces)
    counts = _edge_counts(faces, err)
    pairs = torch.empty(3 * F, 2, dtype=torch.int32, device=dev)
    on =torch.empty(V, dtype=torch.uint8, device=dev)
    degree = torch.empty(V, dtype=torch.int32, device=dev)
    slots = torch.empty(V, 2, dtype=torch.int32, device=dev)
    parent = torch.empty(V, dtype=torch.int32, device=dev)
    flag = torch.empty(V, dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_splice_rim_edges(F, V, _p(faces), _p(counts), _p(pairs), _p(on), _p(degree), _p(slots), _p(parent), _p(flag),
                                        _p(err), st), "gsr_splice_rim_edges")
    size = torch.empty(V, dtype=torch.int32, device=dev)
    bad = torch.empty(V, dtype=torch.int32, device=dev)
    new_faces = torch.empty(V, dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_splice_rim_census(V, _p(degree), _p(parent), _p(size), _p(bad), _p(new_faces), st), "gsr_splice_rim_census")
    scan = torch.cumsum(new_faces, 0, dtype=torch.int32)
    head = torch.cat([scan[-1:], err]).cpu()
    _ma.raise_if(int(head[1]))
    n_new = int(head[0])
    if n_new == 0:
        return faces, 0, none
    out = torch.empty(n_new, 3, dtype=torch.int32, device=dev)
    rim = torch.empty(n_new, dtype=torch.int32, device=dev)
    _lib.check(lib.gsr_splice_rim_emit(V, n_new, _p(new_faces), _p(scan), _p(slots), _p(out), _p(rim), st), "gsr_splice_rim_emit")
    return torch.cat([faces, out]), n_new, rim


@torch.no_grad()
def fill_small_holes(faces: torch.Tensor, n_verts: int) -> FilledMesh:
    """trimesh's fill_holes (refined_mesh.py:589, :617, :652) by one canonical rule.  faces [F,3] over n_verts vertices; vertex
    identity is the index.

    Boundary face-edges are those whose vertex pair exactly one face-edge of the mesh has (face_edge_counts == 1, trimesh's
    group_rows(edges_sorted, require_count=1)); each keeps the direction a -> b it has in its face.  Taken undirected they
    split the vertices they touch into components.  A component is a RIM iff every one of its vertices ends exactly two
    boundary edges; it is then a simple cycle of n vertices and n edges.  Rims with n == 3 or n == 4 are filled (trimesh's
    hole_to_faces); every other component is left as it is: longer rims, and components with a vertex of degree != 2.

    Let m be the rim's lowest vertex, x < y its two neighbours on the rim and, for a quad, o the vertex opposite m.  A triangle
    rim gives the face (m, x, y); a quad rim the faces A = (m, x, o) and B = (o, y, m), so the diagonal always passes through
    the lowest vertex.  A new face (a, b, c) is reversed to (a, c, b) iff the boundary face-edge between a and b runs a -> b in
    its own face -- trimesh's winding repair, which tests the new face's first edge only: the triangle and A on the edge m-x,
    B on the edge o-y, each on its own.  New faces are appended after the existing ones, rims in ascending m, A before B;
    existing faces and all vertices are untouched (the reference asserts the same, :618).  No new face is dropped on geometry:
    a rim's vertices are distinct indices, which is this project's definition of non-degenerate.

    The departure from trimesh, on purpose: trimesh's result follows networkx's cycle_basis traversal, which decides the
    diagonal of a quad, the order of the new faces, and what happens where two rims touch -- it may fill part of a component
    with a vertex of degree != 2, which stays untouched here.  Wherever trimesh's answer does not depend on the traversal the
    two agree.

    An index outside [0, n_verts) raises ValueError.  Host reads: n_new with the err word, and the watertight word."""
    faces = _ma.faces_i32(faces)
    V = int(n_verts)
    if V < 0:
        raise ValueError("n_verts must not be negative")
    with _host.on_device(faces.device):
        out, n_new, rim = _fill(faces, V, _ma.new_err(faces.device))
    return FilledMesh(faces=out, n_new=n_new, rim_of_new=rim, watertight=is_watertight(out))


# ------------------------------------------------------------------------------------------------ areas and means
def _mean_f64(x: torch.Tensor) -> torch.Tensor:
    """[1] float64 on the device: the mean of x [n > 0] float64 contiguous by the fixed-order reduction (the same bits every
    call).  Nothing is read."""
    lib = _lib.load()
    ws = torch.empty(int(lib.gsr_splice_workspace_bytes()) // 8 + 1, dtype=torch.float64, device=x.device)
    out = torch.empty(1, dtype=torch.float64, device=x.device)
    _lib.check(lib.gsr_splice_mean(int(x.shape[0]), _p(x), _p(ws), _p(out), _host.stream_of(x)), "gsr_splice_mean")
    return out


def _areas(verts: torch.Tensor, faces: torch.Tensor, err: torch.Tensor) -> torch.Tensor:
    F = int(faces.shape[0])
    area = torch.empty(F, dtype=torch.float64, device=faces.device)
    _lib.check(_lib.load().gsr_splice_face_areas(F, int(verts.shape[0]), _p(faces), _p(verts), _p(area), _p(err), _host.stream_of(faces)),
               "gsr_splice_face_areas")
    return area


@torch.no_grad()
def face_areas(verts: torch.Tensor, faces: torch.Tensor) -> torch.Tensor:
    """trimesh's area_faces (refined_mesh.py:683, :685): [F] float64.  On doubles converted from the f32 vertices, without
    contraction: u = v1 - v0, w = v2 - v1, c = u x w, area = 0.5 sqrt((cx cx + cy cy) + cz cz).  One host read: the err word."""
    verts, faces = _ma.mesh_f32(verts, faces)
    err = _ma.new_err(faces.device)
    with _host.on_device(faces.device):
        area = _areas(verts, faces, err)
    _ma.raise_if(int(err.cpu()))
    return area


@torch.no_grad()
def mean_edge_length(verts: torch.Tensor, faces: torch.Tensor) -> float:
    """The mean length of the mesh's unique edges in float64 (refined_mesh.py:484-485): each length sqrt((dx dx + dy dy) + dz dz)
    on the widened f32 coordinates, the mean by the fixed-order reduction.  NaN for a mesh without faces.  One host read."""
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, F = faces.device, int(faces.shape[0])
    if F == 0:
        return float("nan")
    err, st = _ma.new_err(dev), _host.stream_of(faces)
    with _host.on_device(dev):
        keys = _edge_keys(faces, None, None, 0, err, st)[1]
        _ma.raise_if(int(err.cpu()))                                 # (a negative index: its face's keys are the sentinel)
        keys = torch.unique(keys)
        n = int(keys.shape[0])
        length = torch.empty(n, dtype=torch.float64, device=dev)
        _lib.check(_lib.load().gsr_splice_edge_lengths(n, int(verts.shape[0]), _p(keys), _p(verts), _p(length), _p(err), st),
                   "gsr_splice_edge_lengths")
        head = torch.cat([_mean_f64(length), err.to(torch.float64)]).cpu()
    _ma.raise_if(int(head[1]))
    return float(head[0])


# ------------------------------------------------------------------------------------------------ the loop over the boxes
@dataclass
class TopologyUpdate:
    """What update_mesh_topology returns (refined_mesh.py:689-693).  verts [Nv,3] f32, faces [Nf,3] int32: the updated mesh;
    the surviving faces of the input mesh are a prefix of `faces`, in their original order.  track_face_mask [F0] bool: the
    input faces that survive; track_face_num: how many.  new_ref_area [Nf] f32 (:683-687): the INPUT mesh's areas for that
    prefix, and for all the other faces the mean area of those other faces (NaN when there are none); new_area_mean: that mean
    in float64; None when nothing_to_update.
    cc_update_num mirrors the reference: the regions selected BEFORE merging minus the boxes that failed (an empty cut or no
    boundary vertices, :586 / :601 / :611 / :620); a box skipped because its stitch is not watertight or too long still
    counts; -1 when no region was selected, 0 when every box failed.  n_spliced, this project's addition: the boxes that
    actually replaced the base mesh.  max_dist_in_connection: the running maximum of connect_two_meshes' max_dist, skipped
    boxes included (:633).
    face_origin [Nf] int32, where every face of `faces` came from: k >= 0 = face k of the input mesh (the prefix is therefore
    nonzero(track_face_mask)); -1 - k = face k of the fusion mesh; handover.FILLED (INT32_MIN) = a face made by
    fill_small_holes, at any of the three places it runs.  fusion_faces, fusion_n_verts: the fusion mesh face_origin indexes.
    Face colours are not carried by update_mesh_topology itself: with_colors() fills face_colors [Nf,4] and vertex_colors
    [Nv,4] uint8 from face_origin, and filled faces have none (0, 0, 0, 0)."""
    verts: torch.Tensor
    faces: torch.Tensor
    track_face_mask: torch.Tensor
    track_face_num: int
    new_ref_area: Optional[torch.Tensor]
    new_area_mean: float
    cc_update_num: int
    n_spliced: int
    max_dist_in_connection: float
    nothing_to_update: bool
    face_origin: Optional[torch.Tensor] = None
    fusion_faces: Optional[torch.Tensor] = None
    fusion_n_verts: int = 0
    face_colors: Optional[torch.Tensor] = None
    vertex_colors: Optional[torch.Tensor] = None

    def with_colors(self, base_face_rgba: torch.Tensor, fusion_vertex_colors: torch.Tensor) -> "TopologyUpdate":
        """Carry colour through the update, as the reference carries face_colors through connect_two_meshes
        (refined_mesh.py:183).  base_face_rgba [F0,4] uint8: the input mesh's face colours
        (harness.SurfaceGaussians.color_mesh); fusion_vertex_colors [Vf,>=3] in [0,1] (fusion.FusionMesh.colors).  Fills
        face_colors [Nf,4] uint8 -- an input face keeps its colour, a fusion face gets handover.vertex_to_face_colors of its
        vertices, a filled face (0, 0, 0, 0) -- and vertex_colors [Nv,4] uint8 = handover.face_to_vertex_colors of them, what
        save() writes.  Every vertex of a filled face lies on a rim, so it has a coloured face.  -> self.

        Two departures from trimesh, on purpose (handover's docstring): its fill_holes gives new faces a library default
        colour, which would tint the rim vertices -- here filled faces carry none and are left out of the mean; and the
        roundings of the two conversions are this project's statement of trimesh's, whose parity is not pinned (trimesh is not
        a dependency)."""
        from . import handover
        if self.face_origin is None or self.fusion_faces is None:
            raise ValueError("this TopologyUpdate has no face_origin: it was not made by update_mesh_topology")
        if base_face_rgba.shape[0] != self.track_face_mask.shape[0]:
            raise ValueError("base_face_rgba must have one row per face of the input mesh")
        if fusion_vertex_colors.shape[0] != self.fusion_n_verts:
            raise ValueError("fusion_vertex_colors must have one row per vertex of the fusion mesh")
        self.face_colors = handover.gather_face_colors(self.face_origin, base_face_rgba, self.fusion_faces, fusion_vertex_colors)
        self.vertex_colors = handover.face_to_vertex_colors(self.faces, self.face_colors, int(self.verts.shape[0]))
        return self

    def save(self, directory: str) -> Tuple[str, str]:
        """updated_mesh.obj (formats.save_obj) and face_corr.npz with the keys track_face_mask and ref_area
        (np.savez_compressed), as refine.py:315-323 loads them (refined_mesh.py:1055-1060).  With vertex_colors set
        (with_colors) the vertex lines are `v x y z r g b`, the colours u8 / 255 in float64."""
        from . import formats
        if self.new_ref_area is None:
            raise ValueError("nothing was updated: there is no mesh to save")
        os.makedirs(directory, exist_ok=True)
        obj, npz = os.path.join(directory, "updated_mesh.obj"), os.path.join(directory, "face_corr.npz")
        colours = None if self.vertex_colors is None else self.vertex_colors[:, :3].cpu().numpy().astype(np.float64) / 255.0
        formats.save_obj(obj, self.verts.cpu().numpy(), self.faces.cpu().numpy(), colours)
        np.savez_compressed(npz, track_face_mask=self.track_face_mask.cpu().numpy(), ref_area=self.new_ref_area.cpu().numpy())
        return obj, npz

    def gaussian_mask(self, G: int) -> torch.Tensor:
        """[F0 G] bool: track_face_mask repeated G times per face (refine.py:382, pre_sh_mask)."""
        return self.track_face_mask.repeat_interleave(int(G))


def _patch_for_box(patch: CutMesh, box, outlier_face_threshold, fill: bool, err: Optional[torch.Tensor] = None):
    """Step 1 of update_mesh_topology's docstring after the cut, on a patch that is not empty: with `fill` fill_small_holes (err:
    its word), the outlier mask, select_faces (patch.attrs follow), the boundary vertices across the box.  -> (the selected
    patch, its boundary -- none: the box fails --, the outlier mask over the patch's faces and the n_new filled ones, n_new)."""
    pf, n_new, _rim = _fill(patch.faces, int(patch.verts.shape[0]), err) if fill else (patch.faces, 0, None)
    keep = outlier_component_mask(pf, outlier_face_threshold)
    patch = select_faces(patch.verts, pf, keep, attrs=patch.attrs)
    return patch, boundary_vertices(patch.verts, patch.faces, box, cut_inner=False), keep, n_new


def _base_for_box(cut: CutMesh, box, pad: float, fill: bool, err: Optional[torch.Tensor] = None):
    """Step 2 after the cut, on a base cut that is not empty: with `fill` fill_small_holes, the boundary vertices inside the box
    grown by `pad`.  -> (the cut's faces and the n_new filled ones, the boundary -- none: the box fails --, n_new)."""
    cf, n_new, _rim = _fill(cut.faces, int(cut.verts.shape[0]), err) if fill else (cut.faces, 0, None)
    return cf, boundary_vertices(cut.verts, cf, box, cut_inner=True, pad=pad), n_new


@torch.no_grad()
def update_mesh_topology(verts: torch.Tensor, faces: torch.Tensor, update_regions: UpdateRegions, fusion_mesh, aabb_pad: float = 0.02,
                         outlier_face_threshold=50, force_watertight: bool = True, force_short_edge: bool = False,
                         max_hole_vert_num: int = 10) -> TopologyUpdate:
    """The loop of update_mesh_topo over the merged boxes (refined_mesh.py:578-693) on device tensors.  fusion_mesh: an object
    with .verts [Vf,3] f32 and .faces [Ff,3] (fusion.FusionMesh).  Per box of update_regions.boxes(aabb_pad), in order:
      1. the patch is cut from the WHOLE fusion mesh (:583); empty: the box fails (:586).  fill_small_holes (:589), the outlier
         mask and select_faces (:590-599), its boundary vertices across the box (:600); none: the box fails.
      2. the CURRENT base mesh -- what the previous boxes left -- is cut with cut_inner=True (:609); empty: fails.
         fill_small_holes (:617), then the boundary vertices of the FILLED mesh inside the box grown by 0.02 (:619); none: fails.
      3. connect_two_meshes (:628); max_dist joins the running maximum whatever happens next (:633).
      4. force_watertight and a stitch that is not watertight: the box is skipped (:639-643).
      5. force_short_edge and max_dist > 6 x the mean unique-edge length of the input mesh (:484-485, :645): skipped.
      6. otherwise fill_small_holes on the stitch (:652), the box's mask over the current base mesh's faces from the cut's mask
         and the stitch's mask before the base cut's filling (:656-658), base = stitched (:660), and
         track_face_mask[track_face_mask] = that mask's first track_face_num entries (:663-664).
    Then the reference areas (:683-687).  See TopologyUpdate for cc_update_num and n_spliced."""
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, F0 = faces.device, int(faces.shape[0])
    fv, ff = _ma.verts_f32(fusion_mesh.verts, dev), _ma.faces_i32(fusion_mesh.faces)
    track = torch.ones(F0, dtype=torch.bool, device=dev)
    # face_origin follows the masks the loop has anyway: the cuts' face_mask, the outlier mask, the stitch's face_mask over the
    # concatenation, and a run of FILLED behind every filling
    origin = torch.arange(F0, dtype=torch.int32, device=dev)
    Vf = int(fv.shape[0])
    if update_regions.nothing_to_update:
        return TopologyUpdate(verts, faces, track, F0, None, float("nan"), -1, 0, 0.0, True, origin, ff, Vf)
    filled_run = lambda n: torch.full((n,), -2 ** 31, dtype=torch.int32, device=dev)
    edge_len = mean_edge_length(verts, faces) if force_short_edge else None
    base_v, base_f, track_num = verts, faces, F0
    failed, n_spliced, max_dist = 0, 0, 0.0
    err = _ma.new_err(dev)
    with _host.on_device(dev):
        for box in update_regions.boxes(aabb_pad):
            patch = cut_mesh_by_box(fv, ff, box, False)
            if patch.verts.shape[0] == 0:
                failed += 1
                continue
            p_cut = -1 - torch.nonzero(patch.face_mask).view(-1).to(torch.int32)
            patch, pb, p_keep, p_new = _patch_for_box(patch, box, outlier_face_threshold, True, err)
            p_origin = torch.cat([p_cut, filled_run(p_new)])[p_keep]
            if pb.shape[0] == 0:
                failed += 1
                continue
            cut = cut_mesh_by_box(base_v, base_f, box, True)
            if cut.verts.shape[0] == 0:
                failed += 1
                continue
            n_cut = int(cut.faces.shape[0])
            cf, bb, c_new = _base_for_box(cut, box, 0.02, True, err)
            if bb.shape[0] == 0:
                failed += 1
                continue
            st = connect_two_meshes(cut.verts, cf, bb, patch.verts, patch.faces, pb, max_hole_vert_num)
            max_dist = max(max_dist, st.max_dist)
            if force_watertight and not st.watertight:
                continue
            if force_short_edge and st.max_dist > 6 * edge_len:
                continue
            filled, s_new, _rim = _fill(st.faces, int(st.verts.shape[0]), err)
            mask_cc = compose_face_mask(cut.face_mask, st.face_mask[:n_cut])
            origin = torch.cat([torch.cat([origin[cut.face_mask], filled_run(c_new), p_origin])[st.face_mask], filled_run(s_new)])
            base_v, base_f = st.verts, filled
            track = compose_face_mask(track, mask_cc[:track_num])
            track_num = int(track.sum().cpu())
            n_spliced += 1
        Fn = int(base_f.shape[0])
        ref_area = torch.empty(Fn, dtype=torch.float32, device=dev)
        ref_area[:track_num] = _areas(verts, faces, err)[track].to(torch.float32)
        mean = float("nan")
        if Fn > track_num:
            rest = _areas(base_v, base_f, err)[track_num:].contiguous()
            m = _mean_f64(rest)
            ref_area[track_num:] = m.to(torch.float32)
            head = torch.cat([m, err.to(torch.float64)]).cpu()
            mean = float(head[0])
            _ma.raise_if(int(head[1]))
        else:
            _ma.raise_if(int(err.cpu()))
    return TopologyUpdate(verts=base_v, faces=base_f, track_face_mask=track, track_face_num=track_num, new_ref_area=ref_area,
                          new_area_mean=mean, cc_update_num=update_regions.n_regions - failed, n_spliced=n_spliced,
                          max_dist_in_connection=float(max_dist), nothing_to_update=False, face_origin=origin, fusion_faces=ff,
                          fusion_n_verts=Vf)


def load_tracking(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """(track_face_mask [F0] bool, ref_area [Nf] f32) from the face_corr.npz TopologyUpdate.save wrote (refine.py:315-323)."""
    with np.load(path) as z:
        return z["track_face_mask"].astype(bool), z["ref_area"].astype(np.float32)


def choose_aabb_pad(run: Callable[[float], TopologyUpdate], pads: Sequence[float] = (0.01, 0.015, 0.02, 0.025, 0.03)):
    """The aabb_pad trials of refined_mesh.py:1034-1048.  run(pad) -> an object with cc_update_num, max_dist_in_connection and
    nothing_to_update.  Every pad scores 100 unless its run has cc_update_num > 0, then its max_dist_in_connection; the trials
    stop at the first run with nothing_to_update.  -> (the pad of the lowest score -- np.argmin, so the first among equals --
    or None when there was nothing to update, the scores as a list)."""
    pads = [float(p) for p in pads]
    scores = [100.0] * len(pads)
    for i, pad in enumerate(pads):
        out = run(pad)
        if out.nothing_to_update:
            return None, scores
        if out.cc_update_num > 0:
            scores[i] = float(out.max_dist_in_connection)
    return pads[int(np.argmin(np.asarray(scores, np.float64)))], scores


__all__ = ["MAX_FACES", "face_edge_counts", "face_components", "combine_overlap_aabbs", "UpdateRegions", "select_update_regions",
           "CutMesh", "RegionCut", "cut_mesh_by_box", "boundary_vertices", "outlier_component_mask", "NN_TILE", "NN_QUERIES",
           "nearest_vertices", "select_faces", "is_watertight", "merge_vertices_around_holes", "StitchedMesh", "connect_two_meshes",
           "compose_face_mask", "RegionStitch", "FilledMesh", "fill_small_holes", "face_areas", "mean_edge_length", "TopologyUpdate",
           "update_mesh_topology", "choose_aabb_pad", "load_tracking"]
