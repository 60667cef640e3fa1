"""Quadric mesh decimation and Laplacian / Taubin smoothing on the GPU: what extract_mesh_fusion's `simplify_face_num` and
`smooth` do with Open3D (gaustar_trainers/refined_mesh.py:451-458), the Taubin filter of the reference's tools
(gaustar_tools/internal_use_tools/fusion_depth.py:80-84, mesh_smoothing.py) and the decimation that makes the base mesh every
sequence starts from, `init_mesh_100k.obj` (pyfqmr's simplify_mesh, gaustar_tools/cmr_convert.py:262-266).

    small = simplify_mesh(verts, faces, target_faces, locked=None, attrs=(colors,))     # SimplifiedMesh
    verts = smooth_laplacian(verts, faces, iterations=10, lambda_filter=0.5)
    verts = smooth_taubin(verts, faces, iterations=10, lambda_filter=0.5, mu=-0.53)
    python -m gaustar_amd.remesh IN.obj OUT.obj --faces N [--smooth K] [--taubin K]     # how to make an init_mesh_100k.obj

The meshes stay device tensors; the passes are HIP kernels (include/gsr.h, csrc/gsr_remesh.hip), the sorts, scans and the final
compaction torch's and gaustar_amd.regions'.  Geometry is f64 without contraction, every sum has one stated order and nothing
uses float atomics: the same inputs give the same bits, the bits the numpy restatement tests/remesh_ref.py gives.

Decimation is this project's own statement of Garland-Heckbert: a round-based parallel edge collapse, because a priority
queue does not map to the GPU.

Once: P = the f64 copy of the f32 vertices.  Every face gets the quadric K_f = A p p^T with p = (n / |n|, -(n / |n|) . x0),
n = (x1 - x0) x (x2 - x0), A = |n| / 2 (10 values; zeros where |n| is not > 0), every vertex Q_v = the sum of its faces' K_f in
ascending face order (the order of MeshTopology.vertex_face_csr).

One round over the live faces:
 1. Edges.  The unique edges and their multiplicities from one sort of min << 32 | max keys; an edge's id is its rank.  A
    vertex is FIXED if `locked` names it or if it lies on an edge that is not manifold, i.e. that other than exactly two
    face-edges of two different faces have (a boundary, a fin).  Fixed vertices are never moved or removed, so a cut patch's
    boundary list stays valid after decimation.
 2. Candidates.  Edge (u, v), u < v, is one iff it is manifold, both ends are free, the link condition holds, the cost rounds
    to a finite f32 and no face is turned over.  Link condition: with a, b the corners opposite the edge in its two faces,
    a != b, the vertices that share a face with u and a face with v are a and b only, and the mesh does not hold both a face
    {u, a, b} and a face {v, a, b} (which is all that stops a tetrahedron from folding flat).  Placement: Q = Q_u + Q_v; with
    the 3x3 system's determinant by cofactors along its first row, Cramer's rule where |det| > 1e-10 s^3 (s = the largest
    absolute entry of the 3x3), else the cheapest of P_u, P_v and 0.5 (P_u + P_v), the earlier on ties.  cost = max(x^T Q x, 0),
    rows first: r_i = ((q_i0 x + q_i1 y) + q_i2 z) + q_i3, cost = ((x r0 + y r1) + z r2) + r3.  Flip test: for every face of u
    or v other than the edge's two, n_before . n_after < 0 rejects, and so does == 0 unless n_before == 0 (a face that is
    already degenerate does not block, so marching-cubes slivers can go).
 3. Independent set.  key = f32(cost) bits << 32 | edge id; m1[v] = min key over the candidate edges at v; m2[v] = min over
    ALL edges (v, w) of min(m1[v], m1[w]); an edge is selected iff m2[u] == m2[v] == key (three passes of integer atomicMin).
    No face touches two selected edges and no selected collapse moves a vertex another one's tests read.
 4. Cap.  The selected keys are sorted; only the cheapest (F_live - target + 1) // 2 are applied.
 5. Apply.  u survives at the placement with Q_u + Q_v (added in that order); every attribute becomes (a_u + a_v) * 0.5f; v
    becomes u in every face; the edge's two faces die.  A face keeps its identity, hence face_origin.
Rounds repeat until F_live <= target or a round selects nothing (stalled).  One small host read per round: the number of
selected edges (and the err word).  At the end dead faces and unreferenced vertices go, in ascending order, and the positions
are rounded to f32.  For a closed manifold input an unstalled result has target or target - 1 faces and is a closed manifold of
the same Euler characteristic.

Smoothing: new = prev + lambda (sum w_n prev_n / sum w_n - prev) over the vertex_neighbours list in ascending order, in f64,
ping-pong; w_n = 1 / (|prev - prev_n| + 1e-12) ("inverse_distance") or 1 ("uniform").  A vertex without neighbours or under
`locked` keeps its position.  Laplacian: `iterations` steps with lambda_filter; Taubin: `iterations` pairs of a lambda step and
a mu step.

Stated departures: parity with Open3D or pyfqmr is NOT pinned (neither is a dependency, neither's sources were at hand; the
inverse-distance weight is what is recalled of Open3D's helper); boundary vertices are fixed where Open3D weights boundary
planes; edges are ranked by the f32-rounded cost; only positions are smoothed, where Open3D's filters also average colours and
normals.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Optional, Sequence, Tuple

import numpy as np
import torch

from . import _host, _lib, _meshargs as _ma, regions
from ._lib import ptr as _p
from .meshes import MeshTopology

WEIGHTS = ("inverse_distance", "uniform")
_SENTINEL = 2 ** 63 - 1


@dataclass
class SimplifiedMesh:
    """verts [Nv,3] f32, faces [Nf,3] int32, face_origin [Nf] int32 (the input face every output face is, as
    regions.TopologyUpdate.face_origin's input entries), attrs (the per-vertex arrays given, merged and gathered), n_rounds
    (rounds that collapsed something), stalled (no legal collapse was left above the target)."""
    verts: torch.Tensor
    faces: torch.Tensor
    face_origin: torch.Tensor
    attrs: Tuple[torch.Tensor, ...]
    n_rounds: int
    stalled: bool


def _locked_u8(locked: Optional[torch.Tensor], V: int, dev) -> Optional[torch.Tensor]:
    if locked is None:
        return None
    if tuple(locked.shape) != (V,) or locked.dtype not in (torch.bool, torch.uint8):
        raise ValueError("locked must be [V] bool or uint8")
    if locked.device != dev:
        raise RuntimeError("locked and the mesh must be on the same GPU")
    return (locked != 0).to(torch.uint8).contiguous()


def _f32_attrs(attrs: Sequence[torch.Tensor], V: int, dev) -> Tuple[torch.Tensor, ...]:
    attrs = tuple(attrs)
    for a in attrs:
        if a.dim() < 1 or a.shape[0] != V or a.dtype != torch.float32 or a.device != dev:
            raise ValueError("attrs must be per-vertex float32 arrays [V, ...] on the mesh's GPU")
    return attrs


class _Round:
    """The buffers of the rounds and one round's launches (simplify_mesh has made the mesh's device the current one)."""

    def __init__(self, verts: torch.Tensor, faces: torch.Tensor, locked: Optional[torch.Tensor], attrs):
        self.lib = _lib.load()
        dev = faces.device
        self.dev, self.F, self.V = dev, int(faces.shape[0]), int(verts.shape[0])
        F, V = self.F, self.V
        self.faces = faces.clone()
        self.attrs = tuple(a.detach().clone().contiguous() for a in attrs)
        self.locked = locked
        self.err = _ma.new_err(dev)
        self.pos = torch.empty(V, 3, dtype=torch.float64, device=dev)
        self.live = torch.empty(F, dtype=torch.int32, device=dev)
        self.quadric = torch.empty(V, 10, dtype=torch.float64, device=dev)
        self.ekeys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        self.ckeys = torch.empty(3 * F, dtype=torch.int64, device=dev)
        self.degree = torch.empty(V, dtype=torch.int32, device=dev)
        self.offsets = torch.zeros(V + 1, dtype=torch.int32, device=dev)
        self.fixed = torch.empty(V, dtype=torch.uint8, device=dev)
        self.m1 = torch.empty(V, dtype=torch.int64, device=dev)
        self.m2 = torch.empty(V, dtype=torch.int64, device=dev)
        st = _host.stream_of(faces)
        face_quadric = torch.empty(F, 10, dtype=torch.float64, device=dev)
        _lib.check(self.lib.gsr_remesh_setup(F, V, _p(verts), _p(self.faces), _p(self.pos), _p(self.live), _p(face_quadric), _p(self.err),
                                             st), "gsr_remesh_setup")
        self.corners = self._vertex_faces(st)
        self.stale = False                                # (the keys and lists are those of self.faces as they are)
        _lib.check(self.lib.gsr_remesh_vertex_quadrics(F, V, _p(self.offsets), _p(self.corners), _p(face_quadric), _p(self.quadric), st),
                   "gsr_remesh_vertex_quadrics")

    def _vertex_faces(self, st) -> torch.Tensor:
        """The keys of the faces as they are: self.ekeys, and -> the sorted corner keys with self.offsets their vertices' ranges."""
        _lib.check(self.lib.gsr_remesh_keys(self.F, self.V, _p(self.faces), _p(self.live), _p(self.ekeys), _p(self.ckeys),
                                            _p(self.degree), st), "gsr_remesh_keys")
        torch.cumsum(self.degree, 0, dtype=torch.int32, out=self.offsets[1:])
        return torch.sort(self.ckeys)[0]

    def select(self, n_live: int):
        """One round up to the independent set -> (state for apply, sorted selected keys, their number: one host read)."""
        lib, V, F = self.lib, self.V, self.F
        st = _host.stream_of(self.faces)
        if self.stale:
            self.corners = self._vertex_faces(st)
            self.stale = False
        corners = self.corners
        n = 3 * n_live                                    # the live face-edges sort in front of the dead ones' sentinels
        skeys, order = torch.sort(self.ekeys, stable=True)
        head = torch.empty(n, dtype=torch.int32, device=self.dev)
        _lib.check(lib.gsr_remesh_edge_heads(n, _p(skeys), _p(head), st), "gsr_remesh_edge_heads")
        scan = torch.cumsum(head, 0, dtype=torch.int32)
        n_edges = scan[-1:]
        euv = torch.empty(n, 2, dtype=torch.int32, device=self.dev)
        manifold = torch.empty(n, dtype=torch.uint8, device=self.dev)
        if self.locked is None:
            self.fixed.zero_()
        else:
            self.fixed.copy_(self.locked)
        _lib.check(lib.gsr_remesh_edges(n, V, _p(skeys), _p(order), _p(scan), _p(euv), _p(manifold), _p(self.fixed), st),
                   "gsr_remesh_edges")
        key = torch.empty(n, dtype=torch.int64, device=self.dev)
        placement = torch.empty(n, 3, dtype=torch.float64, device=self.dev)
        _lib.check(lib.gsr_remesh_candidates(n, _p(n_edges), F, V, _p(euv), _p(manifold), _p(self.fixed), _p(self.offsets), _p(corners),
                                             _p(self.faces), _p(self.pos), _p(self.quadric), _p(key), _p(placement), st),
                   "gsr_remesh_candidates")
        selected = torch.empty(n, dtype=torch.int64, device=self.dev)
        _lib.check(lib.gsr_remesh_select(n, _p(n_edges), V, _p(euv), _p(key), _p(self.m1), _p(self.m2), _p(selected), st),
                   "gsr_remesh_select")
        ranked = torch.sort(selected)[0]
        word = torch.cat([(ranked != _SENTINEL).sum(dtype=torch.int64).view(1), self.err.to(torch.int64)]).cpu()
        _ma.raise_if(int(word[1]))
        return (n, n_edges, euv, placement, corners, selected), ranked, int(word[0])

    def apply(self, state, ranked: torch.Tensor, n_apply: int) -> None:
        n, n_edges, euv, placement, corners, selected = state
        st = _host.stream_of(self.faces)
        threshold = ranked[n_apply - 1:n_apply]
        for a in self.attrs:
            C = int(a.numel() // self.V)
            if C:
                _lib.check(self.lib.gsr_remesh_apply_attr(n, _p(n_edges), self.V, C, _p(selected), _p(threshold), _p(euv), _p(a), st),
                           "gsr_remesh_apply_attr")
        _lib.check(self.lib.gsr_remesh_apply(n, _p(n_edges), self.F, self.V, _p(selected), _p(threshold), _p(euv), _p(placement),
                                             _p(self.offsets), _p(corners), _p(self.faces), _p(self.live), _p(self.pos),
                                             _p(self.quadric), st), "gsr_remesh_apply")
        self.stale = True


def _identity(verts: torch.Tensor, faces: torch.Tensor, attrs) -> SimplifiedMesh:
    origin = torch.arange(int(faces.shape[0]), dtype=torch.int32, device=faces.device)
    return SimplifiedMesh(verts=verts, faces=faces, face_origin=origin, attrs=tuple(attrs), n_rounds=0, stalled=False)


@torch.no_grad()
def simplify_mesh(verts: torch.Tensor, faces: torch.Tensor, target_faces: int, locked: Optional[torch.Tensor] = None,
                  attrs: Sequence[torch.Tensor] = ()) -> SimplifiedMesh:
    """Quadric decimation of (verts [V,3] f32, faces [F,3] int32 / int64) to at most `target_faces` faces, by the rules of the
    module docstring: Open3D's simplify_quadric_decimation (refined_mesh.py:456-458) and pyfqmr's simplify_mesh
    (cmr_convert.py:262-266), without pinned parity to either.  locked [V] bool: vertices never moved or removed (boundary and
    non-manifold vertices are fixed anyway).  attrs: per-vertex float32 arrays [V, ...] (the fusion's colours); a merged vertex
    takes the mean of its two.  target_faces >= F returns the input unchanged with the identity face_origin and 0 rounds.
    The inputs are not modified.  Host reads: one per round (the number of selected edges and the err word), then the
    compaction's totals.  A face with a vertex index outside [0, V) raises ValueError."""
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, F, V = faces.device, int(faces.shape[0]), int(verts.shape[0])
    target = int(target_faces)
    if target < 0:
        raise ValueError("target_faces must not be negative")
    attrs = _f32_attrs(attrs, V, dev)
    locked = _locked_u8(locked, V, dev)
    if target >= F:
        return _identity(verts, faces, attrs)
    if V == 0:
        _ma.raise_if(1)                         # (faces without vertices: every index is outside the mesh)
    n_live, n_rounds, stalled = F, 0, False
    n_apply = ctypes.c_int(0)
    with _host.on_device(dev):
        rd = _Round(verts, faces, locked, attrs)
        while n_live > target:
            state, ranked, n_selected = rd.select(n_live)
            _lib.check(rd.lib.gsr_remesh_cap(n_live, target, n_selected, ctypes.byref(n_apply)), "gsr_remesh_cap")
            if n_apply.value == 0:
                stalled = True
                break
            rd.apply(state, ranked, n_apply.value)
            n_live -= 2 * n_apply.value
            n_rounds += 1
        out = torch.empty(V, 3, dtype=torch.float32, device=dev)
        _lib.check(rd.lib.gsr_remesh_narrow(3 * V, _p(rd.pos), _p(out), _host.stream_of(out)), "gsr_remesh_narrow")
        cut, _scan = regions._compact(out, rd.faces, None, (rd.live != 0).to(torch.uint8), rd.attrs, rd.err)
    origin = torch.nonzero(cut.face_mask).view(-1).to(torch.int32)
    return SimplifiedMesh(verts=cut.verts, faces=cut.faces, face_origin=origin, attrs=cut.attrs, n_rounds=n_rounds, stalled=stalled)


def _smooth(verts: torch.Tensor, faces: torch.Tensor, steps: int, lam_even: float, lam_odd: float, weights: str,
            locked: Optional[torch.Tensor]) -> torch.Tensor:
    if weights not in WEIGHTS:
        raise ValueError(f"weights must be one of {WEIGHTS}")
    if steps < 0:
        raise ValueError("iterations must not be negative")
    verts, faces = _ma.mesh_f32(verts, faces)
    dev, V = faces.device, int(verts.shape[0])
    locked = _locked_u8(locked, V, dev)
    if V == 0 or steps == 0:
        return verts.clone()
    try:
        off, nbr = MeshTopology.of(faces, V).vertex_neighbours
    except IndexError:
        _ma.raise_if(1)
    work = torch.empty(2, V, 3, dtype=torch.float64, device=dev)
    out = torch.empty(V, 3, dtype=torch.float32, device=dev)
    with _host.on_device(dev):
        _lib.check(_lib.load().gsr_remesh_smooth(V, _p(off), _p(nbr), _p(locked), int(steps), float(lam_even), float(lam_odd),
                                                 int(weights == "uniform"), _p(verts), _p(work[0]), _p(work[1]), _p(out), _host.stream_of(out)),
                   "gsr_remesh_smooth")
    return out


@torch.no_grad()
def smooth_laplacian(verts: torch.Tensor, faces: torch.Tensor, iterations: int = 10, lambda_filter: float = 0.5,
                     weights: str = "inverse_distance", locked: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Open3D's filter_smooth_laplacian (refined_mesh.py:451-453) on the positions: `iterations` sweeps of the module
    docstring's update with lambda_filter -> verts [V,3] f32.  The inputs are not modified; nothing is read back."""
    return _smooth(verts, faces, int(iterations), lambda_filter, lambda_filter, weights, locked)


@torch.no_grad()
def smooth_taubin(verts: torch.Tensor, faces: torch.Tensor, iterations: int = 10, lambda_filter: float = 0.5, mu: float = -0.53,
                  weights: str = "inverse_distance", locked: Optional[torch.Tensor] = None) -> torch.Tensor:
    """Open3D's filter_smooth_taubin (fusion_depth.py:80-84): `iterations` pairs of a lambda_filter sweep and a mu sweep, which
    shrink the shape far less than Laplacian smoothing does -> verts [V,3] f32."""
    return _smooth(verts, faces, 2 * int(iterations), lambda_filter, mu, weights, locked)


def main(argv=None) -> int:
    """python -m gaustar_amd.remesh IN.obj OUT.obj --faces N [--smooth K] [--taubin K]: smooth (Laplacian sweeps, then Taubin
    pairs), then decimate to N faces; vertex colours, where the file has them, are carried as an attribute."""
    import argparse

    from . import formats
    ap = argparse.ArgumentParser(prog="python -m gaustar_amd.remesh", description=main.__doc__)
    ap.add_argument("src")
    ap.add_argument("dst")
    ap.add_argument("--faces", type=int, required=True, help="the face count to decimate to")
    ap.add_argument("--smooth", type=int, default=0, metavar="K", help="Laplacian sweeps before the decimation")
    ap.add_argument("--taubin", type=int, default=0, metavar="K", help="Taubin pairs before the decimation")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    v, f, c = formats.load_obj(args.src)
    dev = torch.device(args.device)
    verts = torch.from_numpy(np.ascontiguousarray(v, np.float32)).to(dev)
    faces = torch.from_numpy(np.ascontiguousarray(f, np.int32)).to(dev)
    attrs = () if c is None or c.shape[1] == 0 else (torch.from_numpy(np.ascontiguousarray(c, np.float32)).to(dev),)
    if args.smooth > 0:
        verts = smooth_laplacian(verts, faces, iterations=args.smooth)
    if args.taubin > 0:
        verts = smooth_taubin(verts, faces, iterations=args.taubin)
    res = simplify_mesh(verts, faces, args.faces, attrs=attrs)
    formats.save_obj(args.dst, res.verts.cpu().numpy(), res.faces.cpu().numpy(), res.attrs[0].cpu().numpy() if attrs else None)
    print(f"{args.dst}: {int(res.faces.shape[0])} faces, {int(res.verts.shape[0])} vertices, {res.n_rounds} rounds"
          + (", stalled" if res.stalled else ""))
    return 0


__all__ = ["SimplifiedMesh", "simplify_mesh", "smooth_laplacian", "smooth_taubin", "WEIGHTS"]

if __name__ == "__main__":
    raise SystemExit(main())
